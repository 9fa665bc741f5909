// Implicit-GEMM convolution for gfx950: NHWC bf16, MFMA
// 16x16x32, LDS-staged double-buffered tiles, fp32 accumulation.
//
// GEMM view of conv fwd: C[M, Kg] = A[M, R*S*Cg] @ B[Kg, R*S*Cg]^T per group,
// where M = N*Ho*Wo output pixels, A rows are gathered input patches (NHWC
// makes each (r, s-span) contiguous in memory) and B is the weight tensor in
// its [K][R][S][C] channels_last layout (already reduction-contiguous).
//
// The same kernel computes dgrad: conv_fwd(dilate(gy), flipT(w)) — the Python
// wrapper materializes the transformed weight [C,R,S,K] and zero-dilated gy,
// and the kernel writes into a larger (HoA, WoA)-strided output region to
// honor output_padding. Linear layers are the R=S=1, H=W=1 case.
//
// Tile: BM=128 x BN=128 x BK=32, 4 waves (2x2), each wave 64x64 via 4x4
// fragments of mfma_f32_16x16x32_bf16. Register-staged global->LDS with
// boundary predication (zero-fill); one-step software pipeline (T14 G15:
// loads for step k+1 issued before compute of step k, LDS write after the
// barrier).
#include "conv_common.h"
#include "conv_route.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDS_K = BK + 8;  // +8 bf16 pad: break 64B-row bank alignment

struct ConvParams {
  const __hip_bfloat16* x;  // [N,H,W,Ct] NHWC
  const __hip_bfloat16* w;  // [Kt,R,S,Cg]
  __hip_bfloat16* y;        // [N,HoA,WoA,Kt] NHWC
  int N, H, W, Ct;          // Ct = total input channels
  int Kt;                   // total output channels
  int R, S, Cg, Kg;         // per-group
  int sh, sw, ph, pw, dh, dw;
  int Ho, Wo;               // logical output (M = N*Ho*Wo)
  int HoA, WoA;             // allocated output strides (>= Ho,Wo)
  int osh, osw;             // output position multipliers (dgrad-s2 scatter)
  int oh0, ow0;             // output position base offsets (parity classes)
  int M, nspan, ksteps;     // nspan = ceil(S*Cg/BK), ksteps = R*nspan
  int tiles_m;              // for XCD swizzle
  float* part;              // EMIT: [tiles_m*2, 2*Kt] BN sum/sumsq partials
};

// EMIT: epilogue also writes the forward BN sum/sumsq partials.
// ACC: epilogue accumulates into y (residual-fork dgrad into gres).
template <bool EMIT, bool ACC = false>
__global__ __launch_bounds__(256) void conv_igemm_fwd_kernel(ConvParams p) {
  static_assert(!(ACC && EMIT), "ACC only with plain epilogue");
  const int g = blockIdx.z;
  // XCD-aware swizzle over m-tiles (T1; bijective form)
  int tile_m = blockIdx.x, tile_n = blockIdx.y;
  {
    const int nwg = p.tiles_m;
    const int q = nwg / 8, r8 = nwg % 8;
    const int xcd = tile_m % 8, idx = tile_m / 8;
    tile_m = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + idx;
  }

  __shared__ __hip_bfloat16 ldsA[2][BM][LDS_K];
  __shared__ __hip_bfloat16 ldsB[2][BN][LDS_K];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;  // 2x2 wave grid
  const int il = lane & 15, kg = lane >> 4;

  // ---- per-thread staging coordinates (fixed across k-steps) ----
  // Each thread stages 2 rows of A and 2 rows of B per k-step (rows t/4 and
  // t/4+64), 8 contiguous elements each at span offset (t%4)*8.
  const int srow = tid >> 2;           // 0..63
  const int scol8 = (tid & 3) << 3;    // 0,8,16,24
  int an[2], ahbase[2], awbase[2];
  bool arow_ok[2];
#pragma unroll
  for (int pss = 0; pss < 2; ++pss) {
    const int m = tile_m * BM + srow + pss * 64;
    arow_ok[pss] = m < p.M;
    const int mm = arow_ok[pss] ? m : 0;
    const int n = mm / (p.Ho * p.Wo);
    const int rem = mm % (p.Ho * p.Wo);
    an[pss] = n;
    ahbase[pss] = (rem / p.Wo) * p.sh - p.ph;
    awbase[pss] = (rem % p.Wo) * p.sw - p.pw;
  }
  const int SCg = p.S * p.Cg;
  int bk[2];
  bool brow_ok[2];
#pragma unroll
  for (int pss = 0; pss < 2; ++pss) {
    const int k = tile_n * BN + srow + pss * 64;
    brow_ok[pss] = k < p.Kg;
    bk[pss] = g * p.Kg + (brow_ok[pss] ? k : 0);
  }

  // ---- staging helpers -----------------------------------------------------
  // loads for k-step ks into registers
  uint4 regA[2], regB[2];
  auto stage_load = [&](int ks) {
    const int r = ks / p.nspan;
    const int span0 = (ks % p.nspan) * BK;
    const int span = span0 + scol8;
    const bool span_ok = span < SCg;
    const int s = span_ok ? span / p.Cg : 0;
    const int c = span - s * p.Cg;
#pragma unroll
    for (int pss = 0; pss < 2; ++pss) {
      // A: x[n, hbase + r*dh, wbase + s*dw, gCg + c .. +8]
      const int h = ahbase[pss] + r * p.dh;
      const int w_ = awbase[pss] + s * p.dw;
      const bool ok = arow_ok[pss] && span_ok && h >= 0 && h < p.H &&
                      w_ >= 0 && w_ < p.W;
      regA[pss] = ok ? *reinterpret_cast<const uint4*>(
                           p.x + (((int64_t)an[pss] * p.H + h) * p.W + w_) *
                                     p.Ct +
                           g * p.Cg + c)
                     : uint4{0, 0, 0, 0};
      // B: w[k, r, span .. +8]
      const bool okb = brow_ok[pss] && span_ok;
      regB[pss] = okb ? *reinterpret_cast<const uint4*>(
                            p.w + ((int64_t)bk[pss] * p.R + r) * SCg + span)
                      : uint4{0, 0, 0, 0};
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int pss = 0; pss < 2; ++pss) {
      *reinterpret_cast<uint4*>(&ldsA[buf][srow + pss * 64][scol8]) = regA[pss];
      *reinterpret_cast<uint4*>(&ldsB[buf][srow + pss * 64][scol8]) = regB[pss];
    }
  };

  // ---- main loop -----------------------------------------------------------
  f32x4 acc[4][4] = {};
  stage_load(0);
  stage_write(0);
  __syncthreads();
  if (p.ksteps > 1) stage_load(1);

  int cur = 0;
  for (int ks = 0; ks < p.ksteps; ++ks) {
    // fragments: A rows wm*64 + mi*16 + il, k = kg*8; B rows wn*64 + ni*16+il
    bf16x8 afrag[4], bfrag[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      afrag[mi] = *reinterpret_cast<const bf16x8*>(
          &ldsA[cur][wm * 64 + mi * 16 + il][kg * 8]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      bfrag[ni] = *reinterpret_cast<const bf16x8*>(
          &ldsB[cur][wn * 64 + ni * 16 + il][kg * 8]);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    __syncthreads();
    if (ks + 1 < p.ksteps) {
      stage_write(cur ^ 1);
      if (ks + 2 < p.ksteps) stage_load(ks + 2);
      __syncthreads();
    }
    cur ^= 1;
  }

  // ---- epilogue: LDS-restage then 16-wide bf16 stores ----------------------
  // Scalar 2-byte stores (64/lane) are store-issue-bound (T21 diagnosis);
  // instead each wave round-trips its 64x64 tile through a private fp32 LDS
  // slab 16 rows at a time, then stores 16 consecutive channels per lane.
  __syncthreads();  // everyone done reading the final A/B tiles
  float* slab = reinterpret_cast<float*>(&ldsA[0][0][0]) + wid * (16 * 68);
  const int HoWo = p.Ho * p.Wo;
  const int er = lane >> 2;          // 0..15 row within the 16-row stripe
  const int ec = (lane & 3) << 4;    // 0,16,32,48 col
  float ps = 0.f, pq = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    // scatter this mi-stripe's fragments to the slab (conflict-free b32)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        slab[(kg * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
    __builtin_amdgcn_wave_barrier();
    const int m = tile_m * BM + wm * 64 + mi * 16 + er;
    if (m < p.M) {
      const int n = m / HoWo;
      const int rem = m - n * HoWo;
      const int64_t obase =
          (((int64_t)n * p.HoA + (rem / p.Wo) * p.osh + p.oh0) * p.WoA +
           (rem % p.Wo) * p.osw + p.ow0) * p.Kt + g * p.Kg;
      const int k0 = tile_n * BN + wn * 64 + ec;
      union {
        __hip_bfloat16 b[16];
        uint4 q[2];
      } u;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
      if (ACC) {
        if (k0 + 16 <= p.Kg) {
          union {
            __hip_bfloat16 b[16];
            uint4 q[2];
          } old;
          old.q[0] = *reinterpret_cast<const uint4*>(&p.y[obase + k0]);
          old.q[1] = *reinterpret_cast<const uint4*>(&p.y[obase + k0 + 8]);
#pragma unroll
          for (int j = 0; j < 16; ++j)
            u.b[j] = from_f32<__hip_bfloat16>(to_f32(u.b[j]) +
                                              to_f32(old.b[j]));
          *reinterpret_cast<uint4*>(&p.y[obase + k0]) = u.q[0];
          *reinterpret_cast<uint4*>(&p.y[obase + k0 + 8]) = u.q[1];
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (k0 + j < p.Kg)
              p.y[obase + k0 + j] = from_f32<__hip_bfloat16>(
                  to_f32(u.b[j]) + to_f32(p.y[obase + k0 + j]));
        }
      } else if (k0 + 16 <= p.Kg) {
        *reinterpret_cast<uint4*>(&p.y[obase + k0]) = u.q[0];
        *reinterpret_cast<uint4*>(&p.y[obase + k0 + 8]) = u.q[1];
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (k0 + j < p.Kg) p.y[obase + k0 + j] = u.b[j];
      }
    }
    if (EMIT) {
      const int base = tile_m * BM + wm * 64 + mi * 16;
      bn_partial_col_accum(slab, ps, pq,
                           (int)min((int64_t)16, (int64_t)p.M - base), lane);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (EMIT) {
    // cross-wave (wm) combine via LDS halves the partial rows
    float* xarea = reinterpret_cast<float*>(&ldsB[0][0][0]);
    if (wm == 1) {
      xarea[(wn * 2 + 0) * 64 + lane] = ps;
      xarea[(wn * 2 + 1) * 64 + lane] = pq;
    }
    __syncthreads();
    if (wm == 0) {
      ps += xarea[(wn * 2 + 0) * 64 + lane];
      pq += xarea[(wn * 2 + 1) * 64 + lane];
      const int kbase = tile_n * BN + wn * 64;
      bn_partial_store(p.part,
                       (int64_t)tile_m * 2 * p.Kt + g * p.Kg + kbase,
                       p.Kt, lane, min(64, p.Kg - kbase), ps, pq);
    }
  }
}


// ---------------------------------------------------------------------------
// Small 1x1 GEMM: y[M, Kt] = x[M, C] @ w[Kt, C]^T for the shallow shapes
// (C <= 256, Kt <= 512) where the 128x128x32 tile kernel spends most of its
// time on pipeline fill/drain (2-8 k-steps) and half-empty B tiles (K = 64).
// Both MFMA operands load DIRECT from global: w (<= 256 KB) is L2-resident
// across the whole launch, and each x row is L1-reused by the wave's four
// B fragments. Each wave owns 64 m-rows and loops over 64-wide k chunks.
// ---------------------------------------------------------------------------
struct SmallGemmParams {
  const __hip_bfloat16* x;
  const __hip_bfloat16* w;
  __hip_bfloat16* y;
  int C, Kt;
  int64_t M;
  float* part;  // EMIT: [ceil(M/256)*4, 2*Kt] BN partials
};

template <bool EMIT>
__global__ __launch_bounds__(256) void conv_gemm_small_kernel(
    SmallGemmParams p) {
  __shared__ float slab4[4][16 * 68];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int64_t mbase = (int64_t)blockIdx.x * 256 + wid * 64;
  const __hip_bfloat16* xrow[4];
  bool m_ok[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = mbase + mi * 16 + il;
    m_ok[mi] = m < p.M;
    xrow[mi] = p.x + (m_ok[mi] ? m : 0) * p.C + kq * 8;
  }
  float* slab = slab4[wid];
  const int er = lane >> 2, ec = (lane & 3) << 4;
  for (int k0 = 0; k0 < p.Kt; k0 += 64) {
    const __hip_bfloat16* wrow[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      wrow[ni] = p.w + (int64_t)(k0 + ni * 16 + il) * p.C + kq * 8;
    f32x4 acc[4][4] = {};
    for (int c0 = 0; c0 < p.C; c0 += 32) {
      bf16x8 afrag[4], bfrag[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        afrag[mi] = m_ok[mi] ? *reinterpret_cast<const bf16x8*>(xrow[mi] + c0)
                             : bf16x8{};
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bfrag[ni] = *reinterpret_cast<const bf16x8*>(wrow[ni] + c0);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    }
    // per-wave LDS-restage epilogue (16-wide bf16 stores; T21)
    float ps = 0.f, pq = 0.f;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          slab[(kq * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
      __builtin_amdgcn_wave_barrier();
      const int64_t m = mbase + mi * 16 + er;
      if (m < p.M) {
        union {
          __hip_bfloat16 b[16];
          uint4 q[2];
        } u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
        __hip_bfloat16* yp = p.y + m * p.Kt + k0 + ec;
        *reinterpret_cast<uint4*>(yp) = u.q[0];
        *reinterpret_cast<uint4*>(yp + 8) = u.q[1];
      }
      if (EMIT)
        bn_partial_col_accum(
            slab, ps, pq,
            (int)min((int64_t)16, p.M - (mbase + mi * 16)), lane);
      __builtin_amdgcn_wave_barrier();
    }
    if (EMIT) {
      __shared__ float xarea[3][2][64];
      if (wid > 0) {
        xarea[wid - 1][0][lane] = ps;
        xarea[wid - 1][1][lane] = pq;
      }
      __syncthreads();
      if (wid == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ps += xarea[j][0][lane];
          pq += xarea[j][1][lane];
        }
        bn_partial_store(p.part, (int64_t)blockIdx.x * 2 * p.Kt + k0,
                         p.Kt, lane, min(64, p.Kt - k0), ps, pq);
      }
      __syncthreads();  // xarea reused next k0 chunk
    }
  }
}


// C <= 64 variant: the whole per-wave A stripe (64 rows x C) is register-
// cached across k chunks, so x is read exactly once regardless of Kt (the
// generic kernel re-reads A per 64-wide k chunk, which loses for Kt > 64).
// min 3 blocks/CU (3 waves/SIMD -> <=170 VGPRs): the EMIT variant's natural
// allocation is 180, which silently dropped smallc to 2 waves/SIMD
template <int CS, bool EMIT>  // CS = C / 32
__global__ __launch_bounds__(256, 3) void conv_gemm_smallc_kernel(
    SmallGemmParams p) {
  __shared__ float slab4[4][16 * 68];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int64_t mbase = (int64_t)blockIdx.x * 256 + wid * 64;
  float* slab = slab4[wid];
  const int er = lane >> 2, ec = (lane & 3) << 4;
  bf16x8 afr[CS][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = mbase + mi * 16 + il;
    const __hip_bfloat16* xr = p.x + (m < p.M ? m : 0) * p.C + kq * 8;
#pragma unroll
    for (int cs = 0; cs < CS; ++cs)
      afr[cs][mi] = m < p.M ? *reinterpret_cast<const bf16x8*>(xr + cs * 32)
                            : bf16x8{};
  }
  for (int k0 = 0; k0 < p.Kt; k0 += 64) {
    const __hip_bfloat16* wrow[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      wrow[ni] = p.w + (int64_t)(k0 + ni * 16 + il) * p.C + kq * 8;
    f32x4 acc[4][4] = {};
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
      bf16x8 bfrag[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bfrag[ni] = *reinterpret_cast<const bf16x8*>(wrow[ni] + cs * 32);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr[cs][mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    }
    float ps = 0.f, pq = 0.f;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          slab[(kq * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
      __builtin_amdgcn_wave_barrier();
      const int64_t m = mbase + mi * 16 + er;
      if (m < p.M) {
        union {
          __hip_bfloat16 b[16];
          uint4 q[2];
        } u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
        __hip_bfloat16* yp = p.y + m * p.Kt + k0 + ec;
        *reinterpret_cast<uint4*>(yp) = u.q[0];
        *reinterpret_cast<uint4*>(yp + 8) = u.q[1];
      }
      if (EMIT)
        bn_partial_col_accum(
            slab, ps, pq,
            (int)min((int64_t)16, p.M - (mbase + mi * 16)), lane);
      __builtin_amdgcn_wave_barrier();
    }
    if (EMIT) {
      __shared__ float xarea[3][2][64];
      if (wid > 0) {
        xarea[wid - 1][0][lane] = ps;
        xarea[wid - 1][1][lane] = pq;
      }
      __syncthreads();
      if (wid == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ps += xarea[j][0][lane];
          pq += xarea[j][1][lane];
        }
        bn_partial_store(p.part, (int64_t)blockIdx.x * 2 * p.Kt + k0,
                         p.Kt, lane, min(64, p.Kt - k0), ps, pq);
      }
      __syncthreads();  // xarea reused next k0 chunk
    }
  }
}


// ---------------------------------------------------------------------------
// K=64 small-C patch conv (stem 7x7 s2 C=8, 3x3 64->64): one 64-col B tile
// means half of the 128-wide tile kernel idles. Here both operands load
// direct from global with full per-lane patch predication: each lane's 16 B
// A fragment is one (r, s, c-pack) patch element (magic-div span
// decomposition), B is the span-padded [64, RSCp] weight (L2-resident).
// Block = 4 waves x 64 m-rows, each wave owns all 64 output channels.
// ---------------------------------------------------------------------------
struct SmallConvParams {
  const __hip_bfloat16* x;  // [N,H,W,C]
  const __hip_bfloat16* w;  // [64, RSCp] span-padded flat
  const __hip_bfloat16* zbuf;  // 16 zero bytes (clamp target for OOB loads)
  __hip_bfloat16* y;        // [N,Ho,Wo,64]
  int C, H, W;
  int R, S, SC;
  int sh, sw, ph, pw;
  int Ho, Wo;
  int RSC, RSCp;
  int64_t M;
  unsigned long long magicHoWo, magicWo, magicSC, magicC;
  float* part;  // EMIT: [ceil(M/256)*4, 2*64] BN partials
};

DEV_INLINE int magic_div2(int m, unsigned long long magic) {
  return (int)(((unsigned long long)(unsigned)m * magic) >> 47);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void conv_smallk_kernel(SmallConvParams p) {
  __shared__ float slab4[4][16 * 68];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int64_t mbase = (int64_t)blockIdx.x * 256 + wid * 64;
  int pn[4], prow[4], pcol[4];
  bool mok[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = mbase + mi * 16 + il;
    mok[mi] = m < p.M;
    const int mm = (int)(mok[mi] ? m : 0);
    const int n = magic_div2(mm, p.magicHoWo);
    const int rem = mm - n * (p.Ho * p.Wo);
    const int ho = magic_div2(rem, p.magicWo);
    const int wo = rem - ho * p.Wo;
    pn[mi] = n;
    prow[mi] = ho * p.sh - p.ph;
    pcol[mi] = wo * p.sw - p.pw;
  }
  const __hip_bfloat16* wr[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    wr[ni] = p.w + (int64_t)(ni * 16 + il) * p.RSCp + kq * 8;
  f32x4 acc[4][4] = {};
  if (p.C % 32 == 0) {
    // tap-ordered loop (C a multiple of 32): the per-tap bounds check and
    // base address are computed once per (r, s) instead of per k-step —
    // the k-step-ordered form below was VALU-bound on its per-step
    // magic-div + predication chain (~80 VALU per 16 MFMAs).
    const int csteps = p.C / 32;
    for (int r = 0; r < p.R; ++r) {
#pragma unroll 1
      for (int sidx = 0; sidx < p.S; ++sidx) {
        const __hip_bfloat16* ab[4];
        bool ok[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const int h = prow[mi] + r;
          const int w_ = pcol[mi] + sidx;
          ok[mi] = mok[mi] && h >= 0 && h < p.H && w_ >= 0 && w_ < p.W;
          ab[mi] = p.x +
                   (((int64_t)pn[mi] * p.H + h) * p.W + w_) * p.C + kq * 8;
        }
        const int e0 = (r * p.S + sidx) * p.C;
        for (int cc = 0; cc < csteps; ++cc) {
          bf16x8 afrag[4], bfrag[4];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            afrag[mi] = ok[mi] ? *reinterpret_cast<const bf16x8*>(ab[mi] +
                                                                  cc * 32)
                               : bf16x8{};
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            bfrag[ni] =
                *reinterpret_cast<const bf16x8*>(wr[ni] + e0 + cc * 32);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
        }
      }
    }
  } else {
    const int ksteps = p.RSCp / 32;
    for (int t = 0; t < ksteps; ++t) {
      const int e = t * 32 + kq * 8;
      const int r = magic_div2(e, p.magicSC);
      const int rem2 = e - r * p.SC;
      const int sidx = magic_div2(rem2, p.magicC);
      const int c = rem2 - sidx * p.C;
      bf16x8 afrag[4], bfrag[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int h = prow[mi] + r;
        const int w_ = pcol[mi] + sidx;
        const bool ok = mok[mi] && e < p.RSC && h >= 0 && h < p.H &&
                        w_ >= 0 && w_ < p.W;
        afrag[mi] =
            ok ? *reinterpret_cast<const bf16x8*>(
                     p.x + (((int64_t)pn[mi] * p.H + h) * p.W + w_) * p.C + c)
               : bf16x8{};
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bfrag[ni] = *reinterpret_cast<const bf16x8*>(wr[ni] + t * 32);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    }
  }
  float* slab = slab4[wid];
  const int er = lane >> 2, ec = (lane & 3) << 4;
  float ps = 0.f, pq = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        slab[(kq * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
    __builtin_amdgcn_wave_barrier();
    const int64_t m = mbase + mi * 16 + er;
    if (m < p.M) {
      union {
        __hip_bfloat16 b[16];
        uint4 q[2];
      } u;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
      __hip_bfloat16* yp = p.y + m * 64 + ec;
      *reinterpret_cast<uint4*>(yp) = u.q[0];
      *reinterpret_cast<uint4*>(yp + 8) = u.q[1];
    }
    if (EMIT)
      bn_partial_col_accum(slab, ps, pq,
                           (int)min((int64_t)16, p.M - (mbase + mi * 16)),
                           lane);
    __builtin_amdgcn_wave_barrier();
  }
  if (EMIT) {
    __shared__ float xarea[3][2][64];
    if (wid > 0) {
      xarea[wid - 1][0][lane] = ps;
      xarea[wid - 1][1][lane] = pq;
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        ps += xarea[j][0][lane];
        pq += xarea[j][1][lane];
      }
      bn_partial_store(p.part, (int64_t)blockIdx.x * 128, 64, lane, 64, ps,
                       pq);
    }
  }
}


// Pipelined variant (C % 32 == 0): PMC showed the plain kernel waits on
// memory ~85% of its cycles (SQ busy 12%) — each k-step's 8 loads are
// consumed by the very next MFMAs. This one (a) selects the ADDRESS
// (OOB -> a 16-byte zero buffer) instead of the loaded value, so no
// post-load cndmask forces an early waitcnt, and (b) prefetches step i+1's
// fragments while step i's MFMAs run.
template <int CSTEPS, bool EMIT>  // CSTEPS = C / 32
__global__ __launch_bounds__(256) void conv_smallk_pipe_kernel(
    SmallConvParams p) {
  __shared__ float slab4[4][16 * 68];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int64_t mbase = (int64_t)blockIdx.x * 256 + wid * 64;
  int pn[4], prow[4], pcol[4];
  bool mok[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = mbase + mi * 16 + il;
    mok[mi] = m < p.M;
    const int mm = (int)(mok[mi] ? m : 0);
    const int n = magic_div2(mm, p.magicHoWo);
    const int rem = mm - n * (p.Ho * p.Wo);
    const int ho = magic_div2(rem, p.magicWo);
    const int wo = rem - ho * p.Wo;
    pn[mi] = n;
    prow[mi] = ho * p.sh - p.ph;
    pcol[mi] = wo * p.sw - p.pw;
  }
  const __hip_bfloat16* wr[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    wr[ni] = p.w + (int64_t)(ni * 16 + il) * p.RSCp + kq * 8;
  const int S = p.S;
  const int steps = p.R * S * CSTEPS;
  int r = 0, si = 0, cc = 0;
  bf16x8 Af[2][4], Bf[2][4];
  auto issue = [&](int buf) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int h = prow[mi] + r;
      const int w_ = pcol[mi] + si;
      const bool ok = mok[mi] && h >= 0 && h < p.H && w_ >= 0 && w_ < p.W;
      const __hip_bfloat16* ap =
          ok ? p.x + (((int64_t)pn[mi] * p.H + h) * p.W + w_) * p.C +
                   cc * 32 + kq * 8
             : p.zbuf;
      Af[buf][mi] = *reinterpret_cast<const bf16x8*>(ap);
    }
    const int e0 = (r * S + si) * p.C + cc * 32;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      Bf[buf][ni] = *reinterpret_cast<const bf16x8*>(wr[ni] + e0);
    ++cc;
    if (cc == CSTEPS) {
      cc = 0;
      ++si;
      if (si == S) {
        si = 0;
        ++r;
      }
    }
  };
  f32x4 acc[4][4] = {};
  // 2x-unrolled so the double-buffer index is a compile-time constant
  // (a runtime `i & 1` index on the fragment arrays spills them to
  // scratch — rule 20 — measured 60x slower)
  issue(0);
  for (int i = 0; i < steps; i += 2) {
    if (i + 1 < steps) issue(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            Af[0][mi], Bf[0][ni], acc[mi][ni], 0, 0, 0);
    if (i + 1 < steps) {
      if (i + 2 < steps) issue(0);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              Af[1][mi], Bf[1][ni], acc[mi][ni], 0, 0, 0);
    }
  }
  float* slab = slab4[wid];
  const int er = lane >> 2, ec = (lane & 3) << 4;
  float ps = 0.f, pq = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        slab[(kq * 4 + rr) * 68 + ni * 16 + il] = acc[mi][ni][rr];
    __builtin_amdgcn_wave_barrier();
    const int64_t m = mbase + mi * 16 + er;
    if (m < p.M) {
      union {
        __hip_bfloat16 b[16];
        uint4 q[2];
      } u;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        u.b[j] = from_f32<__hip_bfloat16>(slab[er * 68 + ec + j]);
      __hip_bfloat16* yp = p.y + m * 64 + ec;
      *reinterpret_cast<uint4*>(yp) = u.q[0];
      *reinterpret_cast<uint4*>(yp + 8) = u.q[1];
    }
    if (EMIT)
      bn_partial_col_accum(slab, ps, pq,
                           (int)min((int64_t)16, p.M - (mbase + mi * 16)),
                           lane);
    __builtin_amdgcn_wave_barrier();
  }
  if (EMIT) {
    __shared__ float xarea[3][2][64];
    if (wid > 0) {
      xarea[wid - 1][0][lane] = ps;
      xarea[wid - 1][1][lane] = pq;
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        ps += xarea[j][0][lane];
        pq += xarea[j][1][lane];
      }
      bn_partial_store(p.part, (int64_t)blockIdx.x * 128, 64, lane, 64, ps,
                       pq);
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
// one launch per kernel family: each picks the instantiation from its flags
static void launch_v1(const ConvParams& p, dim3 grid, bool emit, bool acc) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(), p);
  };
  if (emit) go(conv_igemm_fwd_kernel<true>);
  else if (acc) go(conv_igemm_fwd_kernel<false, true>);
  else go(conv_igemm_fwd_kernel<false>);
}

// small 1x1 GEMM family: the register-cached C = 64 / 32 kernels, else generic
template <bool EMIT>
static void launch_small_gemm(const SmallGemmParams& p, dim3 grid) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(), p);
  };
  if (p.C == 64) go(conv_gemm_smallc_kernel<2, EMIT>);
  else if (p.C == 32) go(conv_gemm_smallc_kernel<1, EMIT>);
  else go(conv_gemm_small_kernel<EMIT>);
}

// K = 64 patch family: the pipelined C = 64 / 32 kernels, else generic
template <bool EMIT>
static void launch_smallk(const SmallConvParams& p, dim3 grid) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(), p);
  };
  if (p.C == 64) go(conv_smallk_pipe_kernel<2, EMIT>);
  else if (p.C == 32) go(conv_smallk_pipe_kernel<1, EMIT>);
  else go(conv_smallk_kernel<EMIT>);
}

at::Tensor conv2d_fwd_into(at::Tensor x, at::Tensor w, at::Tensor y, int64_t Ho,
                           int64_t Wo, int64_t sh, int64_t sw, int64_t ph,
                           int64_t pw, int64_t dh, int64_t dw, int64_t groups,
                           int64_t osh = 1, int64_t osw = 1, int64_t oh0 = 0,
                           int64_t ow0 = 0, at::Tensor* part_out = nullptr,
                           bool acc = false) {
  CHECK_GPU(x);
  if (x.scalar_type() == at::kFloat)
    return conv2d_fwd_into_fp32(x, w, y, Ho, Wo, sh, sw, ph, pw, dh, dw,
                                groups, osh, osw, oh0, ow0, part_out);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "conv2d_fwd: bf16/fp32 only");
  {
    // deep pad-free windows (parity-decomposed / strided dgrads) ride the
    // v2 glds ring with the scatter epilogue instead of the v1 tile kernel
    const ConvGates& gates = conv_gates();
    const int Cgi = w.size(1), Ri = w.size(2), Si = w.size(3);
    const int Kgi = (int)(w.size(0) / groups);
    if (gates.v2into && part_out == nullptr && ph == 0 && pw == 0 &&
        sh == 1 && sw == 1 && dh == 1 && dw == 1 &&
        (Si * Cgi) % 64 == 0 && Kgi >= 96 &&
        (int64_t)Ri * Si * Cgi >= gates.v2into_minrsc && Cgi % 8 == 0 &&
        Ho + Ri - 1 <= x.size(2) && Wo + Si - 1 <= x.size(3))
      return conv2d_fwd_v2_into(x, w, y, Ho, Wo, groups, osh, osw, oh0, ow0,
                                acc);
  }
  check_nhwc(x, "x");
  check_nhwc(w, "w");
  const int N = x.size(0), Ct = x.size(1), H = x.size(2), W = x.size(3);
  const int Kt = w.size(0), Cg = w.size(1), R = w.size(2), S = w.size(3);
  TORCH_CHECK(Ct == Cg * groups, "channel/group mismatch");
  TORCH_CHECK(Cg % 8 == 0, "conv2d_fwd: per-group C must be a multiple of 8");
  const int Kg = Kt / groups;
  ConvParams p;
  p.x = (const __hip_bfloat16*)x.data_ptr();
  p.w = (const __hip_bfloat16*)w.data_ptr();
  p.y = (__hip_bfloat16*)y.data_ptr();
  p.N = N; p.H = H; p.W = W; p.Ct = Ct; p.Kt = Kt;
  p.R = R; p.S = S; p.Cg = Cg; p.Kg = Kg;
  p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.Ho = Ho; p.Wo = Wo;
  p.HoA = y.size(2); p.WoA = y.size(3);
  p.osh = osh; p.osw = osw;
  p.oh0 = oh0; p.ow0 = ow0;
  p.M = N * Ho * Wo;
  p.nspan = (S * Cg + BK - 1) / BK;
  p.ksteps = R * p.nspan;
  p.tiles_m = (p.M + BM - 1) / BM;
  p.part = nullptr;
  dim3 grid(p.tiles_m, (Kg + BN - 1) / BN, groups);
  if (part_out != nullptr) {
    *part_out = at::empty({(int64_t)p.tiles_m, (int64_t)2 * Kt},
                          x.options().dtype(at::kFloat));
    p.part = part_out->data_ptr<float>();
  }
  launch_v1(p, grid, part_out != nullptr, acc);
  return y;
}

// halo_force: -1 = the dispatcher's own choice, 0 / 1 = force the 3x3 64->64
// route off / on (conv2d_fwd_halo_dbg)
static at::Tensor conv2d_fwd_impl(at::Tensor x, at::Tensor w, int64_t sh,
                                  int64_t sw, int64_t ph, int64_t pw,
                                  int64_t dh, int64_t dw, int64_t groups,
                                  at::Tensor* part_out,
                                  int halo_force = -1) {
  const int N = x.size(0), H = x.size(2), W = x.size(3);
  const int Kt = w.size(0), R = w.size(2), S = w.size(3);
  // v2 (3-slot glds ring) wins when the reduction is deep enough to fill
  // its pipeline; v1 handles shallow-K, small-K and grouped shapes.
  const ConvGates& gates = conv_gates();
  const int C_ = x.size(1);
  // per-group geometry decides the ring gate (v2_ring_ok)
  if (v2_ring_ok(Kt / (int)groups, C_ / (int)groups, R, S,
                 x.scalar_type() == at::kBFloat16))
    return conv2d_fwd_v2p(x, w, sh, sw, ph, pw, dh, dw, groups, part_out);
  if (gates.small && groups == 1 && R == 1 && S == 1 && sh == 1 && sw == 1 &&
      C_ % 32 == 0 && Kt % 64 == 0 && x.scalar_type() == at::kBFloat16 &&
      ((C_ <= 64 && Kt <= 512) || (C_ <= 256 && Kt <= 64))) {
    const int64_t M = (int64_t)N * H * W;
    auto y = at::empty({N, Kt, H, W},
                       x.options().memory_format(at::MemoryFormat::ChannelsLast));
    SmallGemmParams sp;
    sp.x = (const __hip_bfloat16*)x.data_ptr();
    sp.w = (const __hip_bfloat16*)w.data_ptr();
    sp.y = (__hip_bfloat16*)y.data_ptr();
    sp.C = C_; sp.Kt = Kt; sp.M = M;
    sp.part = nullptr;
    const dim3 sg((int)((M + 255) / 256));
    if (part_out != nullptr) {
      *part_out = at::empty({(int64_t)sg.x, (int64_t)2 * Kt},
                            x.options().dtype(at::kFloat));
      sp.part = part_out->data_ptr<float>();
    }
    sp.part ? launch_small_gemm<true>(sp, sg)
            : launch_small_gemm<false>(sp, sg);
    return y;
  }
  const int Ho = (H + 2 * ph - dh * (R - 1) - 1) / sh + 1;
  const int Wo = (W + 2 * pw - dw * (S - 1) - 1) / sw + 1;
  if (gates.small && groups == 1 && Kt == 64 && C_ <= 64 && C_ % 8 == 0 &&
      dh == 1 && dw == 1 && R * S > 1 && R * S * C_ <= 1024 &&
      x.scalar_type() == at::kBFloat16) {
    const int RSC = R * S * C_;
    const int RSCp = (RSC + 31) / 32 * 32;
    at::Tensor wsp = w;
    if (RSCp != RSC) {
      wsp = at::zeros({(int64_t)Kt, RSCp}, w.options());
      wsp.narrow(1, 0, RSC).copy_(
          w.permute({0, 2, 3, 1}).reshape({(int64_t)Kt, RSC}));
    }
    auto y = at::empty({N, Kt, Ho, Wo},
                       x.options().memory_format(at::MemoryFormat::ChannelsLast));
    SmallConvParams sp;
    sp.x = (const __hip_bfloat16*)x.data_ptr();
    sp.w = (const __hip_bfloat16*)wsp.data_ptr();
    sp.y = (__hip_bfloat16*)y.data_ptr();
    sp.C = C_; sp.H = H; sp.W = W;
    sp.R = R; sp.S = S; sp.SC = S * C_;
    sp.sh = sh; sp.sw = sw; sp.ph = ph; sp.pw = pw;
    sp.Ho = Ho; sp.Wo = Wo;
    sp.RSC = RSC; sp.RSCp = RSCp;
    sp.M = (int64_t)N * Ho * Wo;
    sp.magicHoWo = ((1ULL << 47) / ((unsigned long long)Ho * Wo)) + 1;
    sp.magicWo = ((1ULL << 47) / (unsigned long long)Wo) + 1;
    sp.magicSC = ((1ULL << 47) / (unsigned long long)(S * C_)) + 1;
    sp.magicC = ((1ULL << 47) / (unsigned long long)C_) + 1;
    static at::Tensor zbuf;  // 16 zero bytes; allocated outside any capture
    if (!zbuf.defined() || zbuf.device() != x.device())
      zbuf = at::zeros({8}, x.options());
    sp.zbuf = (const __hip_bfloat16*)zbuf.data_ptr();
    sp.part = nullptr;
    const dim3 skg((int)((sp.M + 255) / 256));
    // 3x3 / stride 1 / pad 1 / 64->64: input tile + halo staged in LDS once
    // instead of nine global reads per pixel (conv_halo.hip); bit-identical
    const bool halo_fits =
        C_ == 64 && R == 3 && S == 3 && sh == 1 && sw == 1 && ph == 1 &&
        pw == 1 && x.is_contiguous(at::MemoryFormat::ChannelsLast) &&
        w.is_contiguous(at::MemoryFormat::ChannelsLast) &&
        conv3x3_halo_admits(N, H, W);
    TORCH_CHECK(halo_force != 1 || halo_fits,
                "conv2d_fwd: shape outside the halo kernel's gate");
    if (halo_force == 1 || (halo_force < 0 && gates.halo && halo_fits)) {
      float* hp = nullptr;
      if (part_out != nullptr) {
        *part_out = at::empty({(int64_t)skg.x, 128},
                              x.options().dtype(at::kFloat));
        hp = part_out->data_ptr<float>();
      }
      conv3x3_halo_launch(x, w, y, zbuf, hp);
      return y;
    }
    if (part_out != nullptr) {
      *part_out = at::empty({(int64_t)skg.x, 128},
                            x.options().dtype(at::kFloat));
      sp.part = part_out->data_ptr<float>();
    }
    sp.part ? launch_smallk<true>(sp, skg) : launch_smallk<false>(sp, skg);
    return y;
  }
  auto y = at::empty({N, Kt, Ho, Wo},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  return conv2d_fwd_into(x, w, y, Ho, Wo, sh, sw, ph, pw, dh, dw, groups, 1,
                         1, 0, 0, part_out);
}


// Probe/testing entry: force the v1 predicated kernel (bypasses the
// small-family routing in conv2d_fwd_impl).
at::Tensor conv2d_fwd_v1(at::Tensor x, at::Tensor w, at::Tensor y,
                         int64_t Ho, int64_t Wo, int64_t sh, int64_t sw,
                         int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                         int64_t groups) {
  return conv2d_fwd_into(x, w, y, Ho, Wo, sh, sw, ph, pw, dh, dw, groups);
}

at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                      int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                      int64_t groups) {
  return conv2d_fwd_impl(x, w, sh, sw, ph, pw, dh, dw, groups, nullptr);
}

// Debug/benchmark entry: the dispatcher's launch for a small-K conv with the
// halo route forced on or off, so both kernels run in one process (the env
// knobs are read once). 3x3 / stride 1 / pad 1. Returns {y} or {y, part}.
std::vector<at::Tensor> conv2d_fwd_halo_dbg(at::Tensor x, at::Tensor w,
                                            bool emit, bool halo) {
  at::Tensor part;
  auto y = conv2d_fwd_impl(x, w, 1, 1, 1, 1, 1, 1, 1, emit ? &part : nullptr,
                           halo ? 1 : 0);
  if (!emit) return {y};
  TORCH_CHECK(part.defined(), "conv2d_fwd_halo_dbg: route without partials");
  return {y, part};
}

// conv forward + BN sum/sumsq partials emitted from the epilogue (F1):
// returns {y, part} with part a [nblocks, 2*Kt] fp32 tensor consumable by
// bn_stats(part_opt=...). Stats are over the bf16-rounded stored y, exactly
// matching what bn_sums(y) would compute.
std::vector<at::Tensor> conv2d_fwd_bn(at::Tensor x, at::Tensor w, int64_t sh,
                                      int64_t sw, int64_t ph, int64_t pw,
                                      int64_t dh, int64_t dw, int64_t groups) {
  at::Tensor part;
  auto y = conv2d_fwd_impl(x, w, sh, sw, ph, pw, dh, dw, groups, &part);
  TORCH_CHECK(part.defined(), "conv2d_fwd_bn: dispatch path without partials");
  return {y, part};
}

// NT GEMM through the conv kernel: y[M, N] = a[M, K] @ b[N, K]^T
at::Tensor gemm_nt(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "gemm_nt expects 2-D");
  const int M = a.size(0), K = a.size(1), Nc = b.size(0);
  // NHWC 4-D with H=W=1: logical [M,K,1,1] channels_last == [M][K] rows
  auto a_cl = a.reshape({M, K, 1, 1}).contiguous(at::MemoryFormat::ChannelsLast);
  auto b_cl = b.reshape({Nc, K, 1, 1}).contiguous(at::MemoryFormat::ChannelsLast);
  // route through the dispatcher so deep-K GEMMs hit the v2 ring kernel
  auto y = conv2d_fwd(a_cl, b_cl, 1, 1, 0, 0, 1, 1, 1);
  return y.reshape({M, Nc});
}

// ---------------------------------------------------------------------------
// dgrad transforms
// ---------------------------------------------------------------------------
namespace {

// wt[g*Cg + c][r][s][Kg] = w[g*Kg + k][R-1-r][S-1-s][c]  (per group)
template <typename T>
__global__ void weight_flip_t_kernel(const T* __restrict__ w, T* __restrict__ wt,
                                     int Kg, int Cg, int R, int S, int G) {
  const int64_t total = (int64_t)G * Cg * R * S * Kg;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = i;
    const int k = t % Kg;
    t /= Kg;
    const int s = t % S;
    t /= S;
    const int r = t % R;
    t /= R;
    const int c = t % Cg;
    const int g = t / Cg;
    wt[i] = w[((((int64_t)(g * Kg + k) * R) + (R - 1 - r)) * S + (S - 1 - s)) *
                  Cg +
              c];
  }
}

// zero-dilate NHWC: out[n, ho*sh, wo*sw, c] = x[n, ho, wo, c]
template <typename T>
__global__ void dilate_nhwc_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   int N, int Ho, int Wo, int C, int sh,
                                   int sw, int Hd, int Wd) {
  const int64_t total = (int64_t)N * Ho * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = i % C;
    int64_t t = i / C;
    const int wo = t % Wo;
    t /= Wo;
    const int ho = t % Ho;
    const int n = t / Ho;
    y[(((int64_t)n * Hd + ho * sh) * Wd + wo * sw) * C + c] = x[i];
  }
}

}  // namespace

namespace {
// fused dgrad weight transform: flipT + span-pad in ONE pass. Output flat
// [Ct, R, SPAN64] rows for the v2 ring (sp < S*Kg: w[gKg+k][R-1-r][S-1-s][c],
// else 0) — replaces the separate flip write + pad read/write passes.
template <typename T>
__global__ void weight_flip_t_span_kernel(const T* __restrict__ w,
                                          T* __restrict__ o, int Kg, int Cg,
                                          int R, int S, int G, int SPAN64) {
  const int64_t total = (int64_t)G * Cg * R * SPAN64;
  const int SKg = S * Kg;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int sp = i % SPAN64;
    int64_t t = i / SPAN64;
    const int r = t % R;
    t /= R;
    const int c = t % Cg;
    const int g = t / Cg;
    T v = from_f32<T>(0.f);
    if (sp < SKg) {
      const int sidx = sp / Kg;
      const int k = sp - sidx * Kg;
      v = w[((((int64_t)(g * Kg + k) * R) + (R - 1 - r)) * S +
             (S - 1 - sidx)) * Cg + c];
    }
    o[i] = v;
  }
}
}  // namespace

at::Tensor weight_flip_t_span(at::Tensor w, int64_t groups, int64_t SPAN64) {
  CHECK_GPU(w);
  check_nhwc(w, "w");
  const int Kt = w.size(0), Cg = w.size(1), R = w.size(2), S = w.size(3);
  const int Kg = Kt / groups;
  auto o = at::empty({(int64_t)Cg * groups * R * SPAN64}, w.options());
  const int64_t total = o.numel();
  DISPATCH_FLOAT_AND_BF16(w.scalar_type(), "weight_flip_t_span", [&] {
    hipLaunchKernelGGL((weight_flip_t_span_kernel<scalar_t>),
                       dim3(grid_1d(total, 256)), dim3(256), 0, cur_stream(),
                       (const scalar_t*)w.data_ptr(), (scalar_t*)o.data_ptr(),
                       Kg, Cg, R, S, (int)groups, (int)SPAN64);
  });
  return o;
}

// weight transform for dgrad: [Kt,Cg,R,S]cl -> [Ct,Kg,R,S]cl flipped
at::Tensor weight_flip_t(at::Tensor w, int64_t groups) {
  CHECK_GPU(w);
  check_nhwc(w, "w");
  const int Kt = w.size(0), Cg = w.size(1), R = w.size(2), S = w.size(3);
  const int Kg = Kt / groups;
  auto wt = at::empty({Cg * groups, Kg, R, S},
                      w.options().memory_format(at::MemoryFormat::ChannelsLast));
  int64_t total = (int64_t)Kt * Cg * R * S;
  DISPATCH_FLOAT_AND_BF16(w.scalar_type(), "weight_flip_t", [&] {
    hipLaunchKernelGGL((weight_flip_t_kernel<scalar_t>),
                       dim3(grid_1d(total, 256)), dim3(256), 0, cur_stream(),
                       (const scalar_t*)w.data_ptr(), (scalar_t*)wt.data_ptr(),
                       Kg, Cg, R, S, (int)groups);
  });
  return wt;
}

at::Tensor dilate_nhwc(at::Tensor x, int64_t sh, int64_t sw) {
  CHECK_GPU(x);
  check_nhwc(x, "x");
  const int N = x.size(0), C = x.size(1), Ho = x.size(2), Wo = x.size(3);
  const int Hd = (Ho - 1) * sh + 1, Wd = (Wo - 1) * sw + 1;
  auto y = at::empty({N, C, Hd, Wd},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  y.zero_();
  int64_t total = (int64_t)N * Ho * Wo * C;
  DISPATCH_FLOAT_AND_BF16(x.scalar_type(), "dilate_nhwc", [&] {
    hipLaunchKernelGGL((dilate_nhwc_kernel<scalar_t>),
                       dim3(grid_1d(total, 256)), dim3(256), 0, cur_stream(),
                       (const scalar_t*)x.data_ptr(), (scalar_t*)y.data_ptr(),
                       N, Ho, Wo, C, sh, sw, Hd, Wd);
  });
  return y;
}

// pad the channel dim (NHWC innermost) with zeros: stem C=3 -> 8 so the
// MFMA kernel's Cg%8 requirement holds
namespace {
template <typename T>
__global__ void pad_channels_kernel(const T* __restrict__ x, T* __restrict__ y,
                                    int64_t rows, int C, int Cn) {
  constexpr int V = 16 / sizeof(T);
  if (Cn == V) {
    // one 16-byte output pack per thread (stem 3->8): the per-element
    // modulo form ran at 2.8 TB/s
    union {
      T b[V];
      uint4 q;
    } u;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < rows; r += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
      for (int j = 0; j < V; ++j)
        u.b[j] = j < C ? x[r * C + j] : from_f32<T>(0.f);
      *reinterpret_cast<uint4*>(y + r * V) = u.q;
    }
    return;
  }
  const int64_t total = rows * Cn;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = i % Cn;
    const int64_t r = i / Cn;
    y[i] = (c < C) ? x[r * C + c] : from_f32<T>(0.f);
  }
}
}  // namespace

at::Tensor pad_channels(at::Tensor x, int64_t Cn) {
  CHECK_GPU(x);
  check_nhwc(x, "x");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  auto y = at::empty({N, Cn, H, W},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t rows = (int64_t)N * H * W;
  DISPATCH_FLOAT_AND_BF16(x.scalar_type(), "pad_channels", [&] {
    hipLaunchKernelGGL((pad_channels_kernel<scalar_t>),
                       dim3(grid_1d(rows * Cn, 256)), dim3(256), 0,
                       cur_stream(), (const scalar_t*)x.data_ptr(),
                       (scalar_t*)y.data_ptr(), rows, C, (int)Cn);
  });
  return y;
}

// ---------------------------------------------------------------------------
// dgrad: dgrad_route (conv_route.h) decides, conv2d_dgrad_run executes
// ---------------------------------------------------------------------------
// `into` (may be null) is a candidate accumulate buffer; it qualifies when it
// is a bf16 channels_last tensor of exactly gx's shape.
static DgradRoute dgrad_route_of(const at::Tensor& gy, const at::Tensor& w,
                                 int64_t H, int64_t W, int64_t sh, int64_t sw,
                                 int64_t ph, int64_t pw, int64_t dh,
                                 int64_t dw, int64_t groups,
                                 const at::Tensor* into) {
  const bool into_ok =
      into != nullptr && into->scalar_type() == at::kBFloat16 &&
      into->is_contiguous(at::MemoryFormat::ChannelsLast) &&
      into->sizes() ==
          at::IntArrayRef({gy.size(0), w.size(1) * groups, H, W});
  return dgrad_route(gy.size(1), w.size(1), w.size(2), w.size(3), sh, sw, ph,
                     pw, dh, dw, groups,
                     gy.scalar_type() == at::kBFloat16, into_ok);
}

// gx = conv(dilate(gy), flipT(w)), computed the way `rt` says. With rt.acc
// the epilogue adds gx into *into (ACC epilogues exist in the v1 and v2
// kernels only) and *into is returned; otherwise gx is a fresh tensor.
// pre / pre_kind: an already-transformed weight (conv2d_dgrad_prep), used
// when its kind is the one the route needs.
static at::Tensor conv2d_dgrad_run(DgradRoute rt, at::Tensor gy, at::Tensor w,
                                   int64_t H, int64_t W, int64_t sh,
                                   int64_t sw, int64_t ph, int64_t pw,
                                   int64_t dh, int64_t dw, int64_t groups,
                                   const at::Tensor* pre = nullptr,
                                   int64_t pre_kind = -1,
                                   at::Tensor* into = nullptr) {
  CHECK_GPU(gy);
  check_nhwc(gy, "gy");
  const bool acc = rt.acc;
  TORCH_CHECK(!acc || into, "dgrad: acc needs a buffer");
  const int N = gy.size(0);
  const int Cg = w.size(1), R = w.size(2), S = w.size(3);
  const int Ct = Cg * groups;
  // padding of the stride-1 as-forward conv
  const int pph = dh * (R - 1) - ph, ppw = dw * (S - 1) - pw;
  auto canvas = [&]() {
    return at::empty({N, Ct, H, W}, gy.options().memory_format(
                                        at::MemoryFormat::ChannelsLast));
  };
  if (rt.kind == DgradKind::V2Same) {
    // ONE fused flip+span-pad weight pass feeds the ring directly
    const int fCg = gy.size(1) / (int)groups;
    const int SPAN64 = ((int)(S * fCg) + 63) / 64 * 64;
    auto wsp = (pre != nullptr && pre_kind == 1)
                   ? *pre
                   : weight_flip_t_span(w, groups, SPAN64);
    return conv2d_fwd_v2_flat(gy, wsp, Ct, fCg, R, S, 1, 1, pph, ppw, dh, dw,
                              groups, nullptr, acc ? into : nullptr);
  }
  auto wt = (pre != nullptr && pre_kind == 0)
                ? *pre
                : weight_flip_t(w, groups);  // [Ct, Kg, R, S] cl
  switch (rt.kind) {
    case DgradKind::Strided1x1: {
      // strided-output GEMM: gx[ho*sh, wo*sw] = gy[ho, wo] @ w^T, rest zero.
      // With acc the gaps receive no main-branch gradient: `into` already
      // holds their final values.
      at::Tensor gx = acc ? *into : canvas();
      if (!acc) gx.zero_();
      conv2d_fwd_into(gy, wt, gx, gy.size(2), gy.size(3), 1, 1, 0, 0, 1, 1,
                      groups, sh, sw, 0, 0, nullptr, acc);
      return gx;
    }
    case DgradKind::Parity3x3: {
      // parity decomposition: for stride-2 with pad 1, each output-parity
      // class (h%2, w%2) of gx receives only the taps of matching parity —
      // four small {1,2}x{1,2}-tap convs over gy scattered with stride 2
      // instead of a 3x3 conv over 2x-dilated (3/4-zero) gy. Derivation:
      // for h = 2u + h0, ho = u + e with e = (h0 + 1 - r)/2, so the
      // e-ordered tap weights are flipT(w) rows (1 - h0)::2. The four
      // classes tile gx disjointly, so with acc each sub-conv
      // scatter-accumulates its own positions exactly once.
      at::Tensor gx = acc ? *into : canvas();
      for (int h0 = 0; h0 < 2; ++h0) {
        const int64_t hu = (H - h0 + 1) >> 1;
        auto wr = (h0 == 0) ? wt.slice(2, 1, 2) : wt.slice(2, 0, 3, 2);
        for (int w0 = 0; w0 < 2; ++w0) {
          const int64_t wu = (W - w0 + 1) >> 1;
          auto wsub = ((w0 == 0) ? wr.slice(3, 1, 2) : wr.slice(3, 0, 3, 2))
                          .contiguous(at::MemoryFormat::ChannelsLast);
          conv2d_fwd_into(gy, wsub, gx, hu, wu, 1, 1, 0, 0, 1, 1, groups, 2,
                          2, h0, w0, nullptr, acc);
        }
      }
      return gx;
    }
    case DgradKind::Same:
      // same-size conv. Fresh output: the plain fwd dispatcher applies and
      // reaches the small and halo kernels. acc: the v1 predicated kernel.
      if (acc)
        return conv2d_fwd_into(gy, wt, *into, H, W, 1, 1, pph, ppw, dh, dw,
                               groups, 1, 1, 0, 0, nullptr, true);
      return conv2d_fwd_impl(gy, wt, 1, 1, pph, ppw, dh, dw, groups, nullptr);
    default: {
      auto gyd = (sh == 1 && sw == 1) ? gy : dilate_nhwc(gy, sh, sw);
      TORCH_CHECK(pph >= 0 && ppw >= 0, "dgrad pad underflow");
      // Every input row/col receives its own output: run the conv at
      // logical output size exactly (H, W); the kernel's bounds predication
      // supplies the zero-padding of the dilated gy on both ends (incl. rows
      // past the last forward window, where forward's floor division
      // dropped input).
      auto gx = canvas();
      conv2d_fwd_into(gyd, wt, gx, H, W, 1, 1, pph, ppw, dh, dw, groups);
      return gx;
    }
  }
}

// pre / pre_kind: what conv2d_dgrad_prep returned for this weight, if any
at::Tensor conv2d_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                        int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                        int64_t dh, int64_t dw, int64_t groups,
                        c10::optional<at::Tensor> pre, int64_t pre_kind) {
  return conv2d_dgrad_run(
      dgrad_route_of(gy, w, H, W, sh, sw, ph, pw, dh, dw, groups, nullptr),
      gy, w, H, W, sh, sw, ph, pw, dh, dw, groups,
      pre.has_value() ? &*pre : nullptr, pre_kind);
}

// Forward-time dgrad weight-transform precompute (launched on a side
// stream during the forward pass so backward's critical path skips the
// flip kernels). Returns {transformed_weight, kind}: the kind is the
// route's wkind (1 = span-padded flat flip, 0 = plain flipT).
std::tuple<at::Tensor, int64_t> conv2d_dgrad_prep(
    at::Tensor w, int64_t Kt0, int64_t sh, int64_t sw, int64_t ph,
    int64_t pw, int64_t dh, int64_t dw, int64_t groups) {
  const int S = w.size(3);
  const int wkind =
      dgrad_route(Kt0, w.size(1), w.size(2), S, sh, sw, ph, pw, dh, dw,
                  groups, w.scalar_type() == at::kBFloat16, false)
          .wkind;
  if (wkind == 1) {
    const int SPAN64 = (S * (int)(Kt0 / groups) + 63) / 64 * 64;
    return {weight_flip_t_span(w, groups, SPAN64), 1};
  }
  return {weight_flip_t(w, groups), 0};
}

// The route a dgrad with these operands takes, as (name, wkind, acc);
// launches nothing (shapes and dtypes only, so meta tensors work).
std::tuple<std::string, int64_t, bool> conv2d_dgrad_route(
    at::Tensor gy, at::Tensor w, int64_t H, int64_t W, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t groups,
    c10::optional<at::Tensor> into) {
  const DgradRoute rt =
      dgrad_route_of(gy, w, H, W, sh, sw, ph, pw, dh, dw, groups,
                     into.has_value() ? &*into : nullptr);
  return {dgrad_kind_name(rt.kind), rt.wkind, rt.acc};
}

// Residual-fork gradient accumulation (docs/ARCHITECTURE.md "Round-2
// status"): compute this conv's dgrad and ADD it into `into` — the other
// fork branch's already-computed gradient — inside the dgrad epilogue
// (+1 read stream) instead of autograd's separate 2-read/1-write
// elementwise add over the whole gx. Returns {tensor, flag}: flag 1 means
// `into` now holds the sum; flag 0 means the route has no ACC epilogue and
// the returned tensor is a FRESH gx (caller must add).
std::tuple<at::Tensor, int64_t> conv2d_dgrad_acc(
    at::Tensor gy, at::Tensor w, int64_t H, int64_t W, int64_t sh, int64_t sw,
    int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t groups,
    at::Tensor into, c10::optional<at::Tensor> pre, int64_t pre_kind) {
  const DgradRoute rt =
      dgrad_route_of(gy, w, H, W, sh, sw, ph, pw, dh, dw, groups, &into);
  auto gx = conv2d_dgrad_run(rt, gy, w, H, W, sh, sw, ph, pw, dh, dw, groups,
                             pre.has_value() ? &*pre : nullptr, pre_kind,
                             &into);
  return {gx, rt.acc ? 1 : 0};
}
