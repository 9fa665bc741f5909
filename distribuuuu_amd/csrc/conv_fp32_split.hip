// fp32 convolution on the bf16 matrix pipe: the opt-in "high" fp32 precision
// (ops.set_fp32_precision, docs/ARCHITECTURE.md "fp32 split-bf16 conv").
//
// Every fp32 operand a is split once, at LDS staging, into two bf16 parts
//   hi = bf16(a)  (round to nearest even),  lo = bf16(a - float(hi)),
// |a - hi - lo| <= 2^-17 |a|, and each fp32 product is accumulated as
//   lo_a*hi_b + hi_a*lo_b + hi_a*hi_b          (lo_a*lo_b is dropped)
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: three 32-deep bf16
// MFMAs where the exact kernel (conv_fp32.hip) issues eight 4-deep fp32 ones.
// bf16 products are exact in fp32, so only the adds round:
//   err <= 2^-15 * sum|ab| + 2 n 2^-24 * sum|ab|   for an n-term output.
// +-Inf splits into hi = +-Inf, lo = NaN and so yields NaN where the exact
// kernel yields +-Inf; no instruction is spent on that.
//
// Kernels:
//   conv_igemm_f32s_kernel<EMIT>  fwd / dgrad engine, 128x128x32 tile, 4 waves
//                                 (2x2), 4x4 fragments, 48 MFMAs per wave and
//                                 k-step; groups, stride, dilation, pad
//                                 predication, strided/offset output scatter
//                                 and the BN-partials epilogue, under the
//                                 contract of conv_igemm_fp32_kernel.
//   conv_wgrad_f32s_kernel<DET>   64x64 (k x rsc) tile, k-steps of 32 pixels
//                                 staged [m][col] and read transposed with
//                                 ds_read_b64_tr_b16; split-m chunks meet by
//                                 fp32 atomics or ordered workspace slots.
//
// MFMA operands (lane = 16 * kq + il): A row il / B column il, k = 8 kq .. + 8;
// D column il, rows 4 kq .. + 4.
#include "common.h"
#include "conv_common.h"
#include "conv_route.h"

// packed fp32 math (v_pk_*_f32) is kept out of this file's kernels. Header
// helpers lack the attribute and would be called, not inlined: builtins only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4s;
typedef __attribute__((ext_vector_type(2))) float f32x2s;
typedef __bf16 bf16x2s __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8s __attribute__((ext_vector_type(8)));

// q = (m * magic) >> 47 == m / d exactly for m * d < 2^47
DEV_INLINE int magic_div_s(int m, unsigned long long magic) {
  return (int)(((unsigned long long)(unsigned)m * magic) >> 47);
}
inline unsigned long long magic_of(int64_t d) {
  return ((1ULL << 47) / (unsigned long long)d) + 1;
}

// two floats -> one dword of {hi, hi} and one of {lo, lo} bf16 pairs
// (v_cvt_pk_bf16_f32 rounds to nearest even and keeps NaN a NaN). A zero
// splits into two zeros, so a zero-filled tail is zero in both images.
DEV_INLINE void split2(unsigned u0, unsigned u1, unsigned& hi, unsigned& lo) {
  const float f0 = __builtin_bit_cast(float, u0);
  const float f1 = __builtin_bit_cast(float, u1);
  hi = __builtin_bit_cast(
      unsigned, __builtin_convertvector(f32x2s{f0, f1}, bf16x2s));
  const float h0 = __builtin_bit_cast(float, hi << 16);
  const float h1 = __builtin_bit_cast(float, hi & 0xffff0000u);
  lo = __builtin_bit_cast(
      unsigned, __builtin_convertvector(f32x2s{f0 - h0, f1 - h1}, bf16x2s));
}

// 8 floats (two 16-byte loads) -> 16 bytes of hi and 16 bytes of lo
DEV_INLINE void split8(const uint4& a, const uint4& b, uint4& hi, uint4& lo) {
  split2(a.x, a.y, hi.x, lo.x);
  split2(a.z, a.w, hi.y, lo.y);
  split2(b.x, b.y, hi.z, lo.z);
  split2(b.z, b.w, hi.w, lo.w);
}

DEV_INLINE bf16x8s lds_frag(const char* p) {
  return __builtin_bit_cast(bf16x8s, *reinterpret_cast<const uint4*>(p));
}

DEV_INLINE f32x4s mfma3(bf16x8s ahi, bf16x8s alo, bf16x8s bhi, bf16x8s blo,
                        f32x4s acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bhi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, blo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bhi, acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// forward / dgrad engine
// ---------------------------------------------------------------------------
constexpr int SBM = 128, SBN = 128, SBK = 32;
// bf16 row of 32 k plus 8 pad elements = 80 bytes = 20 dwords: the sixteen
// rows of a fragment read (16 bytes per lane) start 4 * (5 i mod 16) dwords
// apart and cover the 64 banks once
constexpr int SROW = (SBK + 8) * 2;
constexpr int SIMG = SBM * SROW;    // one bf16 image of one operand: 10 KiB
constexpr int SSTAGE = 4 * SIMG;    // A hi, A lo, B hi, B lo
constexpr int SLAB_LD = 68;         // epilogue slab row, as in conv_fp32.hip

// the fields of conv_fp32.hip's ConvF32Params, plus the staging magic
struct ConvF32SParams {
  const float* x;  // [N,H,W,Ct] NHWC
  const float* w;  // [Kt,R,S,Cg]
  float* y;        // [N,HoA,WoA,Kt]
  int N, H, W, Ct, Kt;
  int R, S, Cg, Kg;
  int sh, sw, ph, pw, dh, dw;
  int Ho, Wo;
  int HoA, WoA, osh, osw, oh0, ow0;
  int M, nspan, ksteps;
  int tiles_m;
  float* part;  // EMIT: [tiles_m*2, 2*Kt]
  unsigned long long magicCg;
};

template <bool EMIT>
__global__ __launch_bounds__(256) void conv_igemm_f32s_kernel(
    ConvF32SParams p) {
  const int g = blockIdx.z;
  int tile_m = blockIdx.x;
  const int tile_n = blockIdx.y;
  {  // XCD-aware bijective remap over m-tiles
    const int nwg = p.tiles_m;
    const int q = nwg / 8, r8 = nwg % 8;
    const int xcd = tile_m % 8, idx = tile_m / 8;
    tile_m = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + idx;
  }

  // ONE shared object: two stages of four images; the epilogue's four
  // 16 x 68 fp32 slabs reuse its head
  __shared__ __align__(16) char smem[2 * SSTAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int il = lane & 15, kq = lane >> 4;

  // staging: thread t owns the 8-float group q8 = t & 3 of rows t >> 2 and
  // (t >> 2) + 64 of both operands, so one (s, c) decomposition per k-step
  // serves its four 32-byte loads
  const int srow = tid >> 2;
  const int scol8 = (tid & 3) << 3;
  const int SCg = p.S * p.Cg;
  int64_t abase[2], bbase[2];
  int ah[2], aw[2];
  bool arow_ok[2], brow_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = tile_m * SBM + srow + i * 64;
    arow_ok[i] = m < p.M;
    const int mm = arow_ok[i] ? m : 0;
    const int n = mm / (p.Ho * p.Wo);
    const int rem = mm - n * (p.Ho * p.Wo);
    ah[i] = (rem / p.Wo) * p.sh - p.ph;
    aw[i] = (rem % p.Wo) * p.sw - p.pw;
    abase[i] = (((int64_t)n * p.H + ah[i]) * p.W + aw[i]) * p.Ct + g * p.Cg;
    const int k = tile_n * SBN + srow + i * 64;
    brow_ok[i] = k < p.Kg;
    bbase[i] = (int64_t)(g * p.Kg + (brow_ok[i] ? k : 0)) * p.R * SCg;
  }
  const int wroff = srow * SROW + scol8 * 2;

  uint4 regA[2][2], regB[2][2];
  int lr = 0, lsp = 0;  // (r, span index) of the next k-step to load
  auto stage_load = [&]() {
    const int span = lsp * SBK + scol8;
    const bool span_ok = span < SCg;  // S*Cg % 8 == 0: a group is in or out
    const int s = span_ok ? magic_div_s(span, p.magicCg) : 0;
    const int c = span - s * p.Cg;
    const int64_t aoff = ((int64_t)lr * p.dh * p.W + s * p.dw) * p.Ct + c;
    const int64_t boff = (int64_t)lr * SCg + span;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int h = ah[i] + lr * p.dh;
      const int w_ = aw[i] + s * p.dw;
      const bool ok = arow_ok[i] && span_ok && h >= 0 && h < p.H && w_ >= 0 &&
                      w_ < p.W;
      const float* ap = p.x + abase[i] + aoff;
      regA[i][0] = ok ? *reinterpret_cast<const uint4*>(ap) : uint4{0, 0, 0, 0};
      regA[i][1] =
          ok ? *reinterpret_cast<const uint4*>(ap + 4) : uint4{0, 0, 0, 0};
      const bool okb = brow_ok[i] && span_ok;
      const float* bp = p.w + bbase[i] + boff;
      regB[i][0] =
          okb ? *reinterpret_cast<const uint4*>(bp) : uint4{0, 0, 0, 0};
      regB[i][1] =
          okb ? *reinterpret_cast<const uint4*>(bp + 4) : uint4{0, 0, 0, 0};
    }
    if (++lsp == p.nspan) {
      lsp = 0;
      ++lr;
    }
  };
  // the split happens here, once per element: predicated-off groups are
  // zeros in registers and are WRITTEN as zeros into both images
  auto stage_write = [&](int buf) {
    char* st = smem + buf * SSTAGE + wroff;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint4 hi, lo;
      split8(regA[i][0], regA[i][1], hi, lo);
      *reinterpret_cast<uint4*>(st + i * 64 * SROW) = hi;
      *reinterpret_cast<uint4*>(st + SIMG + i * 64 * SROW) = lo;
      split8(regB[i][0], regB[i][1], hi, lo);
      *reinterpret_cast<uint4*>(st + 2 * SIMG + i * 64 * SROW) = hi;
      *reinterpret_cast<uint4*>(st + 3 * SIMG + i * 64 * SROW) = lo;
    }
  };

  f32x4s acc[4][4] = {};
  stage_load();
  stage_write(0);
  if (p.ksteps > 1) stage_load();
  __syncthreads();

  // stage ks+1 is written while stage ks is read: every wave left stage
  // ks-1 (the same buffer) at the barrier that ended the previous step
  int cur = 0;
  const int aoffl = (wm * 64 + il) * SROW + kq * 16;
  const int boffl = 2 * SIMG + (wn * 64 + il) * SROW + kq * 16;
  for (int ks = 0; ks < p.ksteps; ++ks) {
    if (ks + 1 < p.ksteps) {
      stage_write(cur ^ 1);
      if (ks + 2 < p.ksteps) stage_load();
    }
    const char* st = smem + cur * SSTAGE;
    bf16x8s ahi[4], alo[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      ahi[mi] = lds_frag(st + aoffl + mi * 16 * SROW);
      alo[mi] = lds_frag(st + aoffl + SIMG + mi * 16 * SROW);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const bf16x8s bhi = lds_frag(st + boffl + ni * 16 * SROW);
      const bf16x8s blo = lds_frag(st + boffl + SIMG + ni * 16 * SROW);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[mi][ni] = mfma3(ahi[mi], alo[mi], bhi, blo, acc[mi][ni]);
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: per-wave fp32 slab restage -> 16-wide float stores
  float* slab = reinterpret_cast<float*>(smem) + wid * (16 * SLAB_LD);
  const int HoWo = p.Ho * p.Wo;
  const int er = lane >> 2;
  const int ec = (lane & 3) << 4;
  const bool vec_ok = ((p.Kt | p.Kg) & 3) == 0;
  float ps = 0.f, pq = 0.f;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        slab[(kq * 4 + rr) * SLAB_LD + ni * 16 + il] = acc[mi][ni][rr];
    __builtin_amdgcn_wave_barrier();
    const int m = tile_m * SBM + wm * 64 + mi * 16 + er;
    if (m < p.M) {
      const int n = m / HoWo;
      const int rem = m - n * HoWo;
      const int64_t obase =
          (((int64_t)n * p.HoA + (rem / p.Wo) * p.osh + p.oh0) * p.WoA +
           (rem % p.Wo) * p.osw + p.ow0) * p.Kt + g * p.Kg;
      const int k0 = tile_n * SBN + wn * 64 + ec;
      if (vec_ok && k0 + 16 <= p.Kg) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<uint4*>(&p.y[obase + k0 + q * 4]) =
              *reinterpret_cast<const uint4*>(&slab[er * SLAB_LD + ec + q * 4]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (k0 + j < p.Kg) p.y[obase + k0 + j] = slab[er * SLAB_LD + ec + j];
      }
    }
    if (EMIT) {
      // fp32 outputs are stored unrounded: sum the slab values directly
      const int base = tile_m * SBM + wm * 64 + mi * 16;
      const int left = p.M - base;
      const int rows_valid = left < 16 ? left : 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r < rows_valid) {
          const float v = slab[r * SLAB_LD + lane];
          ps += v;
          pq += v * v;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (EMIT) {
    // bn_partial_store's contract (common.h), written out: a header helper
    // would be a call from this file's functions
    const int kbase = tile_n * SBN + wn * 64;
    const int64_t slot =
        (int64_t)(tile_m * 2 + wm) * 2 * p.Kt + g * p.Kg + kbase;
    if (lane < p.Kg - kbase) {  // lane < 64 already
      p.part[slot + lane] = ps;
      p.part[slot + p.Kt + lane] = pq;
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: gw[k][rsc] = sum_m gy[m][k] * patch(x)[m][rsc]
// ---------------------------------------------------------------------------
constexpr int WS_BM = 64;        // k rows per tile
constexpr int WS_BN = 64;        // rsc cols per tile
constexpr int WS_BK = 32;        // pixels per k-step
constexpr int WS_CHUNK = 32;     // k-steps per split-m chunk (1024 pixels)
// [32 m][16 col] bf16 subtile: 32 rows x 32 B, padded to 1056 B so the
// 8-lane b128 write groups land on distinct banks (wgrad.hip's layout)
constexpr int WS_SUBT = 1056;
constexpr int WS_IMG = 4 * WS_SUBT;   // [32 m][64 col]: 4 col-subtiles
constexpr int WS_STAGE = 4 * WS_IMG;  // gy hi, gy lo, x hi, x lo

struct WgradF32SParams {
  const float* x;   // [N,H,W,Ct]
  const float* gy;  // [N,Ho,Wo,Kt]
  float* gw;        // [Kt, R*S*Cg] zeroed fp32, or part[chunks][pstride]
  int N, H, W, Ct, Kt;
  int R, S, Cg, Kg;
  int sh, sw, ph, pw, dh, dw;
  int Ho, Wo;
  int M, RSC;
  int ktiles, ntiles, chunks;
  unsigned long long magicHoWo, magicWo;
  int64_t pstride;  // DET: workspace slot stride (0 otherwise)
};

// two transposed reads: this lane supplies the addresses of rows
// 8 kq + (il >> 2) and + 4 of a subtile, word il & 3, and receives 8
// consecutive m of column il (lane semantics: docs/ARCHITECTURE.md "Weight
// gradient")
union TrFragS {
  uint2 h[2];
  bf16x8s v;
};
DEV_INLINE void tr_issue(unsigned a, TrFragS& f) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:128"
      : "=&v"(f.h[0]), "=&v"(f.h[1])
      : "v"(a)
      : "memory");
}

template <bool DET>
__global__ __launch_bounds__(256) void conv_wgrad_f32s_kernel(
    WgradF32SParams p) {
  const int g = blockIdx.z;
  const int ktile = blockIdx.x % p.ktiles;
  const int ntile = blockIdx.x / p.ktiles;
  const int chunk = blockIdx.y;

  __shared__ __align__(16) char smem[2 * WS_STAGE];
  const unsigned smem_base = (unsigned)(unsigned long long)&smem[0];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int il = lane & 15, kq = lane >> 4;

  // staging: thread t loads 8 floats of pixel t >> 3 at column (t & 7) * 8
  const int sml = tid >> 3;
  const int scol8 = (tid & 7) << 3;
  const int SCg = p.S * p.Cg;
  const int rsc = ntile * WS_BN + scol8;
  const bool rsc_ok = rsc < p.RSC;  // Cg % 8 == 0: a group is in or out
  const int br = rsc_ok ? rsc / SCg : 0;
  const int brem = rsc - br * SCg;
  const int bs = brem / p.Cg;
  const int bc = brem - bs * p.Cg;
  const int kcol = ktile * WS_BM + scol8;
  const bool k_ok = kcol < p.Kg;    // Kg % 8 == 0
  const int wroff = (scol8 >> 4) * WS_SUBT + sml * 32 + (scol8 & 15) * 2;

  const int m0 = chunk * (WS_CHUNK * WS_BK);
  const int HoWo = p.Ho * p.Wo;
  const int mleft = (p.M - m0 + WS_BK - 1) / WS_BK;
  const int msteps = mleft < WS_CHUNK ? mleft : WS_CHUNK;

  uint4 regG[2], regX[2];
  auto stage_load = [&](int ms) {
    const int m = m0 + ms * WS_BK + sml;
    const bool m_ok = m < p.M;
    const int mm = m_ok ? m : 0;
    const int n = magic_div_s(mm, p.magicHoWo);
    const int rem = mm - n * HoWo;
    const int ho = magic_div_s(rem, p.magicWo);
    const int wo = rem - ho * p.Wo;
    const float* gp = p.gy + (int64_t)mm * p.Kt + g * p.Kg + kcol;
    const bool okg = m_ok && k_ok;
    regG[0] = okg ? *reinterpret_cast<const uint4*>(gp) : uint4{0, 0, 0, 0};
    regG[1] = okg ? *reinterpret_cast<const uint4*>(gp + 4) : uint4{0, 0, 0, 0};
    const int h = ho * p.sh - p.ph + br * p.dh;
    const int w_ = wo * p.sw - p.pw + bs * p.dw;
    const bool okx =
        m_ok && rsc_ok && h >= 0 && h < p.H && w_ >= 0 && w_ < p.W;
    const float* xp =
        p.x + (((int64_t)n * p.H + h) * p.W + w_) * p.Ct + g * p.Cg + bc;
    regX[0] = okx ? *reinterpret_cast<const uint4*>(xp) : uint4{0, 0, 0, 0};
    regX[1] = okx ? *reinterpret_cast<const uint4*>(xp + 4) : uint4{0, 0, 0, 0};
  };
  // out-of-image and tail pixels are zeros in registers and are written as
  // zeros into both images
  auto stage_write = [&](int buf) {
    char* st = smem + buf * WS_STAGE + wroff;
    uint4 hi, lo;
    split8(regG[0], regG[1], hi, lo);
    *reinterpret_cast<uint4*>(st) = hi;
    *reinterpret_cast<uint4*>(st + WS_IMG) = lo;
    split8(regX[0], regX[1], hi, lo);
    *reinterpret_cast<uint4*>(st + 2 * WS_IMG) = hi;
    *reinterpret_cast<uint4*>(st + 3 * WS_IMG) = lo;
  };

  f32x4s acc[2][2] = {};
  stage_load(0);
  stage_write(0);
  if (msteps > 1) stage_load(1);
  __syncthreads();

  // this lane's transposed-read address inside a subtile
  const unsigned traddr = (kq * 8 + (il >> 2)) * 32 + (il & 3) * 8;
  int cur = 0;
  for (int ms = 0; ms < msteps; ++ms) {
    if (ms + 1 < msteps) {
      stage_write(cur ^ 1);
      if (ms + 2 < msteps) stage_load(ms + 2);
    }
    const unsigned st = smem_base + (unsigned)(cur * WS_STAGE) + traddr;
    TrFragS ghi[2], glo[2], xhi[2], xlo[2];
    // the stage's ds_writes above are ordered before these reads by the
    // "memory" clobber; the counted wait below covers all 16 reads
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned ga = st + (wm * 2 + i) * WS_SUBT;
      tr_issue(ga, ghi[i]);
      tr_issue(ga + WS_IMG, glo[i]);
      const unsigned xa = st + 2 * WS_IMG + (wn * 2 + i) * WS_SUBT;
      tr_issue(xa, xhi[i]);
      tr_issue(xa + WS_IMG, xlo[i]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = mfma3(ghi[mi].v, glo[mi].v, xhi[ni].v, xlo[ni].v,
                            acc[mi][ni]);
    __syncthreads();
    cur ^= 1;
  }

  // D: col = il, row = 4 kq + rr. Atomic accumulate, or (DET) plain stores
  // into this chunk's slot: every (chunk, k < Kg, col < RSC) has one writer
  float* dst = DET ? p.gw + (int64_t)chunk * p.pstride : p.gw;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int k = ktile * WS_BM + wm * 32 + mi * 16 + kq * 4 + rr;
      if (k >= p.Kg) continue;
      const int64_t rowbase = (int64_t)(g * p.Kg + k) * p.RSC;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = ntile * WS_BN + wn * 32 + ni * 16 + il;
        if (col < p.RSC) {
          if constexpr (DET)
            dst[rowbase + col] = acc[mi][ni][rr];
          else
            __hip_atomic_fetch_add(&dst[rowbase + col], acc[mi][ni][rr],
                                   __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Same arguments and results as conv2d_fwd_into_fp32, which calls this when
// fp32_conv_route says "split".
at::Tensor conv2d_fwd_into_f32s(at::Tensor x, at::Tensor w, at::Tensor y,
                                int64_t Ho, int64_t Wo, int64_t sh, int64_t sw,
                                int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                                int64_t groups, int64_t osh, int64_t osw,
                                int64_t oh0, int64_t ow0,
                                at::Tensor* part_out) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == at::kFloat && w.scalar_type() == at::kFloat &&
                  y.scalar_type() == at::kFloat,
              "conv2d_fwd_f32s: fp32 only");
  check_nhwc(x, "x");
  check_nhwc(w, "w");
  const int N = x.size(0), Ct = x.size(1), H = x.size(2), W = x.size(3);
  const int Kt = w.size(0), Cg = w.size(1), R = w.size(2), S = w.size(3);
  TORCH_CHECK(Ct == Cg * groups, "channel/group mismatch");
  TORCH_CHECK(Cg % 8 == 0, "conv2d_fwd_f32s: per-group C must be 8-aligned");
  const int Kg = Kt / groups;
  TORCH_CHECK(y.size(0) == N && y.size(1) == Kt &&
                  (Ho - 1) * osh + oh0 < y.size(2) &&
                  (Wo - 1) * osw + ow0 < y.size(3),
              "conv2d_fwd_f32s: output scatter leaves y");
  ConvF32SParams p;
  p.x = (const float*)x.data_ptr();
  p.w = (const float*)w.data_ptr();
  p.y = (float*)y.data_ptr();
  p.N = N; p.H = H; p.W = W; p.Ct = Ct; p.Kt = Kt;
  p.R = R; p.S = S; p.Cg = Cg; p.Kg = Kg;
  p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.Ho = Ho; p.Wo = Wo;
  p.HoA = y.size(2); p.WoA = y.size(3);
  p.osh = osh; p.osw = osw; p.oh0 = oh0; p.ow0 = ow0;
  p.M = N * Ho * Wo;
  p.nspan = (S * Cg + SBK - 1) / SBK;
  p.ksteps = R * p.nspan;
  p.tiles_m = (p.M + SBM - 1) / SBM;
  p.part = nullptr;
  p.magicCg = magic_of(Cg);
  dim3 grid(p.tiles_m, (Kg + SBN - 1) / SBN, groups);
  if (part_out != nullptr) {
    *part_out = at::empty({(int64_t)p.tiles_m * 2, (int64_t)2 * Kt},
                          x.options().dtype(at::kFloat));
    p.part = part_out->data_ptr<float>();
    hipLaunchKernelGGL(conv_igemm_f32s_kernel<true>, grid, dim3(256), 0,
                       cur_stream(), p);
  } else {
    hipLaunchKernelGGL(conv_igemm_f32s_kernel<false>, grid, dim3(256), 0,
                       cur_stream(), p);
  }
  return y;
}

// Same arguments and result layout as conv2d_wgrad_fp32, which calls this
// when fp32_conv_route says "split".
at::Tensor conv2d_wgrad_f32s(at::Tensor gy, at::Tensor x, int64_t R, int64_t S,
                             int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                             int64_t dh, int64_t dw, int64_t groups) {
  CHECK_GPU(gy);
  TORCH_CHECK(gy.scalar_type() == at::kFloat && x.scalar_type() == at::kFloat,
              "wgrad_f32s: fp32 only");
  check_nhwc(gy, "gy");
  check_nhwc(x, "x");
  const int N = x.size(0), Ct = x.size(1), H = x.size(2), W = x.size(3);
  const int Kt = gy.size(1), Ho = gy.size(2), Wo = gy.size(3);
  const int Cg = Ct / groups, Kg = Kt / groups;
  TORCH_CHECK(Cg % 8 == 0 && Kg % 8 == 0, "wgrad_f32s: Cg/Kg 8-aligned");
  TORCH_CHECK(gy.size(0) == N, "wgrad_f32s: batch mismatch");
  WgradF32SParams p;
  p.x = (const float*)x.data_ptr();
  p.gy = (const float*)gy.data_ptr();
  p.N = N; p.H = H; p.W = W; p.Ct = Ct; p.Kt = Kt;
  p.R = R; p.S = S; p.Cg = Cg; p.Kg = Kg;
  p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.Ho = Ho; p.Wo = Wo;
  p.M = N * Ho * Wo;
  p.RSC = R * S * Cg;
  p.ktiles = (Kg + WS_BM - 1) / WS_BM;
  p.ntiles = (p.RSC + WS_BN - 1) / WS_BN;
  p.chunks = (p.M + WS_CHUNK * WS_BK - 1) / (WS_CHUNK * WS_BK);
  p.magicHoWo = magic_of((int64_t)Ho * Wo);
  p.magicWo = magic_of(Wo);
  const bool det = is_deterministic();  // sampled per launch
  at::Tensor gwf, part;
  if (det) {
    gwf = at::empty({(int64_t)Kt, p.RSC}, x.options());
    part = at::empty({(int64_t)p.chunks, (int64_t)Kt * p.RSC}, x.options());
    p.gw = part.data_ptr<float>();
    p.pstride = (int64_t)Kt * p.RSC;
  } else {
    gwf = at::zeros({(int64_t)Kt, p.RSC}, x.options());
    p.gw = gwf.data_ptr<float>();
    p.pstride = 0;
  }
  dim3 grid(p.ktiles * p.ntiles, p.chunks, groups);
  if (det) {
    hipLaunchKernelGGL(conv_wgrad_f32s_kernel<true>, grid, dim3(256), 0,
                       cur_stream(), p);
    ordered_reduce<float>(part.data_ptr<float>(), gwf.data_ptr<float>(),
                          p.chunks, (int64_t)Kt * p.RSC, 1.f);
  } else {
    hipLaunchKernelGGL(conv_wgrad_f32s_kernel<false>, grid, dim3(256), 0,
                       cur_stream(), p);
  }
  // [Kt, RSC] rows are already [Kt][R][S][Cg] channels_last order
  return gwf.reshape({Kt, (int64_t)R, (int64_t)S, Cg})
      .permute({0, 3, 1, 2})
      .contiguous(at::MemoryFormat::ChannelsLast);
}
