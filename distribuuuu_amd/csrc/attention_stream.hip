// Streaming BoTNet MHSA for feature maps above 16x16 (256 < L = H*W <= 1024,
// H, W <= 32): forward and backward with an online softmax, so neither the
// probabilities P nor dS ever reach global memory. attention.hip keeps a
// whole score row in registers and stores P [B, L, L] for its backward; at
// L = 576 .. 1024 that tensor alone is hundreds of MB per layer.
//
// Math (tests/mhsa_ref.py): pixel x = hx * W + wx,
//   S[x, y] = scale q[x].k[y] + RW[x][wy-wx+W-1] + RH[x][hy-hx+H-1]
//   RW = scale q rel_w^T, RH = scale q rel_h^T, P = softmax(S), O = P v
//   dV = P^T dO, dP = dO v^T, dS = P (dP - delta), delta[x] = dO[x].O[x]
//   dQ = scale (dS k + dRW rel_w + dRH rel_h), dK = scale dS^T q
//   dRW[x, m] = sum_{y: wy-wx+W-1 == m} dS[x, y], grw = scale dRW^T q
//
// Every kernel: 256 threads, wave w owns rows 16 w .. + 16 of a 64-row block
// tile and streams 64-row tiles of the other side. A streamed tile [64][D] is
// loaded global -> registers (the next tile's loads are issued right after
// the barrier and land under the current tile's MFMAs) -> LDS rows of D + 8
// bf16, once per block for all four waves. It serves both as the NT operand
// (16-byte row reads, reduction over D) and, through ds_read_b64_tr_b16, as
// the key-contiguous operand of the second GEMM (reduction over the tile's
// rows), so no [B, D, L] permute-copy of k or v exists. Transposed read (lane
// semantics: wgrad.hip): lane (il, kq) addresses the 8-byte word of row
// 8 kq + il / 4 (and + 4), columns 4 (il % 4) .. + 4 of a 16-column group and
// receives rows 8 kq .. + 8 of column il.
//
// MFMA v_mfma_f32_16x16x32_bf16, lane = 16 kq + il: A row il / B column il,
// k = 8 kq .. + 8; D column il, rows 4 kq .. + 4.
//
//   mhsa_stream_fwd_kernel     block (b, q tile). Prologue: the wave's 16 rows
//     of RW / RH by MFMA against rel_w / rel_h [M, D] straight from global
//     (D-contiguous = NT operand), kept fp32 in LDS. Per key tile: S by MFMA,
//     rel add from LDS, key tail = -inf, running max m and per-lane partial
//     sum l in fp32, O accumulators rescaled by exp(m_old - m_new), the
//     unnormalised exp tile rounded to bf16 in the wave's slab, O += P~ V.
//     Epilogue: O / l as bf16, lse = m + log l.
//   mhsa_stream_bwd_q_kernel   block (b, q tile). Prologue: delta (fp32, also
//     to global), tables rebuilt. Per key tile: P = exp(S - lse),
//     dP = dO v^T, dS = P (dP - delta) -> bf16 slab, dQ += dS k (k read
//     transposed). The gather-sums run on the matrix unit too, with a
//     per-lane owner scheme and no atomics: sum_{y: wy == n} dS[x, y] is
//     dS times a 0 / 1 indicator [64 keys][W] that each lane builds in
//     registers, accumulated in fp32 fragments; dRW[x][m] is that sum shifted
//     by the row's own wx (dRH: hy, hx). Epilogue: the shifted sums go into
//     the wave's rows of the RW / RH tables, dQ = scale (dQ + dRW rel_w +
//     dRH rel_h); dRW / dRH to global fp32 [B * L, M].
//   mhsa_stream_bwd_kv_kernel  block (b, key tile), streams q tiles: tables
//     of the q tile rebuilt by MFMA, S^T = k q^T and dP^T = v dO^T (both
//     operands D-contiguous), P^T and dS^T as bf16 in the wave's slabs,
//     dV += P^T dO and dK += dS^T q with the q / dO tiles read transposed. A
//     block owns its dK / dV rows for the whole loop: no atomics.
//   mhsa_stream_rel_grad_kernel  grw / grh for M <= 63 (attention.hip's
//     kernel holds M <= 32): fp32 atomics, or per-block workspace slots and
//     ordered_reduce in deterministic mode.
//
// LDS map at D = 128 (bytes; kernels are launched with dynamic LDS and, above
// 64 KB, hipFuncAttributeMaxDynamicSharedMemorySize):
//                       fwd      bwd_q    bwd_kv
//   tile A [64][136]   17408     17408    17408    (k | k | q)
//   tile B [64][136]   17408     17408    17408    (v | v | dO)
//   RW, RH [64][65] f32 33280    33280    33280
//   slabs 4x[16][72]    9216      9216    18432    (P~ | dS | P^T, dS^T)
//   delta / lse f32        -       256      512
//   total              77312     77568    87040
//   blocks per CU by LDS   2         2        1
// VGPRs + AGPRs at D = 128 (the extension's own hipcc flags with
// -Rpass-analysis=kernel-resource-usage; no spills): fwd 218 + 32, bwd_q
// 246 + 48, bwd_kv 256 + 71, i.e. 2 / 1 / 1 waves per SIMD: the backward
// kernels run one block per CU.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4t;
typedef __bf16 bf16x8t __attribute__((ext_vector_type(8)));

namespace {

constexpr int TQ = 64;  // rows of a block tile and of a streamed tile
constexpr int TS = 65;  // fp32 table row stride: M <= 63, odd against banks
constexpr int PS = 72;  // bf16 slab row stride (64 + 8: 16-byte rows)

struct StreamParams {
  const __hip_bfloat16* q;
  const __hip_bfloat16* k;
  const __hip_bfloat16* v;
  const __hip_bfloat16* o;     // backward: the forward's output
  const __hip_bfloat16* dO;
  const __hip_bfloat16* relw;  // [2W-1, D]
  const __hip_bfloat16* relh;  // [2H-1, D]
  __hip_bfloat16* out;         // forward
  float* lse;                  // [B, L]: written by fwd (may be null), read by bwd
  float* delta;                // [B, L]: written by bwd_q, read by bwd_kv
  __hip_bfloat16* dq;
  __hip_bfloat16* dk;
  __hip_bfloat16* dv;
  float* drw;                  // [B * L, 2W-1]
  float* drh;                  // [B * L, 2H-1]
  int B, L, H, W, MW, MH, heads;
  int64_t qpix, kpix, vpix, opix;  // elements per pixel (attention.hip)
  float scale;
};

DEV_INLINE int64_t srow(int b, int l, int L, int heads, int64_t pix, int D) {
  const int n = b / heads, hd = b - n * heads;
  return ((int64_t)n * L + l) * pix + (int64_t)hd * D;
}

DEV_INLINE bf16x8t zero8t() {
  union { uint4 u; bf16x8t v; } z;
  z.u = uint4{0, 0, 0, 0};
  return z.v;
}

// rows row0 .. + 64 of a strided-row tensor -> ND 16-byte chunks per thread
template <int ND>
DEV_INLINE void tile_load(uint4 (&r)[ND], const __hip_bfloat16* base, int b,
                          int row0, int L, int heads, int64_t pix, int tid) {
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int c = tid + i * 256;
    const int row = c / (4 * ND), c8 = (c % (4 * ND)) * 8;
    const int l = row0 + row;
    r[i] = l < L ? *reinterpret_cast<const uint4*>(
                       base + srow(b, l, L, heads, pix, 32 * ND) + c8)
                 : uint4{0, 0, 0, 0};  // tail rows are zeros
  }
}

template <int ND>
DEV_INLINE void tile_store(__hip_bfloat16* lds, const uint4 (&r)[ND], int tid) {
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int c = tid + i * 256;
    const int row = c / (4 * ND), c8 = (c % (4 * ND)) * 8;
    *reinterpret_cast<uint4*>(lds + row * (32 * ND + 8) + c8) = r[i];
  }
}

// A fragments of global row `l` (zeros when !ok)
template <int ND>
DEV_INLINE void row_frags(bf16x8t (&f)[ND], const __hip_bfloat16* base, int b,
                          int l, bool ok, int L, int heads, int64_t pix,
                          int kq) {
  const __hip_bfloat16* rp = base + srow(b, ok ? l : 0, L, heads, pix, 32 * ND);
#pragma unroll
  for (int c = 0; c < ND; ++c)
    f[c] = ok ? *reinterpret_cast<const bf16x8t*>(rp + c * 32 + kq * 8)
              : zero8t();
}

// acc[nt] = A (16 rows, registers) x tile rows 16 nt .. + 16 (NT, from LDS)
template <int ND>
DEV_INLINE void nt_tile(f32x4t (&acc)[4], const bf16x8t (&a)[ND],
                        const __hip_bfloat16* tile, int il, int kq) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    f32x4t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      const bf16x8t bfrag = *reinterpret_cast<const bf16x8t*>(
          tile + (nt * 16 + il) * (32 * ND + 8) + c * 32 + kq * 8);
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c], bfrag, s, 0, 0, 0);
    }
    acc[nt] = s;
  }
}

// tab[row0 + 4 kq + rr][m] = scale * A[row] . rel[m], m < M, fp32
template <int ND>
DEV_INLINE void build_table(float* tab, int row0, const bf16x8t (&a)[ND],
                            const __hip_bfloat16* rel, int M, float scale,
                            int il, int kq) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int m = nt * 16 + il;
    if (nt * 16 >= M) break;  // wave-uniform
    f32x4t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      const bf16x8t bfrag =
          m < M ? *reinterpret_cast<const bf16x8t*>(rel + m * (32 * ND) +
                                                    c * 32 + kq * 8)
                : zero8t();
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c], bfrag, s, 0, 0, 0);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)  // m <= 63 < TS
      tab[(row0 + kq * 4 + rr) * TS + m] = s[rr] * scale;
  }
}

// Two transposed fragments (tile rows 0..31 and 32..63) of one 16-column
// group; `a` is this lane's byte address of row 8 kq + il / 4, word il % 4.
template <int RSB>
DEV_INLINE void tr_read2(unsigned a, bf16x8t& f0, bf16x8t& f1) {
  union { uint2 h[2]; bf16x8t v; } u0, u1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %5\n\t"
      "ds_read_b64_tr_b16 %2, %6\n\t"
      "ds_read_b64_tr_b16 %3, %7\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(u0.h[0]), "=&v"(u0.h[1]), "=&v"(u1.h[0]), "=&v"(u1.h[1])
      : "v"(a), "v"(a + 4 * RSB), "v"(a + 32 * RSB), "v"(a + 36 * RSB)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  f0 = u0.v;
  f1 = u1.v;
}

DEV_INLINE unsigned tr_lane_addr(const __hip_bfloat16* tile, int rs, int il,
                                 int kq) {
  return (unsigned)(unsigned long long)tile +
         ((kq * 8 + (il >> 2)) * rs + (il & 3) * 4) * 2;
}

// acc[dt] += slab (16 rows x 64, A operand) x tile (64 rows x D, transposed)
template <int ND>
DEV_INLINE void tn_accum(f32x4t (&acc)[2 * ND], const __hip_bfloat16* slab,
                         unsigned tile_addr, int il, int kq) {
  const bf16x8t a0 =
      *reinterpret_cast<const bf16x8t*>(slab + il * PS + kq * 8);
  const bf16x8t a1 =
      *reinterpret_cast<const bf16x8t*>(slab + il * PS + 32 + kq * 8);
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) {
    bf16x8t b0, b1;
    tr_read2<(32 * ND + 8) * 2>(tile_addr + dt * 32, b0, b1);
    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[dt], 0, 0, 0);
    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[dt], 0, 0, 0);
  }
}

template <int ND>
constexpr int tile_bytes() { return TQ * (32 * ND + 8) * 2; }
constexpr int TAB_BYTES = TQ * TS * 4;
constexpr int SLAB_BYTES = 4 * 16 * PS * 2;

template <int ND>
constexpr int fwd_lds() { return 2 * tile_bytes<ND>() + 2 * TAB_BYTES + SLAB_BYTES; }
template <int ND>
constexpr int bwd_q_lds() {
  return 2 * tile_bytes<ND>() + 2 * TAB_BYTES + SLAB_BYTES + TQ * 4;
}
template <int ND>
constexpr int bwd_kv_lds() {
  return 2 * tile_bytes<ND>() + 2 * TAB_BYTES + 2 * SLAB_BYTES + 2 * TQ * 4;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_stream_fwd_kernel(StreamParams p) {
  constexpr int D = 32 * ND, RS = D + 8;
  extern __shared__ __align__(16) char smem[];
  __hip_bfloat16* Ks = reinterpret_cast<__hip_bfloat16*>(smem);
  __hip_bfloat16* Vs = Ks + TQ * RS;
  float* RW = reinterpret_cast<float*>(smem + 2 * tile_bytes<ND>());
  float* RH = RW + TQ * TS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  __hip_bfloat16* Pw =
      reinterpret_cast<__hip_bfloat16*>(RH + TQ * TS) + wid * 16 * PS;
  const int b = blockIdx.x;
  const int qrow_base = blockIdx.y * TQ + wid * 16;

  bf16x8t qfrag[ND];
  row_frags<ND>(qfrag, p.q, b, qrow_base + il, qrow_base + il < p.L, p.L,
                p.heads, p.qpix, kq);
  build_table<ND>(RW, wid * 16, qfrag, p.relw, p.MW, p.scale, il, kq);
  build_table<ND>(RH, wid * 16, qfrag, p.relh, p.MH, p.scale, il, kq);

  // this lane's 4 q rows: table rows pre-offset so that [wy] / [hy] index them
  const float* rwrow[4];
  const float* rhrow[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int qr = min(qrow_base + kq * 4 + rr, p.L - 1);  // pad rows: any
    const int hx = qr / p.W, wx = qr - hx * p.W;
    rwrow[rr] = RW + (wid * 16 + kq * 4 + rr) * TS + (p.W - 1 - wx);
    rhrow[rr] = RH + (wid * 16 + kq * 4 + rr) * TS + (p.H - 1 - hx);
  }

  float mrow[4], lrow[4];
  f32x4t oacc[2 * ND];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    mrow[rr] = -INFINITY;
    lrow[rr] = 0.f;
  }
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) oacc[dt] = f32x4t{0.f, 0.f, 0.f, 0.f};
  const unsigned vaddr = tr_lane_addr(Vs, RS, il, kq);

  const int nkt = (p.L + TQ - 1) / TQ;
  uint4 rk[ND], rv[ND];
  tile_load<ND>(rk, p.k, b, 0, p.L, p.heads, p.kpix, tid);
  tile_load<ND>(rv, p.v, b, 0, p.L, p.heads, p.vpix, tid);
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    tile_store<ND>(Ks, rk, tid);
    tile_store<ND>(Vs, rv, tid);
    __syncthreads();
    if (kt + 1 < nkt) {
      tile_load<ND>(rk, p.k, b, (kt + 1) * TQ, p.L, p.heads, p.kpix, tid);
      tile_load<ND>(rv, p.v, b, (kt + 1) * TQ, p.L, p.heads, p.vpix, tid);
    }
    f32x4t s[4];
    nt_tile<ND>(s, qfrag, Ks, il, kq);
    // rel add; keys past L get -inf (every tile holds at least one key < L,
    // so the running max is finite from the first tile on)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int kpos = kt * TQ + nt * 16 + il;
      const bool kok = kpos < p.L;
      const int kc = kok ? kpos : p.L - 1;
      const int hy = kc / p.W, wy = kc - hy * p.W;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        s[nt][rr] = kok ? s[nt][rr] * p.scale + rwrow[rr][wy] + rhrow[rr][hy]
                        : -INFINITY;
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float tmax = fmaxf(fmaxf(s[0][rr], s[1][rr]), fmaxf(s[2][rr], s[3][rr]));
#pragma unroll
      for (int st = 1; st < 16; st <<= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, st));
      const float mnew = fmaxf(mrow[rr], tmax);
      const float alpha = __expf(mrow[rr] - mnew);  // first tile: exp(-inf) = 0
      mrow[rr] = mnew;
      float rsum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float e = __expf(s[nt][rr] - mnew);
        rsum += e;
        Pw[(kq * 4 + rr) * PS + nt * 16 + il] = from_f32<__hip_bfloat16>(e);
      }
      lrow[rr] = lrow[rr] * alpha + rsum;  // per-lane partial of the row sum
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt) oacc[dt][rr] *= alpha;
    }
    __builtin_amdgcn_wave_barrier();
    tn_accum<ND>(oacc, Pw, vaddr, il, kq);
    __syncthreads();
  }

#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    float l = lrow[rr];
#pragma unroll
    for (int st = 1; st < 16; st <<= 1) l += __shfl_xor(l, st);
    const int qr = qrow_base + kq * 4 + rr;
    if (qr < p.L) {
      const float inv = 1.f / l;
      __hip_bfloat16* op = p.out + srow(b, qr, p.L, p.heads, p.opix, D) + il;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt)
        op[dt * 16] = from_f32<__hip_bfloat16>(oacc[dt][rr] * inv);
      if (p.lse != nullptr && il == 0)
        p.lse[(int64_t)b * p.L + qr] = mrow[rr] + logf(l);
    }
  }
}

// ---------------------------------------------------------------------------
// backward, q side
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_stream_bwd_q_kernel(StreamParams p) {
  constexpr int D = 32 * ND, RS = D + 8;
  extern __shared__ __align__(16) char smem[];
  __hip_bfloat16* Ks = reinterpret_cast<__hip_bfloat16*>(smem);
  __hip_bfloat16* Vs = Ks + TQ * RS;
  float* RW = reinterpret_cast<float*>(smem + 2 * tile_bytes<ND>());
  float* RH = RW + TQ * TS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  __hip_bfloat16* DSw =
      reinterpret_cast<__hip_bfloat16*>(RH + TQ * TS) + wid * 16 * PS;
  float* dl_s = reinterpret_cast<float*>(smem + 2 * tile_bytes<ND>() +
                                         2 * TAB_BYTES + SLAB_BYTES);
  const int b = blockIdx.x;
  const int qrow_base = blockIdx.y * TQ + wid * 16;

  bf16x8t qfrag[ND], dofrag[ND];
  {
    const int qr = qrow_base + il;
    const bool ok = qr < p.L;
    row_frags<ND>(qfrag, p.q, b, qr, ok, p.L, p.heads, p.qpix, kq);
    row_frags<ND>(dofrag, p.dO, b, qr, ok, p.L, p.heads, p.opix, kq);
    // delta[row il] = dO . O: 8 ND products per lane, then over the 4 kq
    bf16x8t ofrag[ND];
    row_frags<ND>(ofrag, p.o, b, qr, ok, p.L, p.heads, p.opix, kq);
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < ND; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) d += (float)dofrag[c][j] * (float)ofrag[c][j];
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if (kq == 0) {
      dl_s[wid * 16 + il] = d;
      if (ok) p.delta[(int64_t)b * p.L + qr] = d;
    }
  }
  build_table<ND>(RW, wid * 16, qfrag, p.relw, p.MW, p.scale, il, kq);
  build_table<ND>(RH, wid * 16, qfrag, p.relh, p.MH, p.scale, il, kq);
  __builtin_amdgcn_wave_barrier();

  // pad q rows (>= L) have q = dO = 0: P = exp(0 - 0), dP = delta = 0, dS = 0
  const float* rwrow[4];
  const float* rhrow[4];
  int wxr[4], hxr[4];
  float lse[4], dlt[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = wid * 16 + kq * 4 + rr;
    const int qr = qrow_base + kq * 4 + rr;
    const int qc = min(qr, p.L - 1);
    const int hx = qc / p.W, wx = qc - hx * p.W;
    rwrow[rr] = RW + row * TS + (p.W - 1 - wx);
    rhrow[rr] = RH + row * TS + (p.H - 1 - hx);
    wxr[rr] = wx;
    hxr[rr] = hx;
    lse[rr] = qr < p.L ? p.lse[(int64_t)b * p.L + qr] : 0.f;
    dlt[rr] = dl_s[row];
  }

  f32x4t dqacc[2 * ND];
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) dqacc[dt] = f32x4t{0.f, 0.f, 0.f, 0.f};
  // ew[j][x][n] = sum_{y: wy == 16 j + n} dS[x, y] (eh: hy), by MFMA against
  // 0 / 1 indicator fragments built in registers; dRW[x][m] is ew shifted by
  // the row's own wx. H, W >= 9 here (L > 256 with the other side <= 32).
  f32x4t ew[2], eh[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) ew[j] = eh[j] = f32x4t{0.f, 0.f, 0.f, 0.f};
  const unsigned kaddr = tr_lane_addr(Ks, RS, il, kq);

  const int nkt = (p.L + TQ - 1) / TQ;
  uint4 rk[ND], rv[ND];
  tile_load<ND>(rk, p.k, b, 0, p.L, p.heads, p.kpix, tid);
  tile_load<ND>(rv, p.v, b, 0, p.L, p.heads, p.vpix, tid);
#pragma unroll 1
  for (int kt = 0; kt < nkt; ++kt) {
    tile_store<ND>(Ks, rk, tid);
    tile_store<ND>(Vs, rv, tid);
    __syncthreads();
    if (kt + 1 < nkt) {
      tile_load<ND>(rk, p.k, b, (kt + 1) * TQ, p.L, p.heads, p.kpix, tid);
      tile_load<ND>(rv, p.v, b, (kt + 1) * TQ, p.L, p.heads, p.vpix, tid);
    }
    f32x4t s[4], dp[4];
    nt_tile<ND>(s, qfrag, Ks, il, kq);
    nt_tile<ND>(dp, dofrag, Vs, il, kq);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int kpos = kt * TQ + nt * 16 + il;
      const bool kok = kpos < p.L;
      const int kc = kok ? kpos : p.L - 1;
      const int hy = kc / p.W, wy = kc - hy * p.W;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float pv =
            kok ? __expf(s[nt][rr] * p.scale + rwrow[rr][wy] + rhrow[rr][hy] -
                         lse[rr])
                : 0.f;
        const float ds = pv * (dp[nt][rr] - dlt[rr]);
        DSw[(kq * 4 + rr) * PS + nt * 16 + il] = from_f32<__hip_bfloat16>(ds);
      }
    }
    __builtin_amdgcn_wave_barrier();
    tn_accum<ND>(dqacc, DSw, kaddr, il, kq);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const bf16x8t dsf = *reinterpret_cast<const bf16x8t*>(
          DSw + il * PS + kc * 32 + kq * 8);
      const int y0 = kt * TQ + kc * 32 + kq * 8;  // this lane's 8 keys
      const int h0 = y0 / p.W, w0 = y0 - h0 * p.W;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        union { unsigned short e[8]; bf16x8t v; } iw, ih;
#pragma unroll
        for (int e = 0; e < 8; ++e) {  // keys past L carry dS = 0
          const bool wrap = w0 + e >= p.W;
          const int wy = wrap ? w0 + e - p.W : w0 + e, hy = h0 + (wrap ? 1 : 0);
          iw.e[e] = wy == j * 16 + il ? 0x3F80 : 0;  // bf16 1.0
          ih.e[e] = hy == j * 16 + il ? 0x3F80 : 0;
        }
        if (j * 16 < p.W)
          ew[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, iw.v, ew[j], 0, 0, 0);
        if (j * 16 < p.H)
          eh[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, ih.v, eh[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // dRW / dRH into this wave's rows of the (now free) RW / RH tables
  float* dRW = RW;
  float* dRH = RH;
  for (int i = lane; i < 16 * TS; i += 64) {
    dRW[wid * 16 * TS + i] = 0.f;
    dRH[wid * 16 * TS + i] = 0.f;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = j * 16 + il;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = wid * 16 + kq * 4 + rr;
      if (n < p.W) dRW[row * TS + n - wxr[rr] + p.W - 1] = ew[j][rr];
      if (n < p.H) dRH[row * TS + n - hxr[rr] + p.H - 1] = eh[j][rr];
    }
  }
  __builtin_amdgcn_wave_barrier();
  // dQ = scale (dS k + dRW rel_w + dRH rel_h); rel rows stream through L1
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) {
    const int d = dt * 16 + il;
    f32x4t acc = dqacc[dt];
    for (int m = 0; m < p.MW; ++m) {
      const float r = to_f32(p.relw[m * D + d]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        acc[rr] += dRW[(wid * 16 + kq * 4 + rr) * TS + m] * r;
    }
    for (int m = 0; m < p.MH; ++m) {
      const float r = to_f32(p.relh[m * D + d]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        acc[rr] += dRH[(wid * 16 + kq * 4 + rr) * TS + m] * r;
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int qr = qrow_base + kq * 4 + rr;
      if (qr < p.L)
        p.dq[srow(b, qr, p.L, p.heads, p.qpix, D) + d] =
            from_f32<__hip_bfloat16>(acc[rr] * p.scale);
    }
  }
  for (int r = 0; r < 16; ++r) {
    const int qr = qrow_base + r;
    if (qr >= p.L) break;
    const int64_t grow = (int64_t)b * p.L + qr;
    if (lane < p.MW) p.drw[grow * p.MW + lane] = dRW[(wid * 16 + r) * TS + lane];
    if (lane < p.MH) p.drh[grow * p.MH + lane] = dRH[(wid * 16 + r) * TS + lane];
  }
}

// ---------------------------------------------------------------------------
// backward, k / v side
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_stream_bwd_kv_kernel(
    StreamParams p) {
  constexpr int D = 32 * ND, RS = D + 8;
  extern __shared__ __align__(16) char smem[];
  __hip_bfloat16* Qs = reinterpret_cast<__hip_bfloat16*>(smem);
  __hip_bfloat16* dOs = Qs + TQ * RS;
  float* RW = reinterpret_cast<float*>(smem + 2 * tile_bytes<ND>());
  float* RH = RW + TQ * TS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int il = lane & 15, kq = lane >> 4;
  __hip_bfloat16* PTw =
      reinterpret_cast<__hip_bfloat16*>(RH + TQ * TS) + wid * 16 * PS;
  __hip_bfloat16* DSTw = PTw + 4 * 16 * PS;
  float* lse_s = reinterpret_cast<float*>(smem + 2 * tile_bytes<ND>() +
                                          2 * TAB_BYTES + 2 * SLAB_BYTES);
  float* dl_s = lse_s + TQ;
  const int b = blockIdx.x;
  const int krow_base = blockIdx.y * TQ + wid * 16;

  // pad key rows (>= L) have k = v = 0: finite values, never stored
  bf16x8t kfrag[ND], vfrag[ND];
  row_frags<ND>(kfrag, p.k, b, krow_base + il, krow_base + il < p.L, p.L,
                p.heads, p.kpix, kq);
  row_frags<ND>(vfrag, p.v, b, krow_base + il, krow_base + il < p.L, p.L,
                p.heads, p.vpix, kq);
  int hy[4], wy[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int y = min(krow_base + kq * 4 + rr, p.L - 1);
    hy[rr] = y / p.W;
    wy[rr] = y - hy[rr] * p.W;
  }
  f32x4t dkacc[2 * ND], dvacc[2 * ND];
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) {
    dkacc[dt] = f32x4t{0.f, 0.f, 0.f, 0.f};
    dvacc[dt] = f32x4t{0.f, 0.f, 0.f, 0.f};
  }
  const unsigned qaddr = tr_lane_addr(Qs, RS, il, kq);
  const unsigned doaddr = tr_lane_addr(dOs, RS, il, kq);

  const int nqt = (p.L + TQ - 1) / TQ;
  uint4 rq[ND], rdo[ND];
  float r_lse = 0.f, r_dl = 0.f;
  auto issue = [&](int qt) {
    tile_load<ND>(rq, p.q, b, qt * TQ, p.L, p.heads, p.qpix, tid);
    tile_load<ND>(rdo, p.dO, b, qt * TQ, p.L, p.heads, p.opix, tid);
    if (tid < TQ) {
      const int x = qt * TQ + tid;
      r_lse = x < p.L ? p.lse[(int64_t)b * p.L + x] : 0.f;
      r_dl = x < p.L ? p.delta[(int64_t)b * p.L + x] : 0.f;
    }
  };
  issue(0);
#pragma unroll 1
  for (int qt = 0; qt < nqt; ++qt) {
    tile_store<ND>(Qs, rq, tid);
    tile_store<ND>(dOs, rdo, tid);
    if (tid < TQ) {
      lse_s[tid] = r_lse;
      dl_s[tid] = r_dl;
    }
    __syncthreads();
    if (qt + 1 < nqt) issue(qt + 1);
    {  // tables of this q tile: wave w builds rows 16 w .. + 16 for all waves
      bf16x8t qf[ND];
#pragma unroll
      for (int c = 0; c < ND; ++c)
        qf[c] = *reinterpret_cast<const bf16x8t*>(Qs + (wid * 16 + il) * RS +
                                                  c * 32 + kq * 8);
      build_table<ND>(RW, wid * 16, qf, p.relw, p.MW, p.scale, il, kq);
      build_table<ND>(RH, wid * 16, qf, p.relh, p.MH, p.scale, il, kq);
    }
    __syncthreads();
    f32x4t st[4], dpt[4];  // rows: this wave's keys; columns: the tile's q
    nt_tile<ND>(st, kfrag, Qs, il, kq);
    nt_tile<ND>(dpt, vfrag, dOs, il, kq);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int xl = nt * 16 + il;
      const int x = qt * TQ + xl;
      const bool xok = x < p.L;
      const int xc = xok ? x : p.L - 1;
      const int hx = xc / p.W, wx = xc - hx * p.W;
      const float* rwp = RW + xl * TS + (p.W - 1 - wx);
      const float* rhp = RH + xl * TS + (p.H - 1 - hx);
      const float lsex = lse_s[xl], dlx = dl_s[xl];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float pv =
            xok ? __expf(st[nt][rr] * p.scale + rwp[wy[rr]] + rhp[hy[rr]] - lsex)
                : 0.f;
        const float ds = pv * (dpt[nt][rr] - dlx);
        PTw[(kq * 4 + rr) * PS + xl] = from_f32<__hip_bfloat16>(pv);
        DSTw[(kq * 4 + rr) * PS + xl] = from_f32<__hip_bfloat16>(ds);
      }
    }
    __builtin_amdgcn_wave_barrier();
    tn_accum<ND>(dvacc, PTw, doaddr, il, kq);
    tn_accum<ND>(dkacc, DSTw, qaddr, il, kq);
    __syncthreads();
  }

#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int y = krow_base + kq * 4 + rr;
    if (y < p.L) {
      __hip_bfloat16* dkp = p.dk + srow(b, y, p.L, p.heads, p.kpix, D) + il;
      __hip_bfloat16* dvp = p.dv + srow(b, y, p.L, p.heads, p.vpix, D) + il;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt) {
        dkp[dt * 16] = from_f32<__hip_bfloat16>(dkacc[dt][rr] * p.scale);
        dvp[dt * 16] = from_f32<__hip_bfloat16>(dvacc[dt][rr]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// grw[m, d] = scale * sum_rows dRW[row, m] q[row, d], M <= 63
// ---------------------------------------------------------------------------
struct StreamRelGradParams {
  const float* dr;          // [rows, M]
  const __hip_bfloat16* q;  // strided rows
  float* out;               // [M, D] zeroed, or part[row blocks][M * D]
  int64_t pstride;          // workspace slot stride (deterministic mode)
  int64_t rows;
  int M, D, rows_per_block, heads, L;
  int64_t qpix;
  float scale;
};

// thread (half, d) holds its half of the m range (<= 32 columns) for one d:
// q[r, d] loads coalesce over d, dr[r, m] is uniform over the wave.
template <bool DET>
__global__ __launch_bounds__(256) void mhsa_stream_rel_grad_kernel(
    StreamRelGradParams p) {
  const int d = threadIdx.x & 127, half = threadIdx.x >> 7;
  const int mh = (p.M + 1) / 2;
  const int m0 = half * mh;
  const int mn = min(p.M - m0, mh);
  if (d >= p.D) return;
  float acc[32] = {};
  const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
  const int64_t r1 = min(r0 + p.rows_per_block, p.rows);
  int bb = (int)(r0 / p.L), ll = (int)(r0 - (int64_t)bb * p.L);
  for (int64_t r = r0; r < r1; ++r) {
    const float qv = to_f32(p.q[srow(bb, ll, p.L, p.heads, p.qpix, p.D) + d]);
    const float* dr = p.dr + r * p.M + m0;
#pragma unroll
    for (int m = 0; m < 32; ++m)
      if (m < mn) acc[m] += dr[m] * qv;
    if (++ll == p.L) {
      ll = 0;
      ++bb;
    }
  }
  float* dst = p.out + (DET ? (int64_t)blockIdx.x * p.pstride : 0);
#pragma unroll
  for (int m = 0; m < 32; ++m)
    if (m < mn)
      emit_partial<DET>(&dst[(int64_t)(m0 + m) * p.D + d], acc[m] * p.scale);
}

// grw / grh are cleared by a kernel, not hipMemsetAsync, so the backward can
// be recorded into a hipGraph
__global__ void mhsa_stream_zero_kernel(float* a, int na, float* c, int nc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) a[i] = 0.f;
  if (i < nc) c[i] = 0.f;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <auto KERN, int LDS>
void launch_stream(dim3 grid, const StreamParams& p) {
  // above 64 KB the dynamic-LDS limit must be raised, once per device
  static bool attr_done[64] = {};
  if (LDS > 65536) {
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64,
                "mhsa_stream: no current device");
    if (!attr_done[dev]) {
      const hipError_t err = hipFuncSetAttribute(
          (const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
      TORCH_CHECK(err == hipSuccess, "mhsa_stream: cannot raise dynamic LDS to ",
                  LDS, " bytes: ", hipGetErrorString(err));
      attr_done[dev] = true;
    }
  }
  hipLaunchKernelGGL(KERN, grid, dim3(256), LDS, cur_stream(), p);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "mhsa_stream: launch failed: ",
              hipGetErrorString(err));
}

// the last element a kernel touches through `t` lies inside its storage
void check_span(const at::Tensor& t, int64_t pixels, int64_t pix, int64_t width,
                const char* fn, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, fn, ": ", name,
              " must be a bf16 GPU tensor");
  TORCH_CHECK(pix >= width && pix % 8 == 0, fn, ": ", name,
              " pixel stride must be a multiple of 8 and >= heads*D, got ", pix);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, ": ",
              name, " must be 16-byte aligned");
  const int64_t need = t.storage_offset() + (pixels - 1) * pix + width;
  TORCH_CHECK((int64_t)(t.storage().nbytes() / 2) >= need, fn, ": ", name,
              " holds fewer than ", pixels, " pixels of stride ", pix);
}

// shared geometry checks; returns D
int check_geometry(const char* fn, const at::Tensor& rel_w,
                   const at::Tensor& rel_h, int64_t L, int64_t H, int64_t W,
                   int64_t B, int64_t heads) {
  TORCH_CHECK(rel_w.is_cuda() && rel_h.is_cuda() &&
                  rel_w.scalar_type() == at::kBFloat16 &&
                  rel_h.scalar_type() == at::kBFloat16 && rel_w.dim() == 2 &&
                  rel_h.dim() == 2 && rel_w.is_contiguous() &&
                  rel_h.is_contiguous(),
              fn, ": rel_w / rel_h must be contiguous 2-D bf16 GPU tensors");
  // build_table reads the table rows in 16-byte vectors
  TORCH_CHECK(reinterpret_cast<uintptr_t>(rel_w.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(rel_h.data_ptr()) % 16 == 0,
              fn, ": rel_w / rel_h must be 16-byte aligned");
  const int64_t D = rel_w.size(1);
  TORCH_CHECK(D == 32 || D == 64 || D == 96 || D == 128, fn,
              ": D must be 32, 64, 96 or 128, got ", D);
  TORCH_CHECK(H >= 1 && H <= 32 && W >= 1 && W <= 32, fn,
              ": H and W must be in [1, 32], got ", H, "x", W);
  TORCH_CHECK(L == H * W, fn, ": L = ", L, " != H*W = ", H * W);
  TORCH_CHECK(L > 256 && L <= 1024, fn, ": L must be in (256, 1024], got ", L,
              " (L <= 256 is served by mhsa_fwd / mhsa_bwd)");
  TORCH_CHECK(rel_w.size(0) == 2 * W - 1, fn, ": rel_w must be [2W-1, D]");
  TORCH_CHECK(rel_h.size(0) == 2 * H - 1 && rel_h.size(1) == D, fn,
              ": rel_h must be [2H-1, D]");
  TORCH_CHECK(heads >= 1 && B >= 1 && B % heads == 0, fn, ": B = ", B,
              " is not a positive multiple of heads = ", heads);
  return (int)D;
}

#define STREAM_ND_SWITCH(D, ...)                       \
  switch ((D) / 32) {                                  \
    case 1: { constexpr int ND = 1; __VA_ARGS__; break; } \
    case 2: { constexpr int ND = 2; __VA_ARGS__; break; } \
    case 3: { constexpr int ND = 3; __VA_ARGS__; break; } \
    default: { constexpr int ND = 4; __VA_ARGS__; break; } \
  }

}  // namespace

// q, k, v: bf16, rows addressed as base + ((n*L + l) * pix + hd * D) with
// b = n * heads + hd (attention.hip): heads = 1, pix = D is the dense
// [B, L, D] layout; heads > 1 reads the qkv convs' channels_last outputs in
// place (k is a view whose data pointer is the k half) and returns o as
// channels_last [N, heads*D, H, W]. N = q.numel() / (L * qpix). Returns
// {o, lse}; lse is fp32 [B, L], or empty when need_lse is false.
std::vector<at::Tensor> mhsa_stream_fwd(at::Tensor q, at::Tensor k,
                                        at::Tensor v, at::Tensor rel_w,
                                        at::Tensor rel_h, int64_t L, int64_t H,
                                        int64_t W, int64_t heads, int64_t qpix,
                                        int64_t kpix, int64_t vpix,
                                        double scale, bool need_lse) {
  const char* fn = "mhsa_stream_fwd";
  TORCH_CHECK(L >= 1 && qpix >= 1 && q.numel() % (L * qpix) == 0 &&
                  q.numel() > 0,
              fn, ": q holds no whole number of images of L = ", L,
              " pixels with stride ", qpix);
  const int64_t N = q.numel() / (L * qpix);
  const int64_t B = N * std::max<int64_t>(heads, 1);
  const int D = check_geometry(fn, rel_w, rel_h, L, H, W, B, heads);
  check_span(q, N * L, qpix, heads * D, fn, "q");
  check_span(k, N * L, kpix, heads * D, fn, "k");
  check_span(v, N * L, vpix, heads * D, fn, "v");
  at::Tensor o;
  int64_t opix;
  if (heads > 1) {
    o = at::empty({N, heads * D, H, W},
                  q.options().memory_format(at::MemoryFormat::ChannelsLast));
    opix = heads * D;
  } else {
    o = at::empty({B, L, (int64_t)D}, q.options());
    opix = D;
  }
  auto lse = at::empty({need_lse ? B : 0, need_lse ? L : 0},
                       q.options().dtype(at::kFloat));
  StreamParams p = {};
  p.q = (const __hip_bfloat16*)q.data_ptr();
  p.k = (const __hip_bfloat16*)k.data_ptr();
  p.v = (const __hip_bfloat16*)v.data_ptr();
  p.relw = (const __hip_bfloat16*)rel_w.data_ptr();
  p.relh = (const __hip_bfloat16*)rel_h.data_ptr();
  p.out = (__hip_bfloat16*)o.data_ptr();
  p.lse = need_lse ? lse.data_ptr<float>() : nullptr;
  p.B = (int)B; p.L = (int)L; p.H = (int)H; p.W = (int)W;
  p.MW = 2 * (int)W - 1; p.MH = 2 * (int)H - 1;
  p.heads = (int)heads;
  p.qpix = qpix; p.kpix = kpix; p.vpix = vpix; p.opix = opix;
  p.scale = (float)scale;
  dim3 grid((unsigned)B, (unsigned)((L + TQ - 1) / TQ));
  STREAM_ND_SWITCH(
      D, launch_stream<mhsa_stream_fwd_kernel<ND>, fwd_lds<ND>()>(grid, p));
  return {o, lse};
}

// dO, o: rows of stride opix; dq goes to dqk_out, dk to dqk_out + kqoff
// elements (stride qpix both), dv to dv_out (stride vpix), as mhsa_bwd. B and
// L come from lse [B, L]. Returns {dqk_out, dv_out, grw, grh}, grw / grh fp32.
std::vector<at::Tensor> mhsa_stream_bwd(
    at::Tensor dO, at::Tensor o, at::Tensor lse, at::Tensor q, at::Tensor k,
    at::Tensor v, at::Tensor rel_w, at::Tensor rel_h, int64_t H, int64_t W,
    int64_t heads, int64_t qpix, int64_t kqoff, int64_t vpix, int64_t opix,
    double scale, at::Tensor dqk_out, at::Tensor dv_out) {
  const char* fn = "mhsa_stream_bwd";
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
                  lse.dim() == 2 && lse.is_contiguous(),
              fn, ": lse must be contiguous fp32 [B, L]");
  const int64_t B = lse.size(0), L = lse.size(1);
  const int D = check_geometry(fn, rel_w, rel_h, L, H, W, B, heads);
  const int64_t N = B / heads;
  check_span(q, N * L, qpix, heads * D, fn, "q");
  check_span(k, N * L, qpix, heads * D, fn, "k");
  check_span(v, N * L, vpix, heads * D, fn, "v");
  check_span(dO, N * L, opix, heads * D, fn, "dO");
  check_span(o, N * L, opix, heads * D, fn, "o");
  check_span(dv_out, N * L, vpix, heads * D, fn, "dv_out");
  check_span(dqk_out, N * L, qpix, heads * D, fn, "dqk_out");
  TORCH_CHECK(kqoff >= 0 && kqoff % 8 == 0 &&
                  (int64_t)(dqk_out.storage().nbytes() / 2) >=
                      dqk_out.storage_offset() + kqoff + (N * L - 1) * qpix +
                          heads * D,
              fn, ": dqk_out has no room for dk at offset ", kqoff);
  const int MW = 2 * (int)W - 1, MH = 2 * (int)H - 1;
  auto fopts = lse.options();
  auto delta = at::empty({B, L}, fopts);
  auto drw = at::empty({B * L, (int64_t)MW}, fopts);
  auto drh = at::empty({B * L, (int64_t)MH}, fopts);
  auto grw = at::empty({(int64_t)MW, (int64_t)D}, fopts);
  auto grh = at::empty({(int64_t)MH, (int64_t)D}, fopts);
  StreamParams p = {};
  p.q = (const __hip_bfloat16*)q.data_ptr();
  p.k = (const __hip_bfloat16*)k.data_ptr();
  p.v = (const __hip_bfloat16*)v.data_ptr();
  p.o = (const __hip_bfloat16*)o.data_ptr();
  p.dO = (const __hip_bfloat16*)dO.data_ptr();
  p.relw = (const __hip_bfloat16*)rel_w.data_ptr();
  p.relh = (const __hip_bfloat16*)rel_h.data_ptr();
  p.lse = lse.data_ptr<float>();
  p.delta = delta.data_ptr<float>();
  p.dq = (__hip_bfloat16*)dqk_out.data_ptr();
  p.dk = p.dq + kqoff;
  p.dv = (__hip_bfloat16*)dv_out.data_ptr();
  p.drw = drw.data_ptr<float>();
  p.drh = drh.data_ptr<float>();
  p.B = (int)B; p.L = (int)L; p.H = (int)H; p.W = (int)W;
  p.MW = MW; p.MH = MH;
  p.heads = (int)heads;
  p.qpix = qpix; p.kpix = qpix; p.vpix = vpix; p.opix = opix;
  p.scale = (float)scale;
  dim3 grid((unsigned)B, (unsigned)((L + TQ - 1) / TQ));
  STREAM_ND_SWITCH(
      D, launch_stream<mhsa_stream_bwd_q_kernel<ND>, bwd_q_lds<ND>()>(grid, p));
  STREAM_ND_SWITCH(
      D,
      launch_stream<mhsa_stream_bwd_kv_kernel<ND>, bwd_kv_lds<ND>()>(grid, p));

  const int64_t rows = B * L;
  const int rpb = 128;
  const int rblocks = (int)ceil_div(rows, rpb);
  const bool det = is_deterministic();  // sampled per launch
  at::Tensor part;  // deterministic mode: [rblocks][M * D], fully written
  if (det) {
    part = at::empty({(int64_t)rblocks, (int64_t)std::max(MW, MH) * D}, fopts);
  } else {
    const int na = MW * D, nc = MH * D;
    hipLaunchKernelGGL(mhsa_stream_zero_kernel,
                       dim3((std::max(na, nc) + 255) / 256), dim3(256), 0,
                       cur_stream(), grw.data_ptr<float>(), na,
                       grh.data_ptr<float>(), nc);
  }
  for (int which = 0; which < 2; ++which) {
    StreamRelGradParams rp;
    rp.dr = which == 0 ? drw.data_ptr<float>() : drh.data_ptr<float>();
    rp.q = p.q;
    rp.out = which == 0 ? grw.data_ptr<float>() : grh.data_ptr<float>();
    rp.M = which == 0 ? MW : MH;
    rp.pstride = (int64_t)rp.M * D;
    rp.rows = rows;
    rp.D = D;
    rp.rows_per_block = rpb;
    rp.heads = (int)heads;
    rp.L = (int)L;
    rp.qpix = qpix;
    rp.scale = (float)scale;
    if (det) {  // stream-ordered, so the two tables share one workspace
      float* out = rp.out;
      rp.out = part.data_ptr<float>();
      hipLaunchKernelGGL(mhsa_stream_rel_grad_kernel<true>, dim3(rblocks),
                         dim3(256), 0, cur_stream(), rp);
      ordered_reduce<float>(part.data_ptr<float>(), out, rblocks, rp.pstride,
                            1.f);
    } else {
      hipLaunchKernelGGL(mhsa_stream_rel_grad_kernel<false>, dim3(rblocks),
                         dim3(256), 0, cur_stream(), rp);
    }
  }
  return {dqk_out, dv_out, grw, grh};
}
