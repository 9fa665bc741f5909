// Exact-fp32 BoTNet MHSA for feature maps up to 32x32 (1 <= H, W <= 32,
// L = H*W <= 1024, D in 32 / 64 / 96 / 128): one streaming kernel family with
// an online softmax, forward and recompute backward, every MFMA operand fp32
// (v_mfma_f32_16x16x4_f32). Neither P nor dS is ever rounded below fp32 and
// neither reaches LDS or global memory.
//
// Math (tests/mhsa_ref.py): pixel x = hx * W + wx,
//   S[x, y] = scale q[x].k[y] + RW[x][wy-wx+W-1] + RH[x][hy-hx+H-1]
//   RW = scale q rel_w^T, RH = scale q rel_h^T, P = softmax(S), O = P v
//   dV = P^T dO, dP = dO v^T, dS = P (dP - delta), delta[x] = dO[x].O[x]
//   dQ = scale (dS k + dRW rel_w + dRH rel_h), dK = scale dS^T q
//   dRW[x, m] = sum_{y: wy-wx+W-1 == m} dS[x, y], grw = scale dRW^T q
//
// MFMA operand maps (conv_fp32.hip), lane = 16 g + c, one value per lane:
//   A: A[c][g]      B: B[g][c]      D: register i holds D[4 g + i][c]
//
// Register-resident P. A D tile is already an A fragment of the next GEMM when
// the reduction index is permuted. The forward and bwd_q compute the score
// tile transposed, S^T = K Q^T (K tile rows as A, the wave's own 16 q rows as
// B), so register i of lane (g, c) of key sub-tile nt is S[q c][key 16 nt +
// 4 g + i]: every lane holds 16 keys of ONE q row. After the softmax that
// register is the A value P[q c][k-slot g] of a k-step whose four slots are
// the keys {16 nt + 4 g' + i : g' = 0..3}; the matching B value is
// V[16 nt + 4 g + i][n0 + c], a plain ds_read_b32. The order in which keys are
// summed is free, so P (and dS for dQ += dS K, and for the gather-sums) never
// passes through an LDS slab. bwd_kv computes S = Q K^T untransposed for the
// same reason: its lanes hold 16 q rows of one key, the A values of
// dV += P^T dO and dK += dS^T Q. The same freedom serves the first GEMM: the
// lane of slot g takes d = 16 jj + 4 g + e for e = 0..3 as four k-steps, so
// its A values are one ds_read_b128 and its B values one global float4.
//
// A row's softmax statistics are 16 registers per key tile per lane and a
// reduction over the four lane groups l, l + 16, l + 32, l + 48. The output
// fragments are indexed the other way round (register i = row 4 g + i), so
// the rescale factor and 1 / l of row 4 g + i are fetched from lane 4 g + i.
//
// Every kernel: 256 threads, wave w owns rows 16 w .. + 16 of a 64-row block
// tile and streams 64-row tiles of the other side: global -> registers (the
// next tile's loads are issued right after the barrier and land under the
// current tile's MFMAs) -> LDS rows of RS = D + 4 floats.
// Bank argument (64 banks of 4 bytes; RS = 4 mod 16, so RS = 4 mod 64 or
// 36 mod 64 and 4 RS = 16 mod 64):
//   row-operand read, ds_read_b128 at (16 nt + c) RS + 16 jj + 4 g: the 16
//     lanes of one g start at banks 4 c RS/4.. = {4 c (mod 64)} or
//     {36 c (mod 64)}, 16 distinct multiples of 4, four banks each: all 64
//     banks once per 16-lane group.
//   column-operand read, ds_read_b32 at (16 nt + 4 g + i) RS + n0 + c: lane
//     group g is offset by 4 g RS = 16 g (mod 64), c adds 0..15: the 64 lanes
//     hit 64 distinct banks.
//   fp32 tables [64][TS = 65]: row stride odd, so the 16 rows a wave reads at
//     once fall on distinct banks for equal columns.
// No transposed-read instruction is involved.
//
//   mhsa_f32_fwd_kernel     block (b, q tile). Prologue: the wave's 16 rows of
//     RW / RH by MFMA (rel_w / rel_h rows from global as A, the q registers as
//     B), kept fp32 in LDS. Per key tile: S^T, rel add, key tail = -inf,
//     running max and per-lane partial sum, O rescaled, O += P~ V.
//     Epilogue: O / l, lse = m + log l.
//   mhsa_f32_bwd_q_kernel   block (b, q tile). delta (also to global), tables
//     rebuilt. Per key tile: P = exp(S - lse), dP^T = V dO^T, dS in registers,
//     dQ += dS K, and the gather-sums sum_{y: wy == n} dS[x, y] as dS times a
//     0 / 1 indicator built in registers (no LDS atomics). Epilogue: the
//     shifted sums go into the wave's rows of the tables, which then are the A
//     operand of dQ += dRW rel_w + dRH rel_h; dRW / dRH to global [B * L, M].
//   mhsa_f32_bwd_kv_kernel  block (b, key tile), streams q tiles: tables of
//     the q tile rebuilt, S and dP untransposed, dV += P^T dO, dK += dS^T Q.
//     A block owns its rows for the whole loop: no atomics.
//   mhsa_f32_rel_grad_kernel  grw / grh: fp32 atomics, or workspace slots and
//     ordered_reduce in deterministic mode.
//
// LDS (bytes) at D = 128: two tiles 2 * 64 * 132 * 4 = 67584, two tables
// 2 * 64 * 65 * 4 = 33280; fwd and bwd_q 100864, bwd_kv 101376 (+ lse and
// delta of the q tile): one block per CU. docs/ARCHITECTURE.md, "fp32
// attention", has the register table.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4a;

namespace {

constexpr int TQ = 64;  // rows of a block tile and of a streamed tile
constexpr int TS = 65;  // table row stride: M <= 63, odd against the banks

struct F32Params {
  const float* q;
  const float* k;
  const float* v;
  const float* o;     // backward: the forward's output
  const float* dO;
  const float* relw;  // [2W-1, D]
  const float* relh;  // [2H-1, D]
  float* out;         // forward
  float* lse;         // [B, L]: written by fwd (may be null), read by bwd
  float* delta;       // [B, L]: written by bwd_q, read by bwd_kv
  float* dq;
  float* dk;
  float* dv;
  float* drw;         // [B * L, 2W-1]
  float* drh;         // [B * L, 2H-1]
  int B, L, H, W, MW, MH, heads;
  int64_t qpix, kpix, vpix, opix;  // elements per pixel (attention.hip)
  float scale, invW;
};

DEV_INLINE int64_t frow(int b, int l, int L, int heads, int64_t pix, int D) {
  const int n = b / heads, hd = b - n * heads;
  return ((int64_t)n * L + l) * pix + (int64_t)hd * D;
}

// y = h * W + w for 0 <= y < 1024, 1 <= W <= 32. (y + 0.5) / W is at least
// 1 / 64 away from an integer and the fp32 product is within 2^-12 of it.
DEV_INLINE void hw_of(int y, int W, float invW, int& h, int& w) {
  h = (int)(((float)y + 0.5f) * invW);
  w = y - h * W;
}

DEV_INLINE f32x4a zero4() { return f32x4a{0.f, 0.f, 0.f, 0.f}; }

DEV_INLINE f32x4a mfma4(float a, float b, f32x4a c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows row0 .. + 64 of a strided-row tensor -> 2 ND float4 per thread
template <int ND>
DEV_INLINE void tile_load(f32x4a (&r)[2 * ND], const float* base, int b,
                          int row0, int L, int heads, int64_t pix, int tid) {
#pragma unroll
  for (int i = 0; i < 2 * ND; ++i) {
    const int ch = tid + i * 256;
    const int row = ch / (8 * ND), c4 = (ch % (8 * ND)) * 4;
    const int l = row0 + row;
    r[i] = l < L ? *reinterpret_cast<const f32x4a*>(
                       base + frow(b, l, L, heads, pix, 32 * ND) + c4)
                 : zero4();  // tail rows are zeros
  }
}

template <int ND>
DEV_INLINE void tile_store(float* lds, const f32x4a (&r)[2 * ND], int tid) {
#pragma unroll
  for (int i = 0; i < 2 * ND; ++i) {
    const int ch = tid + i * 256;
    const int row = ch / (8 * ND), c4 = (ch % (8 * ND)) * 4;
    *reinterpret_cast<f32x4a*>(lds + row * (32 * ND + 4) + c4) = r[i];
  }
}

// The lane's share of one row as the register operand of the first GEMM:
// f[jj][e] = row[16 jj + 4 g + e] (zeros when !ok)
template <int ND>
DEV_INLINE void row_frags(f32x4a (&f)[2 * ND], const float* rp, bool ok,
                          int g) {
#pragma unroll
  for (int jj = 0; jj < 2 * ND; ++jj)
    f[jj] = ok ? *reinterpret_cast<const f32x4a*>(rp + 16 * jj + 4 * g)
               : zero4();
}

// acc[nt][i] = tile row (16 nt + 4 g + i) . register row c, reduction over D
template <int ND>
DEV_INLINE void nt_tile(f32x4a (&acc)[4], const f32x4a (&b)[2 * ND],
                        const float* tile, int c, int g) {
  constexpr int RS = 32 * ND + 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = zero4();
#pragma unroll
  for (int jj = 0; jj < 2 * ND; ++jj) {
    f32x4a a[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      a[nt] = *reinterpret_cast<const f32x4a*>(tile + (nt * 16 + c) * RS +
                                               16 * jj + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[nt] = mfma4(a[nt][e], b[jj][e], acc[nt]);
  }
}

// tab[row0 + c][m] = scale * (register row c) . rel[m], 0 <= m < 16 ceil(M/16)
// (columns M .. are zeros; m <= 63 < TS)
template <int ND>
DEV_INLINE void build_table(float* tab, int row0, const f32x4a (&b)[2 * ND],
                            const float* rel, int M, float scale, int c,
                            int g) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    if (mt * 16 >= M) break;  // wave-uniform
    const int m = mt * 16 + c;
    f32x4a s = zero4();
#pragma unroll
    for (int jj = 0; jj < 2 * ND; ++jj) {
      const f32x4a a =
          m < M ? *reinterpret_cast<const f32x4a*>(rel + m * (32 * ND) +
                                                   16 * jj + 4 * g)
                : zero4();
#pragma unroll
      for (int e = 0; e < 4; ++e) s = mfma4(a[e], b[jj][e], s);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      tab[(row0 + c) * TS + mt * 16 + g * 4 + i] = s[i] * scale;
  }
}

// acc[dt][i] (row 4 g + i, column 16 dt + c) += sum over the tile's 64 rows r
// of a[r][row] * tile[r][column]; this lane's a[nt][i] belongs to tile row
// 16 nt + 4 g + i and to output row c.
template <int ND>
DEV_INLINE void ts_accum(f32x4a (&acc)[2 * ND], const f32x4a (&a)[4],
                         const float* tile, int c, int g) {
  constexpr int RS = 32 * ND + 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* tp = tile + (nt * 16 + g * 4 + i) * RS + c;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt)
        acc[dt] = mfma4(a[nt][i], tp[dt * 16], acc[dt]);
    }
  }
}

template <int ND>
constexpr int tile_floats() { return TQ * (32 * ND + 4); }
template <int ND>
constexpr int fwd_lds() { return (2 * tile_floats<ND>() + 2 * TQ * TS) * 4; }
template <int ND>
constexpr int bwd_kv_lds() { return fwd_lds<ND>() + 2 * TQ * 4; }

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_f32_fwd_kernel(F32Params p) {
  constexpr int D = 32 * ND;
  extern __shared__ __align__(16) char smem[];
  float* Ks = reinterpret_cast<float*>(smem);
  float* Vs = Ks + tile_floats<ND>();
  float* RW = Vs + tile_floats<ND>();
  float* RH = RW + TQ * TS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const int qrow_base = blockIdx.y * TQ + wid * 16;

  // this lane's q row for the scores: qrow_base + c
  const bool qok = qrow_base + c < p.L;
  const int qc = min(qrow_base + c, p.L - 1);  // pad rows: any valid row
  f32x4a qf[2 * ND];
  row_frags<ND>(qf, p.q + frow(b, qc, p.L, p.heads, p.qpix, D), qok, g);
  build_table<ND>(RW, wid * 16, qf, p.relw, p.MW, p.scale, c, g);
  build_table<ND>(RH, wid * 16, qf, p.relh, p.MH, p.scale, c, g);
  int hx, wx;
  hw_of(qc, p.W, p.invW, hx, wx);
  // table row pre-offset so that [wy] / [hy] index it
  const float* rwrow = RW + (wid * 16 + c) * TS + (p.W - 1 - wx);
  const float* rhrow = RH + (wid * 16 + c) * TS + (p.H - 1 - hx);

  float mrow = -INFINITY, lrow = 0.f;
  f32x4a oacc[2 * ND];
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) oacc[dt] = zero4();

  const int nkt = (p.L + TQ - 1) / TQ;
  f32x4a rk[2 * ND], rv[2 * ND];
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
    {
    f32x4a s[4];  // s[nt][i] = S[q c][key 64 kt + 16 nt + 4 g + i]
    nt_tile<ND>(s, qf, Ks, c, g);
    // rel add; keys past L get -inf (every tile holds at least one key < L,
    // so the running max is finite from the first tile on)
    float tmax = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int y = kt * TQ + nt * 16 + g * 4 + i;
        const bool kok = y < p.L;
        int hy, wy;
        hw_of(kok ? y : p.L - 1, p.W, p.invW, hy, wy);
        const float sv =
            kok ? s[nt][i] * p.scale + rwrow[wy] + rhrow[hy] : -INFINITY;
        s[nt][i] = sv;
        tmax = fmaxf(tmax, sv);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mnew = fmaxf(mrow, tmax);
    const float alpha = expf(mrow - mnew);  // first tile: exp(-inf) = 0
    mrow = mnew;
    float rsum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float e = expf(s[nt][i] - mnew);
        rsum += e;
        s[nt][i] = e;
      }
    lrow = lrow * alpha + rsum;  // per-lane partial of the row sum
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ai = __shfl(alpha, g * 4 + i);  // output row 4 g + i
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt) oacc[dt][i] *= ai;
    }
    ts_accum<ND>(oacc, s, Vs, c, g);
    }
    __syncthreads();
  }

  lrow += __shfl_xor(lrow, 16);
  lrow += __shfl_xor(lrow, 32);
  const float inv = 1.f / lrow;
  if (p.lse != nullptr && g == 0 && qok)
    p.lse[(int64_t)b * p.L + qrow_base + c] = mrow + logf(lrow);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float invi = __shfl(inv, g * 4 + i);
    const int qr = qrow_base + g * 4 + i;
    if (qr < p.L) {
      float* op = p.out + frow(b, qr, p.L, p.heads, p.opix, D) + c;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt) op[dt * 16] = oacc[dt][i] * invi;
    }
  }
}

// ---------------------------------------------------------------------------
// backward, q side
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_f32_bwd_q_kernel(F32Params p) {
  constexpr int D = 32 * ND;
  extern __shared__ __align__(16) char smem[];
  float* Ks = reinterpret_cast<float*>(smem);
  float* Vs = Ks + tile_floats<ND>();
  float* RW = Vs + tile_floats<ND>();
  float* RH = RW + TQ * TS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const int qrow_base = blockIdx.y * TQ + wid * 16;

  const bool qok = qrow_base + c < p.L;
  const int qc = min(qrow_base + c, p.L - 1);
  f32x4a qf[2 * ND], dof[2 * ND];
  float dlt;
  {
    row_frags<ND>(qf, p.q + frow(b, qc, p.L, p.heads, p.qpix, D), qok, g);
    const int64_t orow = frow(b, qc, p.L, p.heads, p.opix, D);
    row_frags<ND>(dof, p.dO + orow, qok, g);
    f32x4a of[2 * ND];
    row_frags<ND>(of, p.o + orow, qok, g);
    // delta[q c] = dO . O: 8 ND products per lane, then over the 4 groups
    float d = 0.f;
#pragma unroll
    for (int jj = 0; jj < 2 * ND; ++jj)
#pragma unroll
      for (int e = 0; e < 4; ++e) d += dof[jj][e] * of[jj][e];
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    dlt = d;
    if (g == 0 && qok) p.delta[(int64_t)b * p.L + qc] = d;
  }
  build_table<ND>(RW, wid * 16, qf, p.relw, p.MW, p.scale, c, g);
  build_table<ND>(RH, wid * 16, qf, p.relh, p.MH, p.scale, c, g);
  __builtin_amdgcn_wave_barrier();

  // pad q rows (>= L) have q = dO = 0: P = exp(0 - 0), dP = delta = 0, dS = 0
  int hx, wx;
  hw_of(qc, p.W, p.invW, hx, wx);
  const float* rwrow = RW + (wid * 16 + c) * TS + (p.W - 1 - wx);
  const float* rhrow = RH + (wid * 16 + c) * TS + (p.H - 1 - hx);
  const float lse = qok ? p.lse[(int64_t)b * p.L + qc] : 0.f;

  f32x4a dqacc[2 * ND];
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) dqacc[dt] = zero4();
  // ew[j][x][n] = sum_{y: wy == 16 j + n} dS[x, y] (eh: hy), by MFMA against
  // 0 / 1 indicators of this lane's own keys; dRW[x][m] is ew shifted by the
  // row's own wx
  f32x4a ew[2], eh[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) ew[j] = eh[j] = zero4();

  const int nkt = (p.L + TQ - 1) / TQ;
  f32x4a rk[2 * ND], rv[2 * ND];
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
    {
    f32x4a s[4], dp[4];  // [q c][key 64 kt + 16 nt + 4 g + i]
    nt_tile<ND>(s, qf, Ks, c, g);
    nt_tile<ND>(dp, dof, Vs, c, g);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int y = kt * TQ + nt * 16 + g * 4 + i;
        const bool kok = y < p.L;
        int hy, wy;
        hw_of(kok ? y : p.L - 1, p.W, p.invW, hy, wy);
        const float pv =
            kok ? expf(s[nt][i] * p.scale + rwrow[wy] + rhrow[hy] - lse) : 0.f;
        const float ds = pv * (dp[nt][i] - dlt);  // keys past L: dS = 0
        s[nt][i] = ds;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j * 16 < p.W)
            ew[j] = mfma4(ds, wy == j * 16 + c ? 1.f : 0.f, ew[j]);
          if (j * 16 < p.H)
            eh[j] = mfma4(ds, hy == j * 16 + c ? 1.f : 0.f, eh[j]);
        }
      }
    }
    ts_accum<ND>(dqacc, s, Ks, c, g);
    }
    __syncthreads();
  }

  // dRW / dRH into this wave's rows of the (now free) RW / RH tables; the
  // fragments hold rows 4 g + i
  float* dRW = RW + wid * 16 * TS;
  float* dRH = RH + wid * 16 * TS;
  for (int i = lane; i < 16 * TS; i += 64) {
    dRW[i] = 0.f;
    dRH[i] = 0.f;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int hxi, wxi;
    hw_of(min(qrow_base + g * 4 + i, p.L - 1), p.W, p.invW, hxi, wxi);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = j * 16 + c;
      if (n < p.W) dRW[(g * 4 + i) * TS + n - wxi + p.W - 1] = ew[j][i];
      if (n < p.H) dRH[(g * 4 + i) * TS + n - hxi + p.H - 1] = eh[j][i];
    }
  }
  __builtin_amdgcn_wave_barrier();
  // dQ += dRW rel_w + dRH rel_h: table rows as A (columns M .. 63 are zeros),
  // rel rows from global as B
  for (int m0 = 0; m0 < p.MW; m0 += 4) {
    const int m = m0 + g;  // <= 63 < TS
    const float a = dRW[c * TS + m];
    const float* rp = p.relw + (int64_t)min(m, p.MW - 1) * D + c;
#pragma unroll
    for (int dt = 0; dt < 2 * ND; ++dt)
      dqacc[dt] = mfma4(a, m < p.MW ? rp[dt * 16] : 0.f, dqacc[dt]);
  }
  for (int m0 = 0; m0 < p.MH; m0 += 4) {
    const int m = m0 + g;
    const float a = dRH[c * TS + m];
    const float* rp = p.relh + (int64_t)min(m, p.MH - 1) * D + c;
#pragma unroll
    for (int dt = 0; dt < 2 * ND; ++dt)
      dqacc[dt] = mfma4(a, m < p.MH ? rp[dt * 16] : 0.f, dqacc[dt]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qr = qrow_base + g * 4 + i;
    if (qr < p.L) {
      float* dqp = p.dq + frow(b, qr, p.L, p.heads, p.qpix, D) + c;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt)
        dqp[dt * 16] = dqacc[dt][i] * p.scale;
    }
  }
  for (int r = 0; r < 16; ++r) {
    const int qr = qrow_base + r;
    if (qr >= p.L) break;
    const int64_t grow = (int64_t)b * p.L + qr;
    if (lane < p.MW) p.drw[grow * p.MW + lane] = dRW[r * TS + lane];
    if (lane < p.MH) p.drh[grow * p.MH + lane] = dRH[r * TS + lane];
  }
}

// ---------------------------------------------------------------------------
// backward, k / v side
// ---------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(256) void mhsa_f32_bwd_kv_kernel(F32Params p) {
  constexpr int D = 32 * ND, RS = D + 4;
  extern __shared__ __align__(16) char smem[];
  float* Qs = reinterpret_cast<float*>(smem);
  float* dOs = Qs + tile_floats<ND>();
  float* RW = dOs + tile_floats<ND>();
  float* RH = RW + TQ * TS;
  float* lse_s = RH + TQ * TS;
  float* dl_s = lse_s + TQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const int krow_base = blockIdx.y * TQ + wid * 16;

  // this lane's key for the scores: krow_base + c. Pad key rows (>= L) have
  // k = v = 0: finite values in rows that are never stored
  const bool kok = krow_base + c < p.L;
  const int yc = min(krow_base + c, p.L - 1);
  f32x4a kf[2 * ND], vf[2 * ND];
  row_frags<ND>(kf, p.k + frow(b, yc, p.L, p.heads, p.kpix, D), kok, g);
  row_frags<ND>(vf, p.v + frow(b, yc, p.L, p.heads, p.vpix, D), kok, g);
  int hy, wy;
  hw_of(yc, p.W, p.invW, hy, wy);
  f32x4a dkacc[2 * ND], dvacc[2 * ND];
#pragma unroll
  for (int dt = 0; dt < 2 * ND; ++dt) dkacc[dt] = dvacc[dt] = zero4();

  const int nqt = (p.L + TQ - 1) / TQ;
  f32x4a rq[2 * ND], rdo[2 * ND];
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
      f32x4a qf[2 * ND];
      row_frags<ND>(qf, Qs + (wid * 16 + c) * RS, true, g);
      build_table<ND>(RW, wid * 16, qf, p.relw, p.MW, p.scale, c, g);
      build_table<ND>(RH, wid * 16, qf, p.relh, p.MH, p.scale, c, g);
    }
    __syncthreads();
    {
    f32x4a s[4], dp[4];  // [q 64 qt + 16 nt + 4 g + i][key c]
    nt_tile<ND>(s, kf, Qs, c, g);
    nt_tile<ND>(dp, vf, dOs, c, g);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int xl = nt * 16 + g * 4 + i;
        const int x = qt * TQ + xl;
        const bool xok = x < p.L;
        int hx, wx;
        hw_of(xok ? x : p.L - 1, p.W, p.invW, hx, wx);
        const float rel = RW[xl * TS + wy - wx + p.W - 1] +
                          RH[xl * TS + hy - hx + p.H - 1];
        const float pv =
            xok ? expf(s[nt][i] * p.scale + rel - lse_s[xl]) : 0.f;
        s[nt][i] = pv;
        dp[nt][i] = pv * (dp[nt][i] - dl_s[xl]);
      }
    }
    ts_accum<ND>(dvacc, s, dOs, c, g);
    ts_accum<ND>(dkacc, dp, Qs, c, g);
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = krow_base + g * 4 + i;
    if (y < p.L) {
      float* dkp = p.dk + frow(b, y, p.L, p.heads, p.kpix, D) + c;
      float* dvp = p.dv + frow(b, y, p.L, p.heads, p.vpix, D) + c;
#pragma unroll
      for (int dt = 0; dt < 2 * ND; ++dt) {
        dkp[dt * 16] = dkacc[dt][i] * p.scale;
        dvp[dt * 16] = dvacc[dt][i];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// grw[m, d] = scale * sum_rows dRW[row, m] q[row, d], M <= 63
// ---------------------------------------------------------------------------
struct F32RelGradParams {
  const float* dr;   // [rows, M]
  const float* q;    // strided rows
  float* out;        // [M, D] zeroed, or part[row blocks][M * D]
  int64_t pstride;   // workspace slot stride (deterministic mode)
  int64_t rows;
  int M, D, heads, L;
  int64_t qpix;
  float scale;
};

constexpr int RG_ROWS = 128;  // rows per block

// thread (half, d) holds its half of the m range (<= 32 columns) for one d.
// The block's dr rows are staged in LDS once (coalesced; every lane then reads
// the same word, a broadcast), and the q[r, d] loads, coalesced over d, are
// issued eight rows at a time so that their latencies overlap.
template <bool DET>
__global__ __launch_bounds__(256) void mhsa_f32_rel_grad_kernel(
    F32RelGradParams p) {
  __shared__ float drs[RG_ROWS * 63];
  const int d = threadIdx.x & 127, half = threadIdx.x >> 7;
  const int mh = (p.M + 1) / 2;
  const int m0 = half * mh;
  const int mn = min(p.M - m0, mh);
  const int64_t r0 = (int64_t)blockIdx.x * RG_ROWS;
  const int nr = (int)min((int64_t)RG_ROWS, p.rows - r0);
  for (int i = threadIdx.x; i < nr * p.M; i += 256)
    drs[i] = p.dr[r0 * p.M + i];
  __syncthreads();
  if (d >= p.D) return;
  float acc[32] = {};
  int bb = (int)(r0 / p.L), ll = (int)(r0 - (int64_t)bb * p.L);
  for (int r = 0; r < nr; r += 8) {
    float qv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // rows past nr: 0 times a staged row
      qv[u] = r + u < nr
                  ? p.q[frow(bb, ll, p.L, p.heads, p.qpix, p.D) + d]
                  : 0.f;
      if (++ll == p.L) {
        ll = 0;
        ++bb;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* dr = drs + min(r + u, nr - 1) * p.M + m0;
#pragma unroll
      for (int m = 0; m < 32; ++m)
        if (m < mn) acc[m] += dr[m] * qv[u];
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
__global__ void mhsa_f32_zero_kernel(float* a, int na, float* c, int nc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) a[i] = 0.f;
  if (i < nc) c[i] = 0.f;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <auto KERN, int LDS>
void launch_f32(dim3 grid, const F32Params& p) {
  // above 64 KB the dynamic-LDS limit must be raised, once per device
  static bool attr_done[64] = {};
  if (LDS > 65536) {
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64,
                "mhsa_f32: no current device");
    if (!attr_done[dev]) {
      const hipError_t err = hipFuncSetAttribute(
          (const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
      TORCH_CHECK(err == hipSuccess, "mhsa_f32: cannot raise dynamic LDS to ",
                  LDS, " bytes: ", hipGetErrorString(err));
      attr_done[dev] = true;
    }
  }
  hipLaunchKernelGGL(KERN, grid, dim3(256), LDS, cur_stream(), p);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "mhsa_f32: launch failed: ",
              hipGetErrorString(err));
}

// the last element a kernel touches through `t` lies inside its storage
void check_span_f32(const at::Tensor& t, int64_t pixels, int64_t pix,
                    int64_t width, const char* fn, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat, fn, ": ", name,
              " must be an fp32 GPU tensor");
  TORCH_CHECK(pix >= width && pix % 4 == 0, fn, ": ", name,
              " pixel stride must be a multiple of 4 and >= heads*D, got ", pix);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, ": ",
              name, " must be 16-byte aligned");
  const int64_t need = t.storage_offset() + (pixels - 1) * pix + width;
  TORCH_CHECK((int64_t)(t.storage().nbytes() / 4) >= need, fn, ": ", name,
              " holds fewer than ", pixels, " pixels of stride ", pix);
}

// shared geometry checks; returns D
int check_geometry_f32(const char* fn, const at::Tensor& rel_w,
                       const at::Tensor& rel_h, int64_t L, int64_t H, int64_t W,
                       int64_t B, int64_t heads) {
  TORCH_CHECK(rel_w.is_cuda() && rel_h.is_cuda() &&
                  rel_w.scalar_type() == at::kFloat &&
                  rel_h.scalar_type() == at::kFloat && rel_w.dim() == 2 &&
                  rel_h.dim() == 2 && rel_w.is_contiguous() &&
                  rel_h.is_contiguous(),
              fn, ": rel_w / rel_h must be contiguous 2-D fp32 GPU tensors");
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
  TORCH_CHECK(rel_w.size(0) == 2 * W - 1, fn, ": rel_w must be [2W-1, D]");
  TORCH_CHECK(rel_h.size(0) == 2 * H - 1 && rel_h.size(1) == D, fn,
              ": rel_h must be [2H-1, D]");
  TORCH_CHECK(heads >= 1 && B >= 1 && B % heads == 0, fn, ": B = ", B,
              " is not a positive multiple of heads = ", heads);
  return (int)D;
}

#define F32_ND_SWITCH(D, ...)                          \
  switch ((D) / 32) {                                  \
    case 1: { constexpr int ND = 1; __VA_ARGS__; break; } \
    case 2: { constexpr int ND = 2; __VA_ARGS__; break; } \
    case 3: { constexpr int ND = 3; __VA_ARGS__; break; } \
    default: { constexpr int ND = 4; __VA_ARGS__; break; } \
  }

}  // namespace

// q, k, v: fp32, rows addressed as base + ((n*L + l) * pix + hd * D) with
// b = n * heads + hd (attention.hip): heads = 1, pix = D is the dense
// [B, L, D] layout; heads > 1 reads the qkv convs' channels_last outputs in
// place (k is a view whose data pointer is the k half) and returns o as
// channels_last [N, heads*D, H, W]. N = q.numel() / (L * qpix). Returns
// {o, lse}; lse is fp32 [B, L], or empty when need_lse is false.
std::vector<at::Tensor> mhsa_f32_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                     at::Tensor rel_w, at::Tensor rel_h,
                                     int64_t L, int64_t H, int64_t W,
                                     int64_t heads, int64_t qpix, int64_t kpix,
                                     int64_t vpix, double scale,
                                     bool need_lse) {
  const char* fn = "mhsa_f32_fwd";
  TORCH_CHECK(L >= 1 && qpix >= 1 && q.numel() % (L * qpix) == 0 &&
                  q.numel() > 0,
              fn, ": q holds no whole number of images of L = ", L,
              " pixels with stride ", qpix);
  const int64_t N = q.numel() / (L * qpix);
  const int64_t B = N * std::max<int64_t>(heads, 1);
  const int D = check_geometry_f32(fn, rel_w, rel_h, L, H, W, B, heads);
  check_span_f32(q, N * L, qpix, heads * D, fn, "q");
  check_span_f32(k, N * L, kpix, heads * D, fn, "k");
  check_span_f32(v, N * L, vpix, heads * D, fn, "v");
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
  auto lse = at::empty({need_lse ? B : 0, need_lse ? L : 0}, q.options());
  F32Params p = {};
  p.q = q.data_ptr<float>();
  p.k = k.data_ptr<float>();
  p.v = v.data_ptr<float>();
  p.relw = rel_w.data_ptr<float>();
  p.relh = rel_h.data_ptr<float>();
  p.out = o.data_ptr<float>();
  p.lse = need_lse ? lse.data_ptr<float>() : nullptr;
  p.B = (int)B; p.L = (int)L; p.H = (int)H; p.W = (int)W;
  p.MW = 2 * (int)W - 1; p.MH = 2 * (int)H - 1;
  p.heads = (int)heads;
  p.qpix = qpix; p.kpix = kpix; p.vpix = vpix; p.opix = opix;
  p.scale = (float)scale;
  p.invW = 1.f / (float)W;
  dim3 grid((unsigned)B, (unsigned)((L + TQ - 1) / TQ));
  F32_ND_SWITCH(D,
                launch_f32<mhsa_f32_fwd_kernel<ND>, fwd_lds<ND>()>(grid, p));
  return {o, lse};
}

// dO, o: rows of stride opix; dq goes to dqk_out, dk to dqk_out + kqoff
// elements (stride qpix both), dv to dv_out (stride vpix), as mhsa_bwd. B and
// L come from lse [B, L]. Returns {dqk_out, dv_out, grw, grh}, all fp32.
std::vector<at::Tensor> mhsa_f32_bwd(
    at::Tensor dO, at::Tensor o, at::Tensor lse, at::Tensor q, at::Tensor k,
    at::Tensor v, at::Tensor rel_w, at::Tensor rel_h, int64_t H, int64_t W,
    int64_t heads, int64_t qpix, int64_t kqoff, int64_t vpix, int64_t opix,
    double scale, at::Tensor dqk_out, at::Tensor dv_out) {
  const char* fn = "mhsa_f32_bwd";
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
                  lse.dim() == 2 && lse.is_contiguous(),
              fn, ": lse must be contiguous fp32 [B, L]");
  const int64_t B = lse.size(0), L = lse.size(1);
  const int D = check_geometry_f32(fn, rel_w, rel_h, L, H, W, B, heads);
  const int64_t N = B / heads;
  check_span_f32(q, N * L, qpix, heads * D, fn, "q");
  check_span_f32(k, N * L, qpix, heads * D, fn, "k");
  check_span_f32(v, N * L, vpix, heads * D, fn, "v");
  check_span_f32(dO, N * L, opix, heads * D, fn, "dO");
  check_span_f32(o, N * L, opix, heads * D, fn, "o");
  check_span_f32(dv_out, N * L, vpix, heads * D, fn, "dv_out");
  check_span_f32(dqk_out, N * L, qpix, heads * D, fn, "dqk_out");
  TORCH_CHECK(kqoff >= 0 && kqoff % 4 == 0 &&
                  (int64_t)(dqk_out.storage().nbytes() / 4) >=
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
  F32Params p = {};
  p.q = q.data_ptr<float>();
  p.k = k.data_ptr<float>();
  p.v = v.data_ptr<float>();
  p.o = o.data_ptr<float>();
  p.dO = dO.data_ptr<float>();
  p.relw = rel_w.data_ptr<float>();
  p.relh = rel_h.data_ptr<float>();
  p.lse = lse.data_ptr<float>();
  p.delta = delta.data_ptr<float>();
  p.dq = dqk_out.data_ptr<float>();
  p.dk = p.dq + kqoff;
  p.dv = dv_out.data_ptr<float>();
  p.drw = drw.data_ptr<float>();
  p.drh = drh.data_ptr<float>();
  p.B = (int)B; p.L = (int)L; p.H = (int)H; p.W = (int)W;
  p.MW = MW; p.MH = MH;
  p.heads = (int)heads;
  p.qpix = qpix; p.kpix = qpix; p.vpix = vpix; p.opix = opix;
  p.scale = (float)scale;
  p.invW = 1.f / (float)W;
  dim3 grid((unsigned)B, (unsigned)((L + TQ - 1) / TQ));
  F32_ND_SWITCH(
      D, launch_f32<mhsa_f32_bwd_q_kernel<ND>, fwd_lds<ND>()>(grid, p));
  F32_ND_SWITCH(
      D, launch_f32<mhsa_f32_bwd_kv_kernel<ND>, bwd_kv_lds<ND>()>(grid, p));

  const int64_t rows = B * L;
  const int rblocks = (int)ceil_div(rows, RG_ROWS);
  const bool det = is_deterministic();  // sampled per launch
  at::Tensor part;  // deterministic mode: [rblocks][M * D], fully written
  if (det) {
    part = at::empty({(int64_t)rblocks, (int64_t)std::max(MW, MH) * D}, fopts);
  } else {
    const int na = MW * D, nc = MH * D;
    hipLaunchKernelGGL(mhsa_f32_zero_kernel,
                       dim3((std::max(na, nc) + 255) / 256), dim3(256), 0,
                       cur_stream(), grw.data_ptr<float>(), na,
                       grh.data_ptr<float>(), nc);
  }
  for (int which = 0; which < 2; ++which) {
    F32RelGradParams rp;
    rp.dr = which == 0 ? drw.data_ptr<float>() : drh.data_ptr<float>();
    rp.q = p.q;
    rp.out = which == 0 ? grw.data_ptr<float>() : grh.data_ptr<float>();
    rp.M = which == 0 ? MW : MH;
    rp.pstride = (int64_t)rp.M * D;
    rp.rows = rows;
    rp.D = D;
    rp.heads = (int)heads;
    rp.L = (int)L;
    rp.qpix = qpix;
    rp.scale = (float)scale;
    if (det) {  // stream-ordered, so the two tables share one workspace
      float* out = rp.out;
      rp.out = part.data_ptr<float>();
      hipLaunchKernelGGL(mhsa_f32_rel_grad_kernel<true>, dim3(rblocks),
                         dim3(256), 0, cur_stream(), rp);
      ordered_reduce<float>(part.data_ptr<float>(), out, rblocks, rp.pstride,
                            1.f);
    } else {
      hipLaunchKernelGGL(mhsa_f32_rel_grad_kernel<false>, dim3(rblocks),
                         dim3(256), 0, cur_stream(), rp);
    }
  }
  return {dqk_out, dv_out, grw, grh};
}
