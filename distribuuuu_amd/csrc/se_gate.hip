// Squeeze-excite gate s = sigmoid(W2 * act(W1 * p + b1) + b2), forward and
// backward, for pooled inputs p [N, C] and squeeze widths Cr of any size.
//
// Every GEMM here is skinny (a batch of rows against a few-MB weight), so all
// of them run on 16x16 tiles of v_mfma_f32_16x16x32_bf16 with fp32
// accumulation and load their fragments per lane: 16-byte loads where the row
// base and the reduction span are aligned, guarded element loads otherwise.
// No host-side padding, no atomics, one writer per output element and a
// fixed summation order, so results repeat bit for bit.
//
//   forward   se_gemm_kernel  FC1: z1 = p W1^T + b1 (fp32), h = act(z1) (bf16)
//             se_gemm_kernel  FC2: s = sigmoid(h W2^T + b2)
//   backward  se_gemm_kernel  hidden: g2 = gs s (1-s) on the fly (and
//                             stored), g1 = (g2 W2) * act'(z1)
//             se_gemm_kernel  input:  gp = g1 W1
//             se_wgrad_kernel gW2 = g2^T h, gW1 = g1^T p, gb2, gb1
//
// Tile shapes: DEEP (reduction long, few outputs: FC1, hidden) gives a block
// one 16x16 tile and splits the reduction into contiguous quarters over its
// four waves; the partial tiles meet in LDS and wave 0 sums them in wave
// order. Wide (short reduction, many outputs: FC2, input) gives each wave
// its own 16-column tile of a 16x64 block tile.
//
// Operands whose reduction index is memory-strided (W2 over c, W1 over r,
// everything over n) are staged per wave in natural [32 k][16 col] order and
// read transposed with ds_read_b64_tr_b16 (lane semantics: wgrad.hip).
//
// h, z1 and g1 have their row stride rounded up to 32 with the pad columns
// written as zeros, so they are always 16-byte loadable and a reduction over
// them never multiplies recycled Inf/NaN bit patterns by zero.
#include "common.h"

// packed fp32 math (v_pk_*_f32) is kept out of this file's kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

typedef __attribute__((ext_vector_type(4))) float f32x4s;
typedef __bf16 bf16x8s __attribute__((ext_vector_type(8)));
typedef unsigned short bf16raw;

namespace {

constexpr int ACT_RELU = 1, ACT_SILU = 2;  // ids of functional._ACTS
constexpr int EPI_FC1 = 0, EPI_GATE = 1, EPI_G1 = 2, EPI_PLAIN = 3;
constexpr int STAGE_BYTES = 32 * 16 * 2;  // one [32 k][16 col] bf16 subtile

union Frag {
  uint4 q;
  bf16raw e[8];
  bf16x8s v;
};

DEV_INLINE float raw_f32(bf16raw b) {
  return __uint_as_float((unsigned)b << 16);
}
DEV_INLINE bf16raw f32_raw(float f) {
  return __bfloat16_as_ushort(__float2bfloat16(f));
}
DEV_INLINE float sigmoidf(float z) { return 1.f / (1.f + __expf(-z)); }

template <int ACT>
DEV_INLINE float act_fwd(float z) {
  if constexpr (ACT == ACT_RELU) return fmaxf(z, 0.f);
  return z * sigmoidf(z);
}
template <int ACT>
DEV_INLINE float act_grad(float z) {
  if constexpr (ACT == ACT_RELU) return z > 0.f ? 1.f : 0.f;
  const float sg = sigmoidf(z);
  return sg * (1.f + z * (1.f - sg));
}

// Elements [col, col + 8) of row `row` of a [rows][ld] matrix, zero where
// row >= rows or the column >= cols. vec: ld % 8 == 0 and a 16-byte aligned
// base, so any col % 8 == 0 span inside the row is one dwordx4.
DEV_INLINE Frag load_frag(const bf16raw* src, int ld, int row, int rows,
                          int col, int cols, bool vec) {
  Frag f;
  f.q = uint4{0, 0, 0, 0};
  if (row < rows) {
    const bf16raw* r = src + (int64_t)row * ld + col;
    if (vec && col + 8 <= cols) {
      f.q = *reinterpret_cast<const uint4*>(r);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (col + i < cols) f.e[i] = r[i];
    }
  }
  return f;
}

DEV_INLINE void store_frag(bf16raw* dst, int ld, int row, int rows, int col,
                           int cols, bool vec, const Frag& f) {
  if (row >= rows) return;
  bf16raw* r = dst + (int64_t)row * ld + col;
  if (vec && col + 8 <= cols) {
    *reinterpret_cast<uint4*>(r) = f.q;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (col + i < cols) r[i] = f.e[i];
  }
}

// Stage rows [k0, k0 + 32) x columns [c0, c0 + 16) of src[krows][ld] into a
// wave-private subtile in natural order (32-byte rows), zero outside the
// matrix: lane t owns row t / 2, columns (t % 2) * 8 .. + 8.
DEV_INLINE void stage_subtile(char* lds, const bf16raw* src, int ld, int k0,
                              int krows, int c0, int cols, bool vec,
                              int lane) {
  const int kr = lane >> 1, c8 = (lane & 1) * 8;
  const Frag f = load_frag(src, ld, k0 + kr, krows, c0 + c8, cols, vec);
  *reinterpret_cast<uint4*>(lds + kr * 32 + c8 * 2) = f.q;
}

// Transposed fragment of a staged subtile: lane l receives column l & 15,
// rows (l >> 4) * 8 .. + 8, the MFMA operand layout with k = subtile row.
DEV_INLINE bf16x8s tr_read(unsigned lds_addr, int lane) {
  union {
    uint2 h[2];
    bf16x8s v;
  } u;
  const int s = lane & 15, g = lane >> 4;
  const unsigned a0 = lds_addr + (g * 8 + (s >> 2)) * 32 + (s & 3) * 8;
  const unsigned a1 = a0 + 4 * 32;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\t"
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(u.h[0]), "=&v"(u.h[1])
      : "v"(a0), "v"(a1)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  return u.v;
}

struct GemmParams {
  const bf16raw* a;     // [N][lda] rows, reduction-contiguous (EPI_G1: gs)
  const bf16raw* a2;    // EPI_G1: s [N][lda]
  bf16raw* g2;          // EPI_G1: g2 [N][lda] out
  const bf16raw* w;     // BT ? [K][ldw] (k rows, j cols) : [J][ldw]
  const bf16raw* bias;  // [J], EPI_FC1 / EPI_GATE
  const float* zin;     // EPI_G1: z1 [N][ldo]
  float* z;             // EPI_FC1: z1 [N][ldo] out
  bf16raw* out;         // [N][ldo]
  int N, K, J;          // rows, reduction length, outputs
  int ka;               // readable length of an A row (>= K; zeros past K)
  int lda, ldw, ldo;
  int jout;             // columns written: ldo where the pads are zeroed
  bool avec, wvec;
};

// out[n, j] = epi(sum_k a[n, k] * w(j, k)). grid (j-tiles, ceil(N / 16)).
template <bool DEEP, bool BT, int EPI, int ACT>
__global__ __launch_bounds__(256) void se_gemm_kernel(GemmParams p) {
  __shared__ __align__(16) char smem[4 * STAGE_BYTES + 4 * 256 * 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.y * 16;
  const int j0 = (DEEP ? blockIdx.x : blockIdx.x * 4 + wid) * 16;
  if (!DEEP && j0 >= p.jout) return;  // no block barrier on the wide path

  const int nsteps = (p.K + 31) >> 5;
  int s0 = 0, s1 = nsteps;
  if (DEEP) {
    const int q = (nsteps + 3) >> 2;
    s0 = min(wid * q, nsteps);
    s1 = min(s0 + q, nsteps);
  }
  char* stg = smem + wid * STAGE_BYTES;
  const unsigned stg_addr = (unsigned)(unsigned long long)stg;
  const bool g2_owner = EPI == EPI_G1 && blockIdx.x == 0 && (DEEP || wid == 0);

  f32x4s acc = {0.f, 0.f, 0.f, 0.f};
  for (int st = s0; st < s1; ++st) {
    const int k = st * 32 + kq * 8;
    Frag a;
    if constexpr (EPI == EPI_G1) {
      const Frag gs = load_frag(p.a, p.lda, n0 + il, p.N, k, p.ka, p.avec);
      const Frag sv = load_frag(p.a2, p.lda, n0 + il, p.N, k, p.ka, p.avec);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float s = raw_f32(sv.e[i]);
        a.e[i] = f32_raw(raw_f32(gs.e[i]) * s * (1.f - s));
      }
      if (g2_owner)
        store_frag(p.g2, p.lda, n0 + il, p.N, k, p.ka, p.avec, a);
    } else {
      a = load_frag(p.a, p.lda, n0 + il, p.N, k, p.ka, p.avec);
    }
    Frag b;
    if constexpr (BT) {
      stage_subtile(stg, p.w, p.ldw, st * 32, p.K, j0, p.J, p.wvec, lane);
      b.v = tr_read(stg_addr, lane);
    } else {
      b = load_frag(p.w, p.ldw, j0 + il, p.J, k, p.K, p.wvec);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
  }

  // D layout: column il, rows kq * 4 + rr
  if constexpr (DEEP) {
    float* part = reinterpret_cast<float*>(smem + 4 * STAGE_BYTES);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      part[wid * 256 + (kq * 4 + rr) * 16 + il] = acc[rr];
    __syncthreads();
    if (wid != 0) return;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int e = (kq * 4 + rr) * 16 + il;
      acc[rr] = ((part[e] + part[256 + e]) + part[512 + e]) + part[768 + e];
    }
  }

  const int j = j0 + il;
  if (j >= p.jout) return;
  const bool jv = j < p.J;
  float bj = 0.f;
  if constexpr (EPI == EPI_FC1 || EPI == EPI_GATE)
    if (jv) bj = raw_f32(p.bias[j]);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int n = n0 + kq * 4 + rr;
    if (n >= p.N) continue;
    const int64_t o = (int64_t)n * p.ldo + j;
    if constexpr (EPI == EPI_FC1) {
      const float z = jv ? acc[rr] + bj : 0.f;
      p.z[o] = z;
      p.out[o] = f32_raw(jv ? act_fwd<ACT>(z) : 0.f);
    } else if constexpr (EPI == EPI_GATE) {
      p.out[o] = f32_raw(sigmoidf(acc[rr] + bj));
    } else if constexpr (EPI == EPI_G1) {
      p.out[o] = f32_raw(jv ? acc[rr] * act_grad<ACT>(p.zin[o]) : 0.f);
    } else {
      p.out[o] = f32_raw(acc[rr]);
    }
  }
}

struct WgradParams {
  const bf16raw* g2;  // [N][C]
  const bf16raw* h;   // [N][Crp]
  const bf16raw* g1;  // [N][Crp]
  const bf16raw* p;   // [N][C]
  bf16raw* gw2;       // [C][Cr]
  bf16raw* gw1;       // [Cr][C]
  bf16raw* gb2;       // [C]
  bf16raw* gb1;       // [Cr]
  int N, C, Cr, Crp;
  int ct, rt;  // 16-wide tiles of C and of Cr
  bool cvec;   // rows of stride C are 16-byte loadable
};

// One wave per 16x16 tile of gW2 = g2^T h (tiles 0 .. ct*rt) or of
// gW1 = g1^T p (the next ct*rt). The wave reduces over all N rows itself, in
// ascending order. The tiles of a row-tile's first column also take the bias
// gradient: the column sums of the staged g operand, as one more MFMA against
// a fragment of ones.
__global__ __launch_bounds__(256) void se_wgrad_kernel(WgradParams p) {
  __shared__ __align__(16) char smem[4 * 2 * STAGE_BYTES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int T = p.ct * p.rt;
  int tile = blockIdx.x * 4 + wid;
  if (tile >= 2 * T) return;  // waves are independent: no block barrier
  const bool second = tile >= T;
  if (second) tile -= T;

  const bf16raw *x, *y;
  bf16raw *out, *gb;
  int ldx, ldy, I, J, xcols, ycols, it, jt;
  bool xvec, yvec;
  if (!second) {  // gW2[c][r] = sum_n g2[n][c] * h[n][r]
    x = p.g2, ldx = p.C, xcols = p.C, xvec = p.cvec, I = p.C;
    y = p.h, ldy = p.Crp, ycols = p.Crp, yvec = true, J = p.Cr;
    out = p.gw2, gb = p.gb2;
    it = tile / p.rt, jt = tile - it * p.rt;
  } else {  // gW1[r][c] = sum_n g1[n][r] * p[n][c]
    x = p.g1, ldx = p.Crp, xcols = p.Crp, xvec = true, I = p.Cr;
    y = p.p, ldy = p.C, ycols = p.C, yvec = p.cvec, J = p.C;
    out = p.gw1, gb = p.gb1;
    it = tile / p.ct, jt = tile - it * p.ct;
  }

  char* stgx = smem + wid * 2 * STAGE_BYTES;
  char* stgy = stgx + STAGE_BYTES;
  const unsigned ax = (unsigned)(unsigned long long)stgx;
  const unsigned ay = (unsigned)(unsigned long long)stgy;
  Frag ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones.e[i] = 0x3F80;  // bf16 1.0

  f32x4s acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < p.N; n0 += 32) {
    stage_subtile(stgx, x, ldx, n0, p.N, it * 16, xcols, xvec, lane);
    stage_subtile(stgy, y, ldy, n0, p.N, jt * 16, ycols, yvec, lane);
    const bf16x8s a = tr_read(ax, lane);
    const bf16x8s b = tr_read(ay, lane);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    if (jt == 0)
      accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, ones.v, accb, 0, 0, 0);
  }

  const int j = jt * 16 + il;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = it * 16 + kq * 4 + rr;
    if (i >= I) continue;
    if (j < J) out[(int64_t)i * J + j] = f32_raw(acc[rr]);
    if (jt == 0 && il == 0) gb[i] = f32_raw(accb[rr]);
  }
}

inline const bf16raw* rawp(const at::Tensor& t) {
  return reinterpret_cast<const bf16raw*>(t.data_ptr());
}
inline bf16raw* rawp_mut(at::Tensor& t) {
  return reinterpret_cast<bf16raw*>(t.data_ptr());
}
// rows of stride ld starting at t's base take 16-byte loads
inline bool vec_ok(const at::Tensor& t, int ld) {
  return ld % 8 == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}
inline int pad32(int v) { return (v + 31) / 32 * 32; }

void check_bf16(const at::Tensor& t, const char* name) {
  CHECK_GPU(t);
  TORCH_CHECK(t.scalar_type() == at::ScalarType::BFloat16, "se_gate: ", name,
              " must be bf16");
}

// a dense [rows][cols] view of a [rows, cols(, 1, 1)] tensor; a copy only
// where the tensor is not already laid out that way
at::Tensor as_matrix(const at::Tensor& t, int64_t rows, int64_t cols,
                     const char* name) {
  TORCH_CHECK(t.numel() == rows * cols && t.size(0) == rows, "se_gate: ",
              name, " has shape ", t.sizes(), ", expected [", rows, ", ",
              cols, "(, 1, 1)]");
  return t.reshape({rows, cols}).contiguous();
}

template <bool DEEP, bool BT, int EPI>
void launch_gemm(const GemmParams& p, int act) {
  const int jtiles = (int)ceil_div(p.jout, DEEP ? 16 : 64);
  const dim3 grid(jtiles, (unsigned)ceil_div(p.N, 16));
  if constexpr (EPI == EPI_FC1 || EPI == EPI_G1) {
    if (act == ACT_RELU)
      hipLaunchKernelGGL((se_gemm_kernel<DEEP, BT, EPI, ACT_RELU>), grid,
                         dim3(256), 0, cur_stream(), p);
    else
      hipLaunchKernelGGL((se_gemm_kernel<DEEP, BT, EPI, ACT_SILU>), grid,
                         dim3(256), 0, cur_stream(), p);
  } else {
    hipLaunchKernelGGL((se_gemm_kernel<DEEP, BT, EPI, 0>), grid, dim3(256), 0,
                       cur_stream(), p);
  }
}

// the K split pays once every wave has at least one 32-deep step
inline bool deep_shape(int K, int J) { return K >= 128 && K >= J; }

}  // namespace

// -> {s [N, C, 1, 1], h [N, Crp] bf16, z1 [N, Crp] fp32}, Crp = Cr up to 32
std::vector<at::Tensor> se_gate_fwd(at::Tensor p, at::Tensor w1, at::Tensor b1,
                                    at::Tensor w2, at::Tensor b2,
                                    int64_t act) {
  check_bf16(p, "p"), check_bf16(w1, "w1"), check_bf16(b1, "b1");
  check_bf16(w2, "w2"), check_bf16(b2, "b2");
  TORCH_CHECK(act == ACT_RELU || act == ACT_SILU, "se_gate: act relu or silu");
  TORCH_CHECK(p.dim() == 2 || p.dim() == 4, "se_gate: p is [N, C(, 1, 1)]");
  const int64_t N = p.size(0), C = p.size(1), Cr = w1.size(0);
  TORCH_CHECK(N >= 1 && C >= 1 && Cr >= 1 && N <= 65535 * 16 &&
                  C < (1 << 24) && Cr < (1 << 24),
              "se_gate: shape out of range");
  auto pm = as_matrix(p, N, C, "p");
  auto w1m = as_matrix(w1, Cr, C, "w1");
  auto w2m = as_matrix(w2, C, Cr, "w2");
  auto b1c = as_matrix(b1, Cr, 1, "b1");
  auto b2c = as_matrix(b2, C, 1, "b2");
  const int Crp = pad32((int)Cr);

  auto s = at::empty({N, C, 1, 1},
                     p.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto h = at::empty({N, Crp}, p.options());
  auto z1 = at::empty({N, Crp}, p.options().dtype(at::kFloat));

  GemmParams f1{};
  f1.a = rawp(pm), f1.w = rawp(w1m), f1.bias = rawp(b1c);
  f1.z = z1.data_ptr<float>(), f1.out = rawp_mut(h);
  f1.N = (int)N, f1.K = (int)C, f1.J = (int)Cr, f1.ka = (int)C;
  f1.lda = (int)C, f1.ldw = (int)C, f1.ldo = Crp, f1.jout = Crp;
  f1.avec = vec_ok(pm, (int)C), f1.wvec = vec_ok(w1m, (int)C);
  if (deep_shape(f1.K, f1.J))
    launch_gemm<true, false, EPI_FC1>(f1, (int)act);
  else
    launch_gemm<false, false, EPI_FC1>(f1, (int)act);

  GemmParams f2{};
  f2.a = rawp(h), f2.w = rawp(w2m), f2.bias = rawp(b2c);
  f2.out = rawp_mut(s);
  f2.N = (int)N, f2.K = (int)Cr, f2.J = (int)C, f2.ka = Crp;
  f2.lda = Crp, f2.ldw = (int)Cr, f2.ldo = (int)C, f2.jout = (int)C;
  f2.avec = true, f2.wvec = vec_ok(w2m, (int)Cr);
  if (deep_shape(f2.K, f2.J))
    launch_gemm<true, false, EPI_GATE>(f2, 0);
  else
    launch_gemm<false, false, EPI_GATE>(f2, 0);
  return {s, h, z1};
}

// -> {gp (p's shape), gw1, gb1, gw2, gb2, g1 [N, Crp], g2 [N, C]}
std::vector<at::Tensor> se_gate_bwd(at::Tensor gs, at::Tensor s, at::Tensor h,
                                    at::Tensor z1, at::Tensor p, at::Tensor w1,
                                    at::Tensor w2, int64_t act) {
  check_bf16(gs, "gs"), check_bf16(s, "s"), check_bf16(h, "h");
  check_bf16(p, "p"), check_bf16(w1, "w1"), check_bf16(w2, "w2");
  CHECK_GPU(z1);
  TORCH_CHECK(act == ACT_RELU || act == ACT_SILU, "se_gate: act relu or silu");
  const int64_t N = p.size(0), C = p.size(1), Cr = w1.size(0);
  const int Crp = pad32((int)Cr);
  TORCH_CHECK(h.dim() == 2 && h.size(0) == N && h.size(1) == Crp &&
                  h.is_contiguous() && z1.sizes() == h.sizes() &&
                  z1.is_contiguous() &&
                  z1.scalar_type() == at::ScalarType::Float,
              "se_gate_bwd: h / z1 are the forward's [N, Crp] workspaces");
  auto gsm = as_matrix(gs, N, C, "gs");
  auto sm = as_matrix(s, N, C, "s");
  auto pm = as_matrix(p, N, C, "p");
  auto w1m = as_matrix(w1, Cr, C, "w1");
  auto w2m = as_matrix(w2, C, Cr, "w2");

  const auto cl = p.options().memory_format(at::MemoryFormat::ChannelsLast);
  auto g2 = at::empty({N, C}, p.options());
  auto g1 = at::empty({N, Crp}, p.options());
  auto gp = at::empty({N, C}, p.options());
  // shape and strides of conv2d_wgrad's 1x1 weight gradients
  auto gw1 = at::empty({Cr, C, 1, 1}, cl);
  auto gw2 = at::empty({C, Cr, 1, 1}, cl);
  auto gb1 = at::empty({Cr}, p.options());
  auto gb2 = at::empty({C}, p.options());

  GemmParams hd{};
  hd.a = rawp(gsm), hd.a2 = rawp(sm), hd.g2 = rawp_mut(g2);
  hd.w = rawp(w2m), hd.zin = z1.data_ptr<float>(), hd.out = rawp_mut(g1);
  hd.N = (int)N, hd.K = (int)C, hd.J = (int)Cr, hd.ka = (int)C;
  hd.lda = (int)C, hd.ldw = (int)Cr, hd.ldo = Crp, hd.jout = Crp;
  hd.avec = vec_ok(gsm, (int)C) && vec_ok(sm, (int)C) && vec_ok(g2, (int)C);
  hd.wvec = vec_ok(w2m, (int)Cr);
  if (deep_shape(hd.K, hd.J))
    launch_gemm<true, true, EPI_G1>(hd, (int)act);
  else
    launch_gemm<false, true, EPI_G1>(hd, (int)act);

  GemmParams in{};
  in.a = rawp(g1), in.w = rawp(w1m), in.out = rawp_mut(gp);
  in.N = (int)N, in.K = (int)Cr, in.J = (int)C, in.ka = Crp;
  in.lda = Crp, in.ldw = (int)C, in.ldo = (int)C, in.jout = (int)C;
  in.avec = true, in.wvec = vec_ok(w1m, (int)C);
  if (deep_shape(in.K, in.J))
    launch_gemm<true, true, EPI_PLAIN>(in, 0);
  else
    launch_gemm<false, true, EPI_PLAIN>(in, 0);

  WgradParams wp{};
  wp.g2 = rawp(g2), wp.h = rawp(h), wp.g1 = rawp(g1), wp.p = rawp(pm);
  wp.gw2 = rawp_mut(gw2), wp.gw1 = rawp_mut(gw1);
  wp.gb2 = rawp_mut(gb2), wp.gb1 = rawp_mut(gb1);
  wp.N = (int)N, wp.C = (int)C, wp.Cr = (int)Cr, wp.Crp = Crp;
  wp.ct = (int)ceil_div(C, 16), wp.rt = (int)ceil_div(Cr, 16);
  wp.cvec = vec_ok(g2, (int)C) && vec_ok(pm, (int)C);
  const int64_t tiles = 2 * (int64_t)wp.ct * wp.rt;
  hipLaunchKernelGGL(se_wgrad_kernel, dim3((unsigned)ceil_div(tiles, 4)),
                     dim3(256), 0, cur_stream(), wp);

  return {gp.view(p.sizes()), gw1, gb1, gw2, gb2, g1, g2};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
