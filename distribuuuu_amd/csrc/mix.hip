// Batch mixing for mixup / CutMix (trainer: mixing.SoftTargetCriterion).
// The partner of sample n is sample N-1-n (the batch against its own
// reversal), so no permutation tensor exists. Out of place: loaders may hand
// out the same tensor every step.
//
// mixup : out[n] = from_f32(lam * x[n] + (1 - lam) * x[N-1-n]), fp32 math,
//         one rounding to the storage dtype. Flat over the sample: one block
//         per (chunk, n), no index math beyond the chunk base.
// cutmix: out[n] = x[N-1-n] inside [y0, y1) x [x0, x1), x[n] outside; pure
//         copies. Row decomposition: a thread row owns an image row
//         (channels_last, W*C elements) or a (c, h) row (NCHW, W elements),
//         where the box is ONE contiguous element span [s0, s1) on rows
//         y0..y1-1. The inner loop has no division in either layout.
// lam == 1 and lam == 0 run the copy kernel (empty / whole-image box), so
// they return x and x.flip(0) to the bit, signed zeros and NaNs included.
//
// V elements per access: 16-byte packs when base pointers and the sample
// (mixup) or row (cutmix) span are 16-byte multiples, else V = 1.
// Elementwise rules of docs/ARCHITECTURE.md: per-thread pointers advanced by
// a loop-invariant step, no runtime / or % per element.
#include "common.h"

namespace {

template <typename T, int V>
struct alignas(sizeof(T) * V) Vec {
  T v[V];
};

constexpr int MIX_UNROLL = 4;

template <typename T, int V>
__global__ __launch_bounds__(256) void mixup_kernel(
    const T* __restrict__ x, T* __restrict__ out, int N, int64_t S,
    float lam) {
  using P = Vec<T, V>;
  const int n = blockIdx.y;
  const int64_t npacks = S / V;
  int64_t i = (int64_t)blockIdx.x * (256 * MIX_UNROLL) + threadIdx.x;
  const P* a = reinterpret_cast<const P*>(x + (int64_t)n * S) + i;
  const P* b = reinterpret_cast<const P*>(x + (int64_t)(N - 1 - n) * S) + i;
  P* o = reinterpret_cast<P*>(out + (int64_t)n * S) + i;
  const float w = 1.f - lam;
#pragma unroll
  for (int u = 0; u < MIX_UNROLL; ++u) {
    if (i < npacks) {
      const P pa = *a, pb = *b;
      P r;
#pragma unroll
      for (int k = 0; k < V; ++k)
        r.v[k] = from_f32<T>(lam * to_f32(pa.v[k]) + w * to_f32(pb.v[k]));
      *o = r;
    }
    i += 256;
    a += 256;
    b += 256;
    o += 256;
  }
}

// blockDim = (bx, 256 / bx): bx lanes walk a row, blockDim.y rows per block.
// R rows per sample of L elements each; row r is image row r % H.
template <typename T, int V>
__global__ __launch_bounds__(256) void cutmix_kernel(
    const T* __restrict__ x, T* __restrict__ out, int N, int R, int H, int L,
    int64_t S, int y0, int y1, int s0, int s1) {
  using P = Vec<T, V>;
  const int n = blockIdx.y;
  const int r = blockIdx.x * blockDim.y + threadIdx.y;
  if (r >= R) return;
  const int h = (R == H) ? r : r % H;  // once per thread
  const bool inrow = h >= y0 && h < y1;
  const int64_t roff = (int64_t)r * L + (int)threadIdx.x * V;
  const P* own = reinterpret_cast<const P*>(x + (int64_t)n * S + roff);
  const P* oth =
      reinterpret_cast<const P*>(x + (int64_t)(N - 1 - n) * S + roff);
  P* o = reinterpret_cast<P*>(out + (int64_t)n * S + roff);
  const int step = blockDim.x;  // packs
  for (int e = threadIdx.x * V; e < L; e += step * V) {
    const int lo = max(e, s0), hi = min(e + V, s1);
    if (!inrow || hi <= lo) {
      *o = *own;
    } else if (hi - lo == V) {
      *o = *oth;
    } else {
      const P pa = *own, pb = *oth;
      P r2;
#pragma unroll
      for (int k = 0; k < V; ++k)
        r2.v[k] = (e + k >= s0 && e + k < s1) ? pb.v[k] : pa.v[k];
      *o = r2;
    }
    own += step;
    oth += step;
    o += step;
  }
}

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

template <typename T, int V>
void launch_cutmix(const at::Tensor& x, at::Tensor& out, int N, int R, int H,
                   int L, int64_t S, int y0, int y1, int s0, int s1) {
  const int packs = L / V;
  int bx = 8;
  while (bx < packs && bx < 256) bx *= 2;
  const int by = 256 / bx;
  hipLaunchKernelGGL((cutmix_kernel<T, V>),
                     dim3((unsigned)ceil_div(R, by), (unsigned)N),
                     dim3(bx, by), 0, cur_stream(), (const T*)x.data_ptr(),
                     (T*)out.data_ptr(), N, R, H, L, S, y0, y1, s0, s1);
}

}  // namespace

// mode 0 = mixup (box ignored), 1 = cutmix (lam ignored). x: dense
// [N, C, H, W], NCHW-contiguous or channels_last, fp32 or bf16. Returns a new
// tensor of x's layout and dtype.
at::Tensor batch_mix(at::Tensor x, int64_t mode, double lam, int64_t y0,
                     int64_t y1, int64_t x0, int64_t x1) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 4, "batch_mix: x must be [N, C, H, W]");
  TORCH_CHECK(mode == 0 || mode == 1, "batch_mix: mode 0 (mixup) or 1 (cutmix)");
  const bool nchw = x.is_contiguous();
  TORCH_CHECK(nchw || x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "batch_mix: x must be dense, NCHW-contiguous or channels_last");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t S = C * H * W;
  TORCH_CHECK(N >= 1 && S >= 1, "batch_mix: empty tensor");
  TORCH_CHECK(N <= 65535 && S < (int64_t)1 << 31,
              "batch_mix: at most 65535 samples of fewer than 2^31 elements");
  if (mode == 0) {
    TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "batch_mix: lam must be in [0, 1]");
    const float lf = (float)lam;
    if (lf == 1.f) {  // pure copies: x to the bit
      mode = 1;
      y0 = y1 = x0 = x1 = 0;
    } else if (lf == 0.f) {  // x.flip(0) to the bit
      mode = 1;
      y0 = x0 = 0;
      y1 = H;
      x1 = W;
    }
  }
  if (mode == 1)
    TORCH_CHECK(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 &&
                    x1 <= W,
                "batch_mix: box [", y0, ", ", y1, ") x [", x0, ", ", x1,
                ") must lie inside the image with y0 <= y1, x0 <= x1");
  auto out = at::empty_like(x);  // dense input: same strides
  TORCH_CHECK(out.strides() == x.strides(), "batch_mix: layout not preserved");
  const bool base16 = aligned16(x.data_ptr()) && aligned16(out.data_ptr());
  DISPATCH_FLOAT_AND_BF16(x.scalar_type(), "batch_mix", [&] {
    constexpr int PV = 16 / sizeof(scalar_t);
    if (mode == 0) {
      const bool vec = base16 && S % PV == 0;
      const int64_t npacks = vec ? S / PV : S;
      dim3 grid((unsigned)ceil_div(npacks, 256 * MIX_UNROLL), (unsigned)N);
      if (vec)
        hipLaunchKernelGGL((mixup_kernel<scalar_t, PV>), grid, dim3(256), 0,
                           cur_stream(), (const scalar_t*)x.data_ptr(),
                           (scalar_t*)out.data_ptr(), (int)N, S, (float)lam);
      else
        hipLaunchKernelGGL((mixup_kernel<scalar_t, 1>), grid, dim3(256), 0,
                           cur_stream(), (const scalar_t*)x.data_ptr(),
                           (scalar_t*)out.data_ptr(), (int)N, S, (float)lam);
    } else {
      // rows: NCHW (c, h) rows of W; channels_last image rows of W*C
      const int R = (int)(nchw ? C * H : H);
      const int L = (int)(nchw ? W : W * C);
      const int s0 = (int)(nchw ? x0 : x0 * C);
      const int s1 = (int)(nchw ? x1 : x1 * C);
      if (base16 && L % PV == 0)
        launch_cutmix<scalar_t, PV>(x, out, (int)N, R, (int)H, L, S, (int)y0,
                                    (int)y1, s0, s1);
      else
        launch_cutmix<scalar_t, 1>(x, out, (int)N, R, (int)H, L, S, (int)y0,
                                   (int)y1, s0, s1);
    }
  });
  return out;
}
