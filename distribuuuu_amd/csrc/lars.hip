// Fused multi-tensor LARS step (You, Gitman, Ginsburg 2017) on top of the
// SGD-momentum update of sgd.hip. Three launches per step, ordered by kernel
// boundaries only (no grid barrier, no cross-block flag, no atomics):
//
//   1. lars_sqnorm_kernel   one 256-thread block per chunk record writes its
//                           fp32 partial (sum w^2, sum g^2) to part[chunk]
//   2. lars_combine_kernel  one block per tensor record adds that tensor's
//                           chunk partials in a fixed order, forms the trust
//                           ratio q and publishes (sum w^2, sum g^2) and q
//   3. lars_kernel[_dev]    sgd.hip's chunk update with g_eff = q*(g + wd*w)
//
// Table: int64 [nchunks + ntensors, 6]. The first nchunks rows are sgd.hip's
// chunk records; the flags word additionally carries, from bit 8 up, the
// tensor's slot (its position in the param group), where q is read. The
// ntensors rows after them are [first_chunk, chunk_count, slot, adapt, 0, 0].
//
// Every sum has one order whatever the pointers' alignment and whatever the
// determinism mode: a thread owns elements 4*(t + 256*k) .. +3 of its chunk
// and adds them k-major into one accumulator; aligned chunks fetch them as
// one 16-byte (fp32) or 8-byte (bf16) load, others as four scalar loads.
#include "common.h"

namespace {

constexpr int kChunk = 16384;   // ops/optim.py _CHUNK
constexpr int kThreads = 256;
constexpr int kPacks = kChunk / (4 * kThreads);  // 4-packs per thread: 16
constexpr int kSlotShift = 8;   // slot lives in flags bits 8..31

template <bool VEC>
DEV_INLINE void load4(const float* p, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[j];
  }
}

template <bool VEC>
DEV_INLINE void load4(const __hip_bfloat16* p, float (&v)[4]) {
  if constexpr (VEC) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(x.x << 16);
    v[1] = __uint_as_float(x.x & 0xffff0000u);
    v[2] = __uint_as_float(x.y << 16);
    v[3] = __uint_as_float(x.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = to_f32(p[j]);
  }
}

// Full chunk: 16 packs per thread, 4 of each stream in flight at a time.
// Per-thread pointers advance by a constant; no index math in the loop.
template <typename G, bool VEC>
DEV_INLINE void sq_full(const float* wp, const G* gp, float& sw, float& sg) {
#pragma unroll
  for (int k = 0; k < kPacks; k += 4) {
    float w[4][4], g[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      load4<VEC>(wp + u * 4 * kThreads, w[u]);
      load4<VEC>(gp + u * 4 * kThreads, g[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sw += w[u][j] * w[u][j];
        sg += g[u][j] * g[u][j];
      }
    wp += 16 * kThreads;
    gp += 16 * kThreads;
  }
}

// Partial chunk (a tensor's last): same element ownership and order, every
// load guarded by the element count.
template <typename G>
DEV_INLINE void sq_tail(const float* wp, const G* gp, int rem, float& sw,
                        float& sg) {
  // rem: elements from this thread's first pack to the end of the chunk
  for (; rem > 0; rem -= 4 * kThreads) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < rem) {
        const float w = wp[j];
        const float g = to_f32(gp[j]);
        sw += w * w;
        sg += g * g;
      }
    }
    wp += 4 * kThreads;
    gp += 4 * kThreads;
  }
}

template <typename G>
DEV_INLINE void sq_chunk(const float* w, const G* g, int count, float& sw,
                         float& sg) {
  const int t = threadIdx.x;
  if (count == kChunk) {
    const bool vec = (((uintptr_t)w & 15) | ((uintptr_t)g & (4 * sizeof(G) - 1))) == 0;
    if (vec)
      sq_full<G, true>(w + 4 * t, g + 4 * t, sw, sg);
    else
      sq_full<G, false>(w + 4 * t, g + 4 * t, sw, sg);
  } else {
    sq_tail<G>(w + 4 * t, g + 4 * t, count - 4 * t, sw, sg);
  }
}

__global__ __launch_bounds__(kThreads) void lars_sqnorm_kernel(
    const long long* __restrict__ recs, float* __restrict__ part) {
  __shared__ float lds[2][16];
  const long long* rec = recs + (int64_t)blockIdx.x * 6;
  const int64_t off = rec[4];
  const int count = min((int)(rec[5] & 0xffffffffll), kChunk);
  const int flags = (int)(rec[5] >> 32);
  const float* master = (const float*)rec[3] + off;
  float sw = 0.f, sg = 0.f;
  if (flags & 2)
    sq_chunk(master, (const __hip_bfloat16*)rec[0] + off, count, sw, sg);
  else
    sq_chunk(master, (const float*)rec[0] + off, count, sw, sg);
  sw = block_reduce_sum<false>(sw, lds[0]);
  sg = block_reduce_sum<false>(sg, lds[1]);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = sw;
    part[2 * (int64_t)blockIdx.x + 1] = sg;
  }
}

// One block per tensor record. Thread t adds partials t, t+256, ... in
// ascending order, then the block tree: one fixed order for any chunk count.
__global__ __launch_bounds__(kThreads) void lars_combine_kernel(
    const long long* __restrict__ recs, int nchunks,
    const float* __restrict__ part, float* __restrict__ sqnorm,
    float* __restrict__ qout, int nslots, float trust, float wd, float eps) {
  __shared__ float lds[2][16];
  const long long* rec = recs + ((int64_t)nchunks + blockIdx.x) * 6;
  const long long first = rec[0], cnt = rec[1], slot = rec[2];
  const bool adapt = rec[3] != 0;
  // a record that points outside the tables is dropped, never followed
  if (first < 0 || cnt < 0 || first + cnt > nchunks || slot < 0 ||
      slot >= nslots)
    return;
  const float* p = part + 2 * (first + threadIdx.x);
  float sw = 0.f, sg = 0.f;
  for (int i = threadIdx.x; i < (int)cnt; i += kThreads) {
    sw += p[0];
    sg += p[1];
    p += 2 * kThreads;
  }
  sw = block_reduce_sum<false>(sw, lds[0]);
  sg = block_reduce_sum<false>(sg, lds[1]);
  if (threadIdx.x == 0) {
    float q = 1.f;
    if (adapt && sw > 0.f && sg > 0.f) {
      const float nw = sqrtf(sw), ng = sqrtf(sg);
      q = trust * nw / (ng + wd * nw + eps);
    }
    sqnorm[2 * slot] = sw;
    sqnorm[2 * slot + 1] = sg;
    qout[slot] = q;
  }
}

// sgd.hip's sgd_chunk with the tensor's trust ratio applied to g + wd*w.
// Shared by both kernels below, which differ only in where `lr` comes from.
DEV_INLINE void lars_chunk(const long long* __restrict__ recs,
                           const float* __restrict__ qv, int nslots, float lr,
                           float mu, float damp, float wd, int nesterov) {
  const long long* rec = recs + (int64_t)blockIdx.x * 6;
  const void* grad = (const void*)rec[0];
  void* param = (void*)rec[1];
  float* mom = (float*)rec[2];
  float* master = (float*)rec[3];
  const int64_t off = rec[4];
  const int count = (int)(rec[5] & 0xffffffffll);
  const unsigned flags = (unsigned)((unsigned long long)rec[5] >> 32);
  const int slot = (int)(flags >> kSlotShift);
  if (slot >= nslots) return;
  const float q = qv[slot];
  const bool p_bf16 = flags & 1, g_bf16 = flags & 2;
  const float gscale = (flags & 4) ? 1.f : 1.f - damp;
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int64_t j = off + i;
    float g = g_bf16 ? to_f32(((const __hip_bfloat16*)grad)[j])
                     : ((const float*)grad)[j];
    float w = master[j];
    if (wd != 0.f) g += wd * w;
    g *= q;
    float m = mom[j] * mu + gscale * g;
    mom[j] = m;
    const float upd = nesterov ? g + mu * m : m;
    w -= lr * upd;
    master[j] = w;
    if (p_bf16)
      ((__hip_bfloat16*)param)[j] = from_f32<__hip_bfloat16>(w);
    else if ((void*)master != param)
      ((float*)param)[j] = w;
  }
}

__global__ void lars_kernel(const long long* __restrict__ recs,
                            const float* __restrict__ qv, int nslots, float lr,
                            float mu, float damp, float wd, int nesterov) {
  lars_chunk(recs, qv, nslots, lr, mu, damp, wd, nesterov);
}

__global__ void lars_kernel_dev(const long long* __restrict__ recs,
                                const float* __restrict__ qv, int nslots,
                                const float* __restrict__ lr_dev, float mu,
                                float damp, float wd, int nesterov) {
  const float lr = *lr_dev;
  lars_chunk(recs, qv, nslots, lr, mu, damp, wd, nesterov);
}

// Checks shared by both entry points, then stages 1 and 2.
int lars_norms(const at::Tensor& table, int64_t nchunks,
               const at::Tensor& part, const at::Tensor& sqnorm,
               const at::Tensor& q, double weight_decay, double trust_coef,
               double eps) {
  CHECK_GPU(table);
  CHECK_GPU(part);
  CHECK_GPU(sqnorm);
  CHECK_GPU(q);
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 &&
                  table.size(1) == 6 && table.is_contiguous(),
              "lars table must be contiguous int64 [n, 6]");
  TORCH_CHECK(nchunks >= 0 && nchunks <= table.size(0) &&
                  table.size(0) < (1ll << 31),
              "lars: chunk count outside the table");
  for (const at::Tensor* t : {&part, &sqnorm, &q})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(),
                "lars workspaces must be contiguous float32");
  TORCH_CHECK(part.numel() >= 2 * nchunks,
              "lars: partials workspace too small");
  TORCH_CHECK(q.numel() < (1 << 23) && sqnorm.numel() == 2 * q.numel(),
              "lars: sqnorm must be [len(q), 2]");
  const int ntens = (int)(table.size(0) - nchunks);
  const long long* recs = (const long long*)table.data_ptr();
  if (nchunks > 0)
    hipLaunchKernelGGL(lars_sqnorm_kernel, dim3((int)nchunks), dim3(kThreads),
                       0, cur_stream(), recs, (float*)part.data_ptr());
  if (ntens > 0)
    hipLaunchKernelGGL(lars_combine_kernel, dim3(ntens), dim3(kThreads), 0,
                       cur_stream(), recs, (int)nchunks,
                       (const float*)part.data_ptr(),
                       (float*)sqnorm.data_ptr(), (float*)q.data_ptr(),
                       (int)q.numel(), (float)trust_coef, (float)weight_decay,
                       (float)eps);
  return (int)nchunks;
}

}  // namespace

void lars_step(at::Tensor table, int64_t nchunks, at::Tensor part,
               at::Tensor sqnorm, at::Tensor q, double lr, double momentum,
               double dampening, double weight_decay, bool nesterov,
               double trust_coef, double eps) {
  const int n = lars_norms(table, nchunks, part, sqnorm, q, weight_decay,
                           trust_coef, eps);
  if (n == 0) return;
  hipLaunchKernelGGL(lars_kernel, dim3(n), dim3(256), 0, cur_stream(),
                     (const long long*)table.data_ptr(),
                     (const float*)q.data_ptr(), (int)q.numel(), (float)lr,
                     (float)momentum, (float)dampening, (float)weight_decay,
                     nesterov ? 1 : 0);
}

void lars_step_dev(at::Tensor table, int64_t nchunks, at::Tensor part,
                   at::Tensor sqnorm, at::Tensor q, at::Tensor lr_dev,
                   double momentum, double dampening, double weight_decay,
                   bool nesterov, double trust_coef, double eps) {
  CHECK_GPU(lr_dev);
  TORCH_CHECK(lr_dev.scalar_type() == at::kFloat && lr_dev.numel() == 1,
              "lars_step_dev: lr must be a float32 tensor of one element");
  const int n = lars_norms(table, nchunks, part, sqnorm, q, weight_decay,
                           trust_coef, eps);
  if (n == 0) return;
  hipLaunchKernelGGL(lars_kernel_dev, dim3(n), dim3(256), 0, cur_stream(),
                     (const long long*)table.data_ptr(),
                     (const float*)q.data_ptr(), (int)q.numel(),
                     (const float*)lr_dev.data_ptr(), (float)momentum,
                     (float)dampening, (float)weight_decay, nesterov ? 1 : 0);
}
