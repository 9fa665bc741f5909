// Fused multi-tensor SGD-momentum step.
// ONE kernel launch updates every parameter: a device-side chunk table
// (built once by the Python optimizer and cached across steps — no per-step
// host work, hipGraph-capturable) drives 256-thread blocks, each owning one
// 16K-element chunk. Momentum and master weights are fp32; bf16 params get
// w = master update then a bf16 store (fp32-master numerics).
//
// Table layout: int64 [nchunks, 6]:
//   [grad_ptr, param_ptr, mom_ptr, master_ptr, offset, count | flags<<32]
//   flags bit0: param bf16, bit1: grad bf16, bit2: momentum uninitialised
//   (first step of this parameter: the buffer is seeded with the gradient,
//   dampening not applied — torch.optim.SGD semantics)
#include "common.h"

namespace {

// Per-chunk update body shared by both kernels below: the only difference
// between them is where `lr` comes from, so they compile to the same
// arithmetic and give bit-identical results for the same rate.
DEV_INLINE void sgd_chunk(const long long* __restrict__ recs, float lr,
                          float mu, float damp, float wd, int nesterov) {
  const long long* rec = recs + (int64_t)blockIdx.x * 6;
  const void* grad = (const void*)rec[0];
  void* param = (void*)rec[1];
  float* mom = (float*)rec[2];
  float* master = (float*)rec[3];
  const int64_t off = rec[4];
  const int count = (int)(rec[5] & 0xffffffffll);
  const int flags = (int)(rec[5] >> 32);
  const bool p_bf16 = flags & 1, g_bf16 = flags & 2;
  const float gscale = (flags & 4) ? 1.f : 1.f - damp;
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int64_t j = off + i;
    float g = g_bf16 ? to_f32(((const __hip_bfloat16*)grad)[j])
                     : ((const float*)grad)[j];
    float w = master[j];
    if (wd != 0.f) g += wd * w;
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

__global__ void sgd_kernel(const long long* __restrict__ recs, float lr,
                           float mu, float damp, float wd, int nesterov) {
  sgd_chunk(recs, lr, mu, damp, wd, nesterov);
}

// Learning rate read from device memory (one load per thread, before the
// element loop): a captured hipGraph follows the schedule instead of freezing
// the rate it was captured with.
__global__ void sgd_kernel_dev(const long long* __restrict__ recs,
                               const float* __restrict__ lr_dev, float mu,
                               float damp, float wd, int nesterov) {
  const float lr = *lr_dev;
  sgd_chunk(recs, lr, mu, damp, wd, nesterov);
}

}  // namespace

void sgd_step(at::Tensor table, double lr, double momentum, double dampening,
              double weight_decay, bool nesterov) {
  CHECK_GPU(table);
  TORCH_CHECK(table.scalar_type() == at::kLong && table.size(1) == 6,
              "sgd table must be int64 [n, 6]");
  const int n = table.size(0);
  hipLaunchKernelGGL(sgd_kernel, dim3(n), dim3(256), 0, cur_stream(),
                     (const long long*)table.data_ptr(), (float)lr,
                     (float)momentum, (float)dampening, (float)weight_decay,
                     nesterov ? 1 : 0);
}

void sgd_step_dev(at::Tensor table, at::Tensor lr_dev, double momentum,
                  double dampening, double weight_decay, bool nesterov) {
  CHECK_GPU(table);
  CHECK_GPU(lr_dev);
  TORCH_CHECK(table.scalar_type() == at::kLong && table.size(1) == 6,
              "sgd table must be int64 [n, 6]");
  TORCH_CHECK(lr_dev.scalar_type() == at::kFloat && lr_dev.numel() == 1,
              "sgd_step_dev: lr must be a float32 tensor of one element");
  const int n = table.size(0);
  hipLaunchKernelGGL(sgd_kernel_dev, dim3(n), dim3(256), 0, cur_stream(),
                     (const long long*)table.data_ptr(),
                     (const float*)lr_dev.data_ptr(), (float)momentum,
                     (float)dampening, (float)weight_decay, nesterov ? 1 : 0);
}
