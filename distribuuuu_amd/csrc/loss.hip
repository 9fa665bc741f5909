// Cross-entropy loss and top-k accuracy (K15).
// ce_fwd: one block per row; block-reduce max, sum-exp; mean loss via one
// fp32 atomic per row (deterministic mode, docs/DETERMINISM.md: per-row
// losses stored to a [N] buffer and summed in row order by ordered_reduce).
// ce_bwd: gx = gl * (softmax - onehot) / N.
// ce_soft_fwd / ce_soft_bwd: the same two kernel bodies (SOFT template) on
// smoothed, batch-mixed targets; same [N, 2] pair, same deterministic mode.
// The forward hands the backward the row max m and log(sum exp(x - m)) as a
// PAIR ([N, 2]), never their sum: with logits near 100, m + log(sum) rounds at
// ulp(128) = 1.5e-5, a relative error of that size in every probability of
// the row (and a row of gradients that no longer sums to 0). Both kernels
// work on x - m, which is small where it matters.
#include "common.h"

namespace {

// SOFT: soft targets (label smoothing eps, batch mixed with its own reversal
// at weight lam), q[n, j] = (1-eps) * (lam*[j==a] + (1-lam)*[j==b]) + eps/K
// with a = target[n], b = target[N-1-n]:
//   row loss = ls - (1-eps) * (lam*z_a + (1-lam)*z_b) - (eps/K) * sum_j z_j
// on z = x - m, one more block reduction than the hard loss. lam is READ FROM
// MEMORY (a captured step follows a new lambda); lam_p == nullptr means
// lam = 1 and the partner target is never read. !SOFT is the hard-target
// kernel, unchanged to the bit.
template <bool DET, bool SOFT>
__global__ void ce_fwd_kernel(const float* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              const float* __restrict__ lam_p,
                              float* __restrict__ loss,
                              float* __restrict__ lse, int N, int K,
                              float one_m_eps, float eps_k) {
  __shared__ float lds[16];
  const int n = blockIdx.x;
  const float* row = logits + (int64_t)n * K;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < K; j += blockDim.x) m = fmaxf(m, row[j]);
  m = block_reduce_max<true>(m, lds);
  __syncthreads();
  float s = 0.f;
  float zs = 0.f;
  for (int j = threadIdx.x; j < K; j += blockDim.x) {
    const float z = row[j] - m;
    s += expf(z);
    if constexpr (SOFT) zs += z;
  }
  s = block_reduce_sum<true>(s, lds);
  if constexpr (SOFT) {
    __syncthreads();
    zs = block_reduce_sum<false>(zs, lds);
  }
  const float ls = logf(s);
  if (threadIdx.x == 0) {
    lse[2 * n] = m;
    lse[2 * n + 1] = ls;
    float v;
    if constexpr (SOFT) {
      float zt = row[target[n]] - m;
      if (lam_p != nullptr) {
        const float lam = lam_p[0];
        zt = lam * zt + (1.f - lam) * (row[target[N - 1 - n]] - m);
      }
      v = ls - one_m_eps * zt - eps_k * zs;
    } else {
      v = ls - (row[target[n]] - m);
    }
    // DET: loss is the [N] per-row buffer
    emit_partial<DET>(DET ? loss + n : loss, v / N);
  }
}

template <bool SOFT>
__global__ void ce_bwd_kernel(const float* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              const float* __restrict__ lam_p,
                              const float* __restrict__ lse,
                              const float* __restrict__ gl,
                              float* __restrict__ gx, int64_t total, int K,
                              float one_m_eps, float eps_k) {
  const float g = gl[0];
  const int64_t N = total / K;
  float lam = 1.f;
  if constexpr (SOFT) {
    if (lam_p != nullptr) lam = lam_p[0];
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / K;
    const int j = i % K;
    float p = expf((logits[i] - lse[2 * n]) - lse[2 * n + 1]);
    float t = (j == (int)target[n]) ? 1.f : 0.f;
    if constexpr (SOFT) {
      if (lam_p != nullptr) {
        const float tb = (j == (int)target[N - 1 - n]) ? 1.f : 0.f;
        t = lam * t + (1.f - lam) * tb;
      }
      t = one_m_eps * t + eps_k;
    }
    gx[i] = g * (p - t) / N;
  }
}

// top-k accuracy: per row, count how many of the top-maxk logits beat the
// target's logit (rank); correct@k when rank < k. One wave per row.
__global__ void topk_acc_kernel(const float* __restrict__ logits,
                                const int64_t* __restrict__ target,
                                int* __restrict__ correct1,
                                int* __restrict__ correctk, int N, int K,
                                int topk) {
  const int n = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (n >= N) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const float* row = logits + (int64_t)n * K;
  const float tv = row[target[n]];
  const int tj = (int)target[n];
  int rank = 0;  // number of entries strictly better than target
  for (int j = lane; j < K; j += WAVE) {
    float v = row[j];
    if (v > tv || (v == tv && j < tj)) ++rank;
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) rank += __shfl_down(rank, off);
  if (lane == 0) {
    if (rank == 0) atomicAdd(correct1, 1);
    if (rank < topk) atomicAdd(correctk, 1);
  }
}

}  // namespace

namespace {

template <bool SOFT>
std::vector<at::Tensor> ce_fwd_launch(const at::Tensor& logits,
                                      const at::Tensor& target,
                                      const float* lam_p, float one_m_eps,
                                      float eps_k) {
  const int N = logits.size(0), K = logits.size(1);
  auto lse = at::empty({N, 2}, logits.options());  // (max, log sum exp(x - max))
  if (is_deterministic()) {  // sampled per launch
    auto rowloss = at::empty({N}, logits.options());
    auto loss = at::empty({}, logits.options());
    hipLaunchKernelGGL((ce_fwd_kernel<true, SOFT>), dim3(N), dim3(256), 0,
                       cur_stream(), logits.data_ptr<float>(),
                       target.data_ptr<int64_t>(), lam_p,
                       rowloss.data_ptr<float>(), lse.data_ptr<float>(), N, K,
                       one_m_eps, eps_k);
    ordered_reduce<float>(rowloss.data_ptr<float>(), loss.data_ptr<float>(), N,
                          1, 1.f);
    return {loss, lse};
  }
  auto loss = at::zeros({}, logits.options());
  hipLaunchKernelGGL((ce_fwd_kernel<false, SOFT>), dim3(N), dim3(256), 0,
                     cur_stream(), logits.data_ptr<float>(),
                     target.data_ptr<int64_t>(), lam_p,
                     loss.data_ptr<float>(), lse.data_ptr<float>(), N, K,
                     one_m_eps, eps_k);
  return {loss, lse};
}

template <bool SOFT>
at::Tensor ce_bwd_launch(const at::Tensor& logits, const at::Tensor& target,
                         const float* lam_p, const at::Tensor& lse,
                         const at::Tensor& gl, float one_m_eps, float eps_k) {
  const int N = logits.size(0), K = logits.size(1);
  auto gx = at::empty_like(logits);
  int64_t total = (int64_t)N * K;
  hipLaunchKernelGGL((ce_bwd_kernel<SOFT>), dim3(grid_1d(total, 256)),
                     dim3(256), 0, cur_stream(), logits.data_ptr<float>(),
                     target.data_ptr<int64_t>(), lam_p, lse.data_ptr<float>(),
                     gl.data_ptr<float>(), gx.data_ptr<float>(), total, K,
                     one_m_eps, eps_k);
  return gx;
}

void check_lse(const at::Tensor& lse, int N, const char* who) {
  TORCH_CHECK(lse.dim() == 2 && lse.size(0) == N && lse.size(1) == 2 &&
                  lse.is_contiguous() && lse.scalar_type() == at::kFloat,
              who, ": lse must be the forward's [N, 2] (max, log-sum) pairs");
}

// Everything ce_soft_* dereference on the device, checked before any launch.
// Returns the lambda pointer (nullptr: lam = 1, partner target never read).
const float* check_soft(const at::Tensor& logits, const at::Tensor& target,
                        const c10::optional<at::Tensor>& lam, double eps,
                        const char* who) {
  CHECK_GPU(logits);
  TORCH_CHECK(logits.scalar_type() == at::kFloat && logits.dim() == 2 &&
                  logits.is_contiguous(),
              who, " expects contiguous fp32 [N, K] logits");
  TORCH_CHECK(logits.size(0) >= 1 && logits.size(1) >= 1, who,
              ": empty logits");
  TORCH_CHECK(target.is_cuda() && target.scalar_type() == at::kLong &&
                  target.is_contiguous() && target.numel() == logits.size(0),
              who, " expects N int64 targets on the GPU");
  TORCH_CHECK(eps >= 0.0 && eps < 1.0, who,
              ": label smoothing must be in [0, 1), got ", eps);
  if (!lam.has_value()) return nullptr;
  TORCH_CHECK(lam->is_cuda() && lam->scalar_type() == at::kFloat &&
                  lam->numel() == 1,
              who, ": lam must be a float32 GPU tensor of one element");
  return lam->data_ptr<float>();
}

}  // namespace

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target) {
  CHECK_GPU(logits);
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "ce_fwd expects fp32 logits");
  return ce_fwd_launch<false>(logits, target, nullptr, 1.f, 0.f);
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor gl) {
  CHECK_GPU(logits);
  check_lse(lse, logits.size(0), "ce_bwd");
  return ce_bwd_launch<false>(logits, target, nullptr, lse, gl, 1.f, 0.f);
}

// Soft-target pair: label smoothing eps (a launch argument, constant over a
// run) and the batch-reversal mix weight lam (a float32[1] device tensor the
// kernels read, so a replayed graph follows it; absent = 1).
std::vector<at::Tensor> ce_soft_fwd(at::Tensor logits, at::Tensor target,
                                    c10::optional<at::Tensor> lam,
                                    double eps) {
  const float* lam_p = check_soft(logits, target, lam, eps, "ce_soft_fwd");
  return ce_fwd_launch<true>(logits, target, lam_p, (float)(1.0 - eps),
                             (float)(eps / logits.size(1)));
}

at::Tensor ce_soft_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                       at::Tensor gl, c10::optional<at::Tensor> lam,
                       double eps) {
  const float* lam_p = check_soft(logits, target, lam, eps, "ce_soft_bwd");
  check_lse(lse, logits.size(0), "ce_soft_bwd");
  TORCH_CHECK(lse.is_cuda() && gl.is_cuda() &&
                  gl.scalar_type() == at::kFloat && gl.numel() == 1,
              "ce_soft_bwd: gl must be a float32 GPU tensor of one element");
  return ce_bwd_launch<true>(logits, target, lam_p, lse, gl,
                             (float)(1.0 - eps),
                             (float)(eps / logits.size(1)));
}

std::vector<at::Tensor> topk_acc(at::Tensor logits, at::Tensor target,
                                 int64_t topk) {
  CHECK_GPU(logits);
  auto lf = logits.scalar_type() == at::kFloat ? logits : logits.to(at::kFloat);
  const int N = lf.size(0), K = lf.size(1);
  auto c1 = at::zeros({1}, lf.options().dtype(at::kInt));
  auto ck = at::zeros({1}, lf.options().dtype(at::kInt));
  const int waves_per_block = 4;
  int grid = (int)ceil_div(N, waves_per_block);
  hipLaunchKernelGGL(topk_acc_kernel, dim3(grid), dim3(waves_per_block * WAVE),
                     0, cur_stream(), lf.data_ptr<float>(),
                     target.data_ptr<int64_t>(), c1.data_ptr<int>(),
                     ck.data_ptr<int>(), N, K, (int)topk);
  return {c1, ck};
}
