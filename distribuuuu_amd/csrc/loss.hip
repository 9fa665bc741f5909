// Cross-entropy loss and top-k accuracy (K15).
// ce_fwd: one block per row; block-reduce max, sum-exp; mean loss via one
// fp32 atomic per row (deterministic mode, docs/DETERMINISM.md: per-row
// losses stored to a [N] buffer and summed in row order by ordered_reduce).
// ce_bwd: gx = gl * (softmax - onehot) / N.
// The forward hands the backward the row max m and log(sum exp(x - m)) as a
// PAIR ([N, 2]), never their sum: with logits near 100, m + log(sum) rounds at
// ulp(128) = 1.5e-5, a relative error of that size in every probability of
// the row (and a row of gradients that no longer sums to 0). Both kernels
// work on x - m, which is small where it matters.
#include "common.h"

namespace {

template <bool DET>
__global__ void ce_fwd_kernel(const float* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              float* __restrict__ loss,
                              float* __restrict__ lse, int N, int K) {
  __shared__ float lds[16];
  const int n = blockIdx.x;
  const float* row = logits + (int64_t)n * K;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < K; j += blockDim.x) m = fmaxf(m, row[j]);
  m = block_reduce_max<true>(m, lds);
  __syncthreads();
  float s = 0.f;
  for (int j = threadIdx.x; j < K; j += blockDim.x) s += expf(row[j] - m);
  s = block_reduce_sum<true>(s, lds);
  const float ls = logf(s);
  if (threadIdx.x == 0) {
    lse[2 * n] = m;
    lse[2 * n + 1] = ls;
    // DET: loss is the [N] per-row buffer
    emit_partial<DET>(DET ? loss + n : loss, (ls - (row[target[n]] - m)) / N);
  }
}

__global__ void ce_bwd_kernel(const float* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ gl,
                              float* __restrict__ gx, int64_t total, int K) {
  const float g = gl[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / K;
    const int j = i % K;
    float p = expf((logits[i] - lse[2 * n]) - lse[2 * n + 1]);
    float t = (j == (int)target[n]) ? 1.f : 0.f;
    gx[i] = g * (p - t) / (total / K);
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

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target) {
  CHECK_GPU(logits);
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "ce_fwd expects fp32 logits");
  const int N = logits.size(0), K = logits.size(1);
  auto lse = at::empty({N, 2}, logits.options());  // (max, log sum exp(x - max))
  if (is_deterministic()) {  // sampled per launch
    auto rowloss = at::empty({N}, logits.options());
    auto loss = at::empty({}, logits.options());
    hipLaunchKernelGGL(ce_fwd_kernel<true>, dim3(N), dim3(256), 0,
                       cur_stream(), logits.data_ptr<float>(),
                       target.data_ptr<int64_t>(), rowloss.data_ptr<float>(),
                       lse.data_ptr<float>(), N, K);
    ordered_reduce<float>(rowloss.data_ptr<float>(), loss.data_ptr<float>(), N,
                          1, 1.f);
    return {loss, lse};
  }
  auto loss = at::zeros({}, logits.options());
  hipLaunchKernelGGL(ce_fwd_kernel<false>, dim3(N), dim3(256), 0,
                     cur_stream(), logits.data_ptr<float>(),
                     target.data_ptr<int64_t>(), loss.data_ptr<float>(),
                     lse.data_ptr<float>(), N, K);
  return {loss, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor gl) {
  CHECK_GPU(logits);
  const int N = logits.size(0), K = logits.size(1);
  TORCH_CHECK(lse.dim() == 2 && lse.size(0) == N && lse.size(1) == 2 &&
                  lse.is_contiguous() && lse.scalar_type() == at::kFloat,
              "ce_bwd: lse must be ce_fwd's [N, 2] (max, log-sum) pairs");
  auto gx = at::empty_like(logits);
  int64_t total = (int64_t)N * K;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid_1d(total, 256)), dim3(256), 0,
                     cur_stream(), logits.data_ptr<float>(),
                     target.data_ptr<int64_t>(), lse.data_ptr<float>(),
                     gl.data_ptr<float>(), gx.data_ptr<float>(), total, K);
  return gx;
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
