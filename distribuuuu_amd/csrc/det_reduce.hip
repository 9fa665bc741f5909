// Deterministic mode (docs/DETERMINISM.md): the process-global switch and the
// ordered cross-block reduction that replaces fp32 atomics when it is on.
//
// In deterministic mode every kernel that used to atomicAdd its fp32 partial
// into a shared accumulator instead stores it, with plain vector stores, into
// its own slot of a workspace part[P][n] (P = colliding chunks/blocks, n =
// output elements). ordered_reduce then sums the P slots in ascending slot
// order — one fixed association, independent of block scheduling — applies
// `scale` and emits the output dtype directly (it also does the job of the
// fp32->bf16 cast pass, so the mode costs no extra pass over the output).
#include "common.h"

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace {

// exactly "1" turns it on — the same rule as the Python-side copy in
// ops/dispatch.py, so a box without the extension answers alike
std::atomic<int> g_det{[] {
  const char* e = getenv("DISTRIBUUUU_DETERMINISTIC");
  return (e && strcmp(e, "1") == 0) ? 1 : 0;
}()};

template <typename T>
DEV_INLINE void store4(T* out, float a, float b, float c, float d);
template <>
DEV_INLINE void store4<float>(float* out, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(out) = float4{a, b, c, d};
}
template <>
DEV_INLINE void store4<__hip_bfloat16>(__hip_bfloat16* out, float a, float b,
                                       float c, float d) {
  Pack<__hip_bfloat16, 4> o;
  o.v[0] = from_f32<__hip_bfloat16>(a);
  o.v[1] = from_f32<__hip_bfloat16>(b);
  o.v[2] = from_f32<__hip_bfloat16>(c);
  o.v[3] = from_f32<__hip_bfloat16>(d);
  *reinterpret_cast<uint2*>(out) = *reinterpret_cast<const uint2*>(&o);
}

// One thread per float4 of outputs (n % 4 == 0). Pure streaming: P*n*4 bytes
// in, 16-byte loads coalesced along i. The loads of U consecutive slots are
// issued together (they are independent); the ADDS stay strictly in slot
// order p = 0..P-1, which is what fixes the result.
template <typename Tout>
__global__ __launch_bounds__(256) void ordered_reduce_v4_kernel(
    const float* __restrict__ part, Tout* __restrict__ out, int P, int64_t n4,
    float scale) {
  constexpr int U = 8;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4* src = reinterpret_cast<const float4*>(part) + i;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  int p = 0;
  for (; p + U <= P; p += U) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[(int64_t)(p + u) * n4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc.x += v[u].x;
      acc.y += v[u].y;
      acc.z += v[u].z;
      acc.w += v[u].w;
    }
  }
  for (; p < P; ++p) {
    const float4 v = src[(int64_t)p * n4];
    acc.x += v.x;
    acc.y += v.y;
    acc.z += v.z;
    acc.w += v.w;
  }
  store4<Tout>(out + i * 4, acc.x * scale, acc.y * scale, acc.z * scale,
               acc.w * scale);
}

// One thread per output element: small outputs (more threads in flight than
// the float4 form would give) and n % 4 != 0. Loads are 4-byte but still
// coalesced along i (a wave reads 256 contiguous bytes per slot).
template <typename Tout>
__global__ __launch_bounds__(256) void ordered_reduce_v1_kernel(
    const float* __restrict__ part, Tout* __restrict__ out, int P, int64_t n,
    float scale) {
  constexpr int U = 8;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* src = part + i;
  float acc = 0.f;
  int p = 0;
  for (; p + U <= P; p += U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[(int64_t)(p + u) * n];
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u];
  }
  for (; p < P; ++p) acc += src[(int64_t)p * n];
  out[i] = from_f32<Tout>(acc * scale);
}

}  // namespace

void set_deterministic(bool on) { g_det.store(on ? 1 : 0); }
bool is_deterministic() { return g_det.load() != 0; }

template <typename Tout>
void ordered_reduce(const float* part, Tout* out, int P, int64_t n,
                    float scale) {
  if (n <= 0) return;
  // float4 form once it alone fills the machine (256 CUs x 4 blocks of 256
  // threads); below that the per-element form has 4x the threads in flight.
  const bool v4 = (n % 4 == 0) && n >= (int64_t)4 * 256 * 1024;
  if (v4) {
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL((ordered_reduce_v4_kernel<Tout>),
                       dim3((unsigned)ceil_div(n4, 256)), dim3(256), 0,
                       cur_stream(), part, out, P, n4, scale);
  } else {
    hipLaunchKernelGGL((ordered_reduce_v1_kernel<Tout>),
                       dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                       cur_stream(), part, out, P, n, scale);
  }
}

template void ordered_reduce<float>(const float*, float*, int, int64_t, float);
template void ordered_reduce<__hip_bfloat16>(const float*, __hip_bfloat16*,
                                             int, int64_t, float);
