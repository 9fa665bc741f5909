// Dense-block slab kernels: DenseNet's concat-free forward and backward.
//
// A dense block's features live in ONE NHWC buffer, the slab [N, Ctot, H, W]:
// layer i reads the channel prefix [0, cin_i) with row pitch Ctot and appends
// its g new channels behind it. A channel's batch statistics do not depend on
// which layer normalises it, so sum / sum-of-squares are formed once, by the
// append that writes the channel, and every later norm1 only finalizes.
//
//   dense_append : y [rows, g] -> slab[:, c_off:c_off+g] (+ per-block sum /
//                  sumsq partials -> column reduce into sums[2, Ctot])
//   dense_bn_fwd : finalize(sums[:, :cin]) -> mean/rstd/scale/shift (+ running
//                  update), then y = relu(slab[:, :cin]*scale + shift), dense
//   dense_bn_bwd : reduce sum(g'), sum(g'*x) -> finalize gw, gb, (P1, P2, P3)
//                  -> gslab[:, :cin] += P1*g' + P3*x + P2 (read-modify-write)
//   dense_take   : gslab[:, c_off:c_off+g] -> dense [rows, g]
//
// Thread mapping (all row-walk kernels): a 256-thread block owns a band of
// rows; thread t -> (pack column t % ncp, row lane t / ncp), so the dense
// side of every copy is read or written fully contiguously even when a row is
// only a few packs (g = 32 bf16 is four). Each thread keeps its pack column,
// loads the per-channel tables once, and walks rows with two pointers that
// advance by constants - one per pitch. fp32 math, no atomics; reductions are
// per-block partial rows plus a column reduction, so results repeat bit for
// bit. Packs are 16 bytes: Ctot, cin, c_off and g are multiples of the pack
// width, which keeps every pack at any channel offset 16-byte aligned.
#include "common.h"

// packed fp32 math (v_pk_*_f32) is kept out of this file's kernels
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

DEV_INLINE int p2_floor(int v) { return 1 << (31 - __builtin_clz(v)); }

// (pack column, row lane) of this thread and the block's row band
struct RowWalk {
  int ncp, nrl, cp0, rl;
  bool active;
  int64_t row0, row1;
};

DEV_INLINE RowWalk row_walk(int cpacks, int64_t rows, int64_t rows_per_block) {
  RowWalk w;
  w.ncp = min(cpacks, (int)blockDim.x);
  w.nrl = p2_floor(blockDim.x / w.ncp);
  w.cp0 = threadIdx.x % w.ncp;
  w.rl = threadIdx.x / w.ncp;
  w.active = w.rl < w.nrl;
  w.row0 = (int64_t)blockIdx.x * rows_per_block;
  w.row1 = min(w.row0 + rows_per_block, rows);
  return w;
}

// LDS tree over the row lanes of one pack column; row lane 0 then stores the
// block's partial row part[blockIdx.x, 0:C] (a) and [C:2C] (b). `valid` masks
// the ragged last pass of the multi-column loop; every thread of the block
// calls this the same number of times.
template <int V>
DEV_INLINE void block_partial_store(float* red, const RowWalk& w, bool valid,
                                    int cp, int C, const float (&a)[V],
                                    const float (&b)[V],
                                    float* __restrict__ part) {
  float* slot = &red[(w.rl * w.ncp + w.cp0) * 2 * V];
  if (valid) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      slot[j] = a[j];
      slot[V + j] = b[j];
    }
  }
  __syncthreads();
  for (int st = w.nrl >> 1; st > 0; st >>= 1) {
    if (valid && w.rl < st) {
      const float* other = &red[((w.rl + st) * w.ncp + w.cp0) * 2 * V];
#pragma unroll
      for (int j = 0; j < 2 * V; ++j) slot[j] += other[j];
    }
    __syncthreads();
  }
  if (valid && w.rl == 0) {
    float* prow = part + (int64_t)blockIdx.x * 2 * C + cp * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      prow[j] = slot[j];
      prow[C + j] = slot[V + j];
    }
  }
  __syncthreads();
}

// ---- append / take: pitched pack copy, optionally with sum / sumsq ---------
// src and dst point at the first channel of the copied range; pitches are in
// packs. append: src = y (pitch g/V), dst = slab + c_off (pitch Ctot/V);
// take: the reverse.
template <typename T, bool SUMS>
__global__ __launch_bounds__(256) void dense_copy_kernel(
    const T* __restrict__ src, T* __restrict__ dst, float* __restrict__ part,
    int64_t rows, int g, int src_pitch, int dst_pitch,
    int64_t rows_per_block) {
  constexpr int V = 16 / sizeof(T);
  using P = Pack<T, V>;
  __shared__ float red[SUMS ? 256 * 2 * V : 1];
  const int gp = g / V;
  const RowWalk w = row_walk(gp, rows, rows_per_block);
  const P* sp = reinterpret_cast<const P*>(src);
  P* dp = reinterpret_cast<P*>(dst);
  for (int cb = 0; cb < gp; cb += w.ncp) {
    const int cp = cb + w.cp0;
    const bool valid = w.active && cp < gp;
    float acc[V] = {}, acc2[V] = {};
    if (valid) {
      int64_t r = w.row0 + w.rl;
      const int64_t sstep = (int64_t)w.nrl * src_pitch;
      const int64_t dstep = (int64_t)w.nrl * dst_pitch;
      const P* sq = sp + r * src_pitch + cp;
      P* dq = dp + r * dst_pitch + cp;
      for (; r + 3 * (int64_t)w.nrl < w.row1; r += 4 * (int64_t)w.nrl) {
        P pk[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pk[u] = sq[u * sstep];
        sq += 4 * sstep;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          dq[u * dstep] = pk[u];
          if (SUMS) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
              const float v = to_f32(pk[u].v[j]);
              acc[j] += v;
              acc2[j] += v * v;
            }
          }
        }
        dq += 4 * dstep;
      }
      for (; r < w.row1; r += w.nrl) {
        const P p = sq[0];
        sq += sstep;
        dq[0] = p;
        dq += dstep;
        if (SUMS) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float v = to_f32(p.v[j]);
            acc[j] += v;
            acc2[j] += v * v;
          }
        }
      }
    }
    if (SUMS) block_partial_store<V>(red, w, valid, cp, g, acc, acc2, part);
  }
}

// Column-reduce the append's partials [nblocks, 2g] into the slab's sums:
// sums[0, c_off + c] and sums[1, c_off + c]. 16 channels x 16 row lanes.
__global__ void dense_sums_reduce_kernel(const float* __restrict__ part,
                                         int nblocks, int g,
                                         float* __restrict__ sums, int ctot,
                                         int c_off) {
  __shared__ float red[512];
  const int ci = threadIdx.x & 15;
  const int rlane = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + ci;
  float s = 0.f, q = 0.f;
  if (c < g) {
    const float* p = part + (int64_t)rlane * 2 * g + c;
    const int64_t pstep = (int64_t)16 * 2 * g;
    int b = rlane;
    for (; b + 48 < nblocks; b += 64) {
      s += (p[0] + p[pstep]) + (p[2 * pstep] + p[3 * pstep]);
      q += (p[g] + p[pstep + g]) + (p[2 * pstep + g] + p[3 * pstep + g]);
      p += 4 * pstep;
    }
    for (; b < nblocks; b += 16) {
      s += p[0];
      q += p[g];
      p += pstep;
    }
  }
  red[threadIdx.x] = s;
  red[256 + threadIdx.x] = q;
  __syncthreads();
  if (rlane != 0 || c >= g) return;
#pragma unroll
  for (int t = 1; t < 16; ++t) {
    s += red[t * 16 + ci];
    q += red[256 + t * 16 + ci];
  }
  sums[c_off + c] = s;
  sums[ctot + c_off + c] = q;
}

// ---- forward finalize: sums[:, :cin] -> mean/rstd/scale/shift --------------
// Same formulas as bn.hip's bn_finalize_kernel (biased variance clamped at 0,
// unbiased into running_var); eval takes mean/var from the running buffers.
__global__ void dense_bn_finalize_kernel(
    const float* __restrict__ sums, int ctot, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ scale,
    float* __restrict__ shift, int cin, float inv_cnt, float unbias,
    float momentum, float eps, int training, int update_running) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cin) return;
  float m, r;
  if (training) {
    m = sums[c] * inv_cnt;
    float v = sums[ctot + c] * inv_cnt - m * m;
    v = fmaxf(v, 0.f);
    r = rsqrtf(v + eps);
    if (update_running) {
      running_mean[c] = running_mean[c] * (1.f - momentum) + m * momentum;
      running_var[c] =
          running_var[c] * (1.f - momentum) + v * unbias * momentum;
    }
  } else {
    m = running_mean[c];
    r = rsqrtf(running_var[c] + eps);
  }
  mean[c] = m;
  rstd[c] = r;
  const float sc = gamma[c] * r;
  scale[c] = sc;
  shift[c] = beta[c] - m * sc;
}

// ---- forward apply: y = relu(slab[:, :cin] * scale + shift), dense y -------
template <typename T>
__global__ __launch_bounds__(256, 2) void dense_bn_apply_kernel(
    const T* __restrict__ slab, const float* __restrict__ scale,
    const float* __restrict__ shift, T* __restrict__ y, int64_t rows, int cin,
    int slab_pitch, int64_t rows_per_block) {
  constexpr int V = 16 / sizeof(T);
  using P = Pack<T, V>;
  const int cpacks = cin / V;
  const RowWalk w = row_walk(cpacks, rows, rows_per_block);
  if (!w.active) return;
  const P* xp = reinterpret_cast<const P*>(slab);
  P* yp = reinterpret_cast<P*>(y);
  for (int cp = w.cp0; cp < cpacks; cp += w.ncp) {
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sc[j] = scale[cp * V + j];
      sh[j] = shift[cp * V + j];
    }
    int64_t row = w.row0 + w.rl;
    const int64_t xstep = (int64_t)w.nrl * slab_pitch;
    const int64_t ystep = (int64_t)w.nrl * cpacks;
    const P* xq = xp + row * slab_pitch + cp;
    P* yq = yp + row * cpacks + cp;
    for (; row + 3 * (int64_t)w.nrl < w.row1; row += 4 * (int64_t)w.nrl) {
      P px4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) px4[u] = xq[u * xstep];
      xq += 4 * xstep;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j)
          px4[u].v[j] =
              from_f32<T>(fmaxf(to_f32(px4[u].v[j]) * sc[j] + sh[j], 0.f));
        yq[u * ystep] = px4[u];
      }
      yq += 4 * ystep;
    }
    for (; row < w.row1; row += w.nrl) {
      P px = xq[0];
      xq += xstep;
#pragma unroll
      for (int j = 0; j < V; ++j)
        px.v[j] = from_f32<T>(fmaxf(to_f32(px.v[j]) * sc[j] + sh[j], 0.f));
      yq[0] = px;
      yq += ystep;
    }
  }
}

// ---- backward stage 1: per-block sum(g'), sum(g'*x) ------------------------
// g' = gy * [x*scale + shift > 0]: the relu mask is recomputed from x with
// the forward's own fp32 expression, so it matches the forward bit for bit.
template <typename T>
__global__ __launch_bounds__(256, 2) void dense_bn_bwd_reduce_kernel(
    const T* __restrict__ gy, const T* __restrict__ slab,
    const float* __restrict__ scale, const float* __restrict__ shift,
    float* __restrict__ part, int64_t rows, int cin, int slab_pitch,
    int64_t rows_per_block) {
  constexpr int V = 16 / sizeof(T);
  using P = Pack<T, V>;
  __shared__ float red[256 * 2 * V];
  const int cpacks = cin / V;
  const RowWalk w = row_walk(cpacks, rows, rows_per_block);
  const P* gp = reinterpret_cast<const P*>(gy);
  const P* xp = reinterpret_cast<const P*>(slab);
  for (int cb = 0; cb < cpacks; cb += w.ncp) {
    const int cp = cb + w.cp0;
    const bool valid = w.active && cp < cpacks;
    float accg[V] = {}, accgx[V] = {};
    if (valid) {
      float sc[V], sh[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sc[j] = scale[cp * V + j];
        sh[j] = shift[cp * V + j];
      }
      int64_t row = w.row0 + w.rl;
      const int64_t gstep = (int64_t)w.nrl * cpacks;
      const int64_t xstep = (int64_t)w.nrl * slab_pitch;
      const P* gq = gp + row * cpacks + cp;
      const P* xq = xp + row * slab_pitch + cp;
      for (; row + 3 * (int64_t)w.nrl < w.row1; row += 4 * (int64_t)w.nrl) {
        P pg4[4], px4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          pg4[u] = gq[u * gstep];
          px4[u] = xq[u * xstep];
        }
        gq += 4 * gstep;
        xq += 4 * xstep;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float xv = to_f32(px4[u].v[j]);
            const float g =
                xv * sc[j] + sh[j] > 0.f ? to_f32(pg4[u].v[j]) : 0.f;
            accg[j] += g;
            accgx[j] += g * xv;
          }
      }
      for (; row < w.row1; row += w.nrl) {
        const P pg = gq[0], px = xq[0];
        gq += gstep;
        xq += xstep;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xv = to_f32(px.v[j]);
          const float g = xv * sc[j] + sh[j] > 0.f ? to_f32(pg.v[j]) : 0.f;
          accg[j] += g;
          accgx[j] += g * xv;
        }
      }
    }
    block_partial_store<V>(red, w, valid, cp, cin, accg, accgx, part);
  }
}

// ---- backward finalize: partials -> gw, gb, coef = (P1, P2, P3) ------------
// sum_gxh = rstd*(sum(g'x) - mean*sum(g')); gw = sum_gxh, gb = sum(g')
// training: P1 = w*r; P3 = -w*r^2*sum_gxh/cnt; P2 = -P1*sum(g')/cnt - P3*mean
// eval: P1 = w*r; P2 = P3 = 0.
__global__ void dense_bn_bwd_finalize_kernel(
    const float* __restrict__ part, int nblocks,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, float* __restrict__ gw,
    float* __restrict__ gb, float* __restrict__ coef, int cin, float inv_cnt,
    int training) {
  __shared__ float red[512];
  const int ci = threadIdx.x & 15;
  const int rlane = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + ci;
  float sg = 0.f, sgx = 0.f;
  if (c < cin) {
    const float* p = part + (int64_t)rlane * 2 * cin + c;
    const int64_t pstep = (int64_t)16 * 2 * cin;
    int b = rlane;
    for (; b + 48 < nblocks; b += 64) {
      sg += (p[0] + p[pstep]) + (p[2 * pstep] + p[3 * pstep]);
      sgx += (p[cin] + p[pstep + cin]) +
             (p[2 * pstep + cin] + p[3 * pstep + cin]);
      p += 4 * pstep;
    }
    for (; b < nblocks; b += 16) {
      sg += p[0];
      sgx += p[cin];
      p += pstep;
    }
  }
  red[threadIdx.x] = sg;
  red[256 + threadIdx.x] = sgx;
  __syncthreads();
  if (rlane != 0 || c >= cin) return;
#pragma unroll
  for (int t = 1; t < 16; ++t) {
    sg += red[t * 16 + ci];
    sgx += red[256 + t * 16 + ci];
  }
  const float m = mean[c], r = rstd[c], wgt = gamma[c];
  const float sum_gxh = r * (sgx - m * sg);
  gw[c] = sum_gxh;
  gb[c] = sg;
  const float p1 = wgt * r;
  float p2 = 0.f, p3 = 0.f;
  if (training) {
    p3 = -wgt * r * r * sum_gxh * inv_cnt;
    p2 = -p1 * sg * inv_cnt - p3 * m;
  }
  coef[c] = p1;
  coef[cin + c] = p2;
  coef[2 * cin + c] = p3;
}

// ---- backward stage 2: gslab[:, :cin] += P1*g' + P3*x + P2 -----------------
// Read-modify-write on the gradient slab; the sum is formed in fp32 and
// rounded to T once. Each (row, pack) is owned by exactly one thread.
template <typename T>
__global__ __launch_bounds__(256, 2) void dense_bn_bwd_dx_kernel(
    const T* __restrict__ gy, const T* __restrict__ slab,
    const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ coef, T* __restrict__ gslab, int64_t rows,
    int cin, int slab_pitch, int gslab_pitch, int64_t rows_per_block) {
  constexpr int V = 16 / sizeof(T);
  using P = Pack<T, V>;
  const int cpacks = cin / V;
  const RowWalk w = row_walk(cpacks, rows, rows_per_block);
  if (!w.active) return;
  const P* gp = reinterpret_cast<const P*>(gy);
  const P* xp = reinterpret_cast<const P*>(slab);
  P* op = reinterpret_cast<P*>(gslab);
  for (int cp = w.cp0; cp < cpacks; cp += w.ncp) {
    float sc[V], sh[V], a1[V], a2[V], a3[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cc = cp * V + j;
      sc[j] = scale[cc];
      sh[j] = shift[cc];
      a1[j] = coef[cc];
      a2[j] = coef[cin + cc];
      a3[j] = coef[2 * cin + cc];
    }
    int64_t row = w.row0 + w.rl;
    const int64_t gstep = (int64_t)w.nrl * cpacks;
    const int64_t xstep = (int64_t)w.nrl * slab_pitch;
    const int64_t ostep = (int64_t)w.nrl * gslab_pitch;
    const P* gq = gp + row * cpacks + cp;
    const P* xq = xp + row * slab_pitch + cp;
    P* oq = op + row * gslab_pitch + cp;
    for (; row + 3 * (int64_t)w.nrl < w.row1; row += 4 * (int64_t)w.nrl) {
      P pg4[4], px4[4], po4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pg4[u] = gq[u * gstep];
        px4[u] = xq[u * xstep];
        po4[u] = oq[u * ostep];
      }
      gq += 4 * gstep;
      xq += 4 * xstep;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xv = to_f32(px4[u].v[j]);
          const float g =
              xv * sc[j] + sh[j] > 0.f ? to_f32(pg4[u].v[j]) : 0.f;
          po4[u].v[j] = from_f32<T>(to_f32(po4[u].v[j]) +
                                    (a1[j] * g + a3[j] * xv + a2[j]));
        }
        oq[u * ostep] = po4[u];
      }
      oq += 4 * ostep;
    }
    for (; row < w.row1; row += w.nrl) {
      const P pg = gq[0], px = xq[0];
      P po = oq[0];
      gq += gstep;
      xq += xstep;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float xv = to_f32(px.v[j]);
        const float g = xv * sc[j] + sh[j] > 0.f ? to_f32(pg.v[j]) : 0.f;
        po.v[j] = from_f32<T>(to_f32(po.v[j]) +
                              (a1[j] * g + a3[j] * xv + a2[j]));
      }
      oq[0] = po;
      oq += ostep;
    }
  }
}

// ---- host side --------------------------------------------------------------
// Row band per block: about 512 blocks (the bn.hip stage-1 budget), a whole
// number of row-lane sweeps, and of 4-deep unrolled sweeps once a band is
// that long.
int64_t band_rows(int64_t rows, int cpacks) {
  const int nrl = std::max(256 / std::min(cpacks, 256), 1);
  int64_t rpb = std::max<int64_t>(ceil_div(rows, 512), nrl);
  const int unit = rpb >= 4 * nrl ? 4 * nrl : nrl;
  return ceil_div(rpb, unit) * unit;
}

template <typename scalar_t>
int pack_of() { return 16 / (int)sizeof(scalar_t); }

void check_slab(const at::Tensor& slab, const char* name) {
  CHECK_GPU(slab);
  check_nhwc(slab, name);
  TORCH_CHECK(slab.storage_offset() * slab.element_size() % 16 == 0, name,
              " must be 16-byte aligned");
}

void check_range(const at::Tensor& slab, int64_t c_off, int64_t g, int V,
                 const char* what) {
  TORCH_CHECK(c_off >= 0 && g > 0 && c_off + g <= slab.size(1), what,
              ": channels [", c_off, ", ", c_off + g, ") outside the slab's ",
              slab.size(1));
  TORCH_CHECK(slab.size(1) % V == 0 && c_off % V == 0 && g % V == 0, what,
              ": Ctot, c_off and g must be multiples of ", V);
}

void check_vec(const at::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.numel() == n,
              name, " must be a contiguous fp32 GPU tensor of ", n,
              " elements");
}

template <typename scalar_t, bool SUMS>
void launch_copy(const scalar_t* src, scalar_t* dst, float* part,
                 int64_t rows, int g, int src_pitch, int dst_pitch,
                 int64_t rpb, int grid) {
  hipLaunchKernelGGL((dense_copy_kernel<scalar_t, SUMS>), dim3(grid),
                     dim3(256), 0, cur_stream(), src, dst, part, rows, g,
                     src_pitch, dst_pitch, rpb);
}

}  // namespace

// slab[:, c_off:c_off+g] = y; with `sums` ([2, Ctot] fp32) also
// sums[0, c_off:c_off+g] = sum(y), sums[1, ...] = sum(y*y) per channel.
void dense_append(at::Tensor slab, at::Tensor y, int64_t c_off,
                  c10::optional<at::Tensor> sums) {
  check_slab(slab, "slab");
  check_slab(y, "y");
  TORCH_CHECK(y.scalar_type() == slab.scalar_type() &&
                  y.size(0) == slab.size(0) && y.size(2) == slab.size(2) &&
                  y.size(3) == slab.size(3),
              "dense_append: y must match the slab's dtype, N, H and W");
  const int ctot = slab.size(1);
  const int g = y.size(1);
  const int64_t rows = slab.numel() / ctot;
  if (sums.has_value()) check_vec(*sums, 2 * (int64_t)ctot, "sums");
  DISPATCH_FLOAT_AND_BF16(slab.scalar_type(), "dense_append", [&] {
    const int V = pack_of<scalar_t>();
    check_range(slab, c_off, g, V, "dense_append");
    const int64_t rpb = band_rows(rows, g / V);
    const int grid = (int)ceil_div(rows, rpb);
    const scalar_t* src = (const scalar_t*)y.data_ptr();
    scalar_t* dst = (scalar_t*)slab.data_ptr() + c_off;
    if (sums.has_value()) {
      auto part = at::empty({grid, 2 * g}, sums->options());
      launch_copy<scalar_t, true>(src, dst, part.data_ptr<float>(), rows, g,
                                  g / V, ctot / V, rpb, grid);
      hipLaunchKernelGGL(dense_sums_reduce_kernel,
                         dim3((int)ceil_div(g, 16)), dim3(256), 0,
                         cur_stream(), part.data_ptr<float>(), grid, g,
                         sums->data_ptr<float>(), ctot, (int)c_off);
    } else {
      launch_copy<scalar_t, false>(src, dst, nullptr, rows, g, g / V,
                                   ctot / V, rpb, grid);
    }
  });
}

// dense NHWC copy of gslab[:, c_off:c_off+g]
at::Tensor dense_take(at::Tensor gslab, int64_t c_off, int64_t g) {
  check_slab(gslab, "gslab");
  const int ctot = gslab.size(1);
  const int64_t rows = gslab.numel() / ctot;
  auto out = at::empty({gslab.size(0), g, gslab.size(2), gslab.size(3)},
                       gslab.options().memory_format(
                           at::MemoryFormat::ChannelsLast));
  DISPATCH_FLOAT_AND_BF16(gslab.scalar_type(), "dense_take", [&] {
    const int V = pack_of<scalar_t>();
    check_range(gslab, c_off, g, V, "dense_take");
    const int64_t rpb = band_rows(rows, (int)g / V);
    const int grid = (int)ceil_div(rows, rpb);
    launch_copy<scalar_t, false>(
        (const scalar_t*)gslab.data_ptr() + c_off, (scalar_t*)out.data_ptr(),
        nullptr, rows, (int)g, ctot / V, (int)g / V, rpb, grid);
  });
  return out;
}

// norm1 of a dense layer on the slab prefix [0, cin): returns
// {y, mean, rstd, scale, shift}, y = relu(x*scale + shift) dense NHWC.
std::vector<at::Tensor> dense_bn_fwd(at::Tensor slab, int64_t cin,
                                     c10::optional<at::Tensor> sums,
                                     at::Tensor gamma, at::Tensor beta,
                                     c10::optional<at::Tensor> rm_opt,
                                     c10::optional<at::Tensor> rv_opt,
                                     double momentum, double eps,
                                     bool training) {
  check_slab(slab, "slab");
  const int ctot = slab.size(1);
  const int64_t rows = slab.numel() / ctot;
  check_vec(gamma, cin, "gamma");
  check_vec(beta, cin, "beta");
  const bool has_running = rm_opt.has_value() && rv_opt.has_value();
  if (has_running) {
    check_vec(*rm_opt, cin, "running_mean");
    check_vec(*rv_opt, cin, "running_var");
  }
  if (training) {
    TORCH_CHECK(sums.has_value(), "dense_bn_fwd: training needs the sums");
    check_vec(*sums, 2 * (int64_t)ctot, "sums");
  } else {
    TORCH_CHECK(has_running, "dense_bn_fwd: eval needs running statistics");
  }
  auto fopts = slab.options().dtype(at::kFloat).memory_format(
      at::MemoryFormat::Contiguous);
  auto stats = at::empty({4, cin}, fopts);
  auto mean = stats[0], rstd = stats[1], scale = stats[2], shift = stats[3];
  auto y = at::empty({slab.size(0), cin, slab.size(2), slab.size(3)},
                     slab.options().memory_format(
                         at::MemoryFormat::ChannelsLast));
  DISPATCH_FLOAT_AND_BF16(slab.scalar_type(), "dense_bn_fwd", [&] {
    const int V = pack_of<scalar_t>();
    check_range(slab, 0, cin, V, "dense_bn_fwd");
    auto stream = cur_stream();
    const float inv_cnt = 1.f / (float)rows;
    const float unbias = rows > 1 ? (float)rows / (float)(rows - 1) : 1.f;
    hipLaunchKernelGGL(
        dense_bn_finalize_kernel, dim3((int)ceil_div(cin, 256)), dim3(256), 0,
        stream, training ? sums->data_ptr<float>() : nullptr, ctot,
        gamma.data_ptr<float>(), beta.data_ptr<float>(),
        has_running ? rm_opt->data_ptr<float>() : nullptr,
        has_running ? rv_opt->data_ptr<float>() : nullptr,
        mean.data_ptr<float>(), rstd.data_ptr<float>(),
        scale.data_ptr<float>(), shift.data_ptr<float>(), (int)cin, inv_cnt,
        unbias, (float)momentum, (float)eps, training ? 1 : 0,
        has_running ? 1 : 0);
    const int cpacks = (int)cin / V;
    const int64_t rpb = band_rows(rows, cpacks);
    const int grid = (int)ceil_div(rows, rpb);
    hipLaunchKernelGGL((dense_bn_apply_kernel<scalar_t>), dim3(grid),
                       dim3(256), 0, stream,
                       (const scalar_t*)slab.data_ptr(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(),
                       (scalar_t*)y.data_ptr(), rows, (int)cin, ctot / V,
                       rpb);
  });
  return {y, mean, rstd, scale, shift};
}

// Backward of dense_bn_fwd: returns {gw, gb, coef[3, cin]} and, when gslab is
// given, accumulates the input gradient into gslab[:, :cin] in place. gslab
// may be narrower or wider than the slab; it only needs >= cin channels.
std::vector<at::Tensor> dense_bn_bwd(at::Tensor gy, at::Tensor slab,
                                     int64_t cin,
                                     c10::optional<at::Tensor> gslab,
                                     at::Tensor mean, at::Tensor rstd,
                                     at::Tensor gamma, at::Tensor scale,
                                     at::Tensor shift, bool training) {
  check_slab(slab, "slab");
  check_slab(gy, "gy");
  const int ctot = slab.size(1);
  const int64_t rows = slab.numel() / ctot;
  TORCH_CHECK(gy.scalar_type() == slab.scalar_type() &&
                  gy.size(0) == slab.size(0) && gy.size(1) == cin &&
                  gy.size(2) == slab.size(2) && gy.size(3) == slab.size(3),
              "dense_bn_bwd: gy must be [N, cin, H, W] of the slab's dtype");
  if (gslab.has_value()) {
    check_slab(*gslab, "gslab");
    TORCH_CHECK(gslab->scalar_type() == slab.scalar_type() &&
                    gslab->size(0) == slab.size(0) &&
                    gslab->size(2) == slab.size(2) &&
                    gslab->size(3) == slab.size(3) &&
                    gslab->data_ptr() != slab.data_ptr(),
                "dense_bn_bwd: gslab must match the slab's dtype, N, H, W");
  }
  check_vec(mean, cin, "mean");
  check_vec(rstd, cin, "rstd");
  check_vec(gamma, cin, "gamma");
  check_vec(scale, cin, "scale");
  check_vec(shift, cin, "shift");
  auto fopts = slab.options().dtype(at::kFloat).memory_format(
      at::MemoryFormat::Contiguous);
  auto gwb = at::empty({2, cin}, fopts);
  auto gw = gwb[0], gb = gwb[1];
  auto coef = at::empty({3, cin}, fopts);
  DISPATCH_FLOAT_AND_BF16(slab.scalar_type(), "dense_bn_bwd", [&] {
    const int V = pack_of<scalar_t>();
    check_range(slab, 0, cin, V, "dense_bn_bwd");
    if (gslab.has_value()) check_range(*gslab, 0, cin, V, "dense_bn_bwd");
    auto stream = cur_stream();
    const int cpacks = (int)cin / V;
    const int64_t rpb = band_rows(rows, cpacks);
    const int grid = (int)ceil_div(rows, rpb);
    auto part = at::empty({grid, 2 * cin}, fopts);
    hipLaunchKernelGGL((dense_bn_bwd_reduce_kernel<scalar_t>), dim3(grid),
                       dim3(256), 0, stream, (const scalar_t*)gy.data_ptr(),
                       (const scalar_t*)slab.data_ptr(),
                       scale.data_ptr<float>(), shift.data_ptr<float>(),
                       part.data_ptr<float>(), rows, (int)cin, ctot / V, rpb);
    hipLaunchKernelGGL(dense_bn_bwd_finalize_kernel,
                       dim3((int)ceil_div(cin, 16)), dim3(256), 0, stream,
                       part.data_ptr<float>(), grid, mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                       gw.data_ptr<float>(), gb.data_ptr<float>(),
                       coef.data_ptr<float>(), (int)cin, 1.f / (float)rows,
                       training ? 1 : 0);
    if (gslab.has_value())
      hipLaunchKernelGGL((dense_bn_bwd_dx_kernel<scalar_t>), dim3(grid),
                         dim3(256), 0, stream, (const scalar_t*)gy.data_ptr(),
                         (const scalar_t*)slab.data_ptr(),
                         scale.data_ptr<float>(), shift.data_ptr<float>(),
                         coef.data_ptr<float>(), (scalar_t*)gslab->data_ptr(),
                         rows, (int)cin, ctot / V, (int)gslab->size(1) / V,
                         rpb);
  });
  return {gw, gb, coef};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
