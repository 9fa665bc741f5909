// Exact-fp32 LDS-tiled depthwise convolution for gfx950: fp32 NHWC, square
// 3x3 / 5x5, stride 1 or 2, pad <= R/2, C % 4 == 0 (dwconv_f32_route in
// dwconv_route.h decides; docs/ARCHITECTURE.md "Depthwise" has the design).
// Every product and sum is fp32 (FMA); nothing on the path is rounded to a
// narrower type, and set_fp32_precision does not reach it.
//
// Common layout. A pack is four fp32 channels, one 16-byte f4: what an LDS
// read returns is an operand, there is no unpack and no output rounding. A
// block of 256 threads works on a chunk of CP <= 8 packs (32 channels, one
// 128 B line per pixel). Thread t is (pack pk = t % CP, lane = t / CP), so a
// staging load is 16 B per thread and contiguous over the chunk in global
// memory, and the LDS word a thread touches is t * 16 B from its
// neighbour's. A patch is [rows][PW][CP] f4 with PW compile-time;
// out-of-image pixels are WRITTEN as zeros (LDS is recycled) and no load
// leaves the tensor. With 4 accumulators per output instead of 8 a thread
// owns strips twice as long as the bf16 kernels': 1x8 (stride 1, 16-wide
// tiles) or 1x4 outputs forward, two parity quads in the stride-2 data
// gradient, 1x4 pixels in the weight gradient. All tap loops are
// compile-time; the only runtime divisions decode a block or a strip.
#include "common.h"
#include "dwconv_route.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// fp32 math stays scalar (no packed-fp32 forms), as in depthwise_tile.hip
#define DWF_KERNEL \
  __global__ __launch_bounds__(DW_THREADS) __attribute__((target("no-packed-fp32-ops")))
#define DWF_DEV DEV_INLINE __attribute__((target("no-packed-fp32-ops")))

// Header helpers (__syncthreads, fmaf, make_float4) lack the target attribute
// and so would be CALLED, not inlined: builtins only in here.
// what __syncthreads() does
DWF_DEV void dwf_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// acc += a * b per channel, one rounding each
DWF_DEV void fma4(f4& acc, const f4& a, const f4& b) {
  acc.x = __builtin_fmaf(a.x, b.x, acc.x);
  acc.y = __builtin_fmaf(a.y, b.y, acc.y);
  acc.z = __builtin_fmaf(a.z, b.z, acc.z);
  acc.w = __builtin_fmaf(a.w, b.w, acc.w);
}

// Pins a finished accumulator in its registers. Without it the compiler
// sinks each output's FMA chain into that output's predicated store and
// keeps every staged operand of the strip alive until the last one (256
// VGPRs, or a kilobyte of scratch per lane under a cap).
DWF_DEV void pin(f4& v) { asm volatile("" : "+v"(v)); }

// Stage rows [h0, h0 + PH) x cols [w0, w0 + PW) of one image's pack column
// (src already points at the image and the pack) into lds[px * CP + pk].
// ok = false (image or pack past the end) stages zeros.
template <int PW>
DWF_DEV void stage_patch(f4* lds, const float* src, bool ok, int IH, int IW,
                         int C, int h0, int w0, int PH, int CP, int pk,
                         int lane, int nlanes) {
  for (int px = lane; px < PH * PW; px += nlanes) {
    const int row = px / PW, col = px - row * PW;
    const int h = h0 + row, w = w0 + col;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok && (unsigned)h < (unsigned)IH && (unsigned)w < (unsigned)IW)
      v = *reinterpret_cast<const f4*>(src + ((int64_t)h * IW + w) * C);
    lds[px * CP + pk] = v;
  }
}

// Chunk weights [C][R*R] -> LDS [tap][CP * 4] fp32 (an f4 per (tap, pack)),
// back to front when FLIP. Coalesced over the chunk's contiguous weights.
template <int RS, bool FLIP>
DWF_DEV void stage_weights(f4* wl, const float* w, int C, int c0, int CP) {
  float* dst = reinterpret_cast<float*>(wl);
  for (int i = threadIdx.x; i < CP * 4 * RS; i += DW_THREADS) {
    const int cl = i / RS, tap = i - cl * RS;
    const int c = c0 + cl;
    dst[(FLIP ? RS - 1 - tap : tap) * CP * 4 + cl] =
        c < C ? w[(int64_t)c * RS + tap] : 0.f;
  }
}

struct DwfBlock {
  int ck, tw, th, ng;
};

// grid order (image group, tile row, tile col, chunk)
DWF_DEV DwfBlock decode_block(int nchunk, int tilesW, int tilesH) {
  DwfBlock b;
  int i = blockIdx.x;
  b.ck = i % nchunk;
  i /= nchunk;
  b.tw = i % tilesW;
  i /= tilesW;
  b.th = i % tilesH;
  b.ng = i / tilesH;
  return b;
}

// ---------------------------------------------------------------------------
// forward, and stride-1 dgrad (FLIP, x = gy, ph/pw = R-1-pad)
// ---------------------------------------------------------------------------
// A thread owns a pack and 1 x SW strips of outputs (SW = TW / 2): per tap
// row it reads the strip's (SW-1)*STRIDE + R input packs once and feeds SW
// outputs. Accumulation per output is r-major then s-major.
template <int R, int STRIDE, int TW, bool FLIP>
DWF_KERNEL void dwf_fwd_kernel(const float* __restrict__ x,
                               const float* __restrict__ w,
                               float* __restrict__ y, int N, int IH, int IW,
                               int C, int OH, int OW, int ph, int pw, int TH,
                               int CP, int NB, int tilesH, int tilesW,
                               int nchunk) {
  constexpr int SW = TW / 2;
  constexpr int PW = (TW - 1) * STRIDE + R;
  constexpr int TWS = TW / SW;
  constexpr int XN = (SW - 1) * STRIDE + R;
  extern __shared__ f4 smem[];
  const int PH = (TH - 1) * STRIDE + R;
  f4* wl = smem;               // [R*R][CP]
  f4* xl = smem + R * R * CP;  // [NB][PH][PW][CP]
  const DwfBlock b = decode_block(nchunk, tilesW, tilesH);
  const int c0 = b.ck * CP * 4;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 4 < C;
  const int oh0 = b.th * TH, ow0 = b.tw * TW;

  stage_weights<R * R, FLIP>(wl, w, C, c0, CP);
  if (active) {
    for (int img = 0; img < NB; ++img) {
      const int n = b.ng * NB + img;
      const bool ok = ch_ok && n < N;
      const float* src = ok ? x + (int64_t)n * IH * IW * C + c0 + pk * 4 : x;
      stage_patch<PW>(xl + img * PH * PW * CP, src, ok, IH, IW, C,
                      oh0 * STRIDE - ph, ow0 * STRIDE - pw, PH, CP, pk, lane,
                      nlanes);
    }
  }
  dwf_sync();
  if (!active || !ch_ok) return;

  const int per = TH * TWS;
#pragma unroll 1
  for (int sidx = lane; sidx < NB * per; sidx += nlanes) {
    const int img = sidx / per, rem = sidx - img * per;
    const int oh = rem / TWS, os = (rem % TWS) * SW;
    const int n = b.ng * NB + img;
    if (n >= N || oh0 + oh >= OH || ow0 + os >= OW) continue;
    f4 acc[SW] = {};
    const f4* xp = xl + ((img * PH + oh * STRIDE) * PW + os * STRIDE) * CP + pk;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // one tap row of inputs and weights live at a time: hoisting all 25
      // weight packs of a 5x5 out of the strip loop costs 100 VGPRs
      asm volatile("" ::: "memory");
      f4 xf[XN];
#pragma unroll
      for (int i = 0; i < XN; ++i) xf[i] = xp[(r * PW + i) * CP];
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const f4 wv = wl[(r * R + s) * CP + pk];
#pragma unroll
        for (int o = 0; o < SW; ++o) fma4(acc[o], xf[o * STRIDE + s], wv);
      }
    }
#pragma unroll
    for (int o = 0; o < SW; ++o) pin(acc[o]);
    float* yp = y + (((int64_t)n * OH + oh0 + oh) * OW + ow0 + os) * C + c0 +
                pk * 4;
#pragma unroll
    for (int o = 0; o < SW; ++o)
      if (ow0 + os + o < OW)
        *reinterpret_cast<f4*>(yp + (int64_t)o * C) = acc[o];
  }
}

// ---------------------------------------------------------------------------
// stride-2 dgrad
// ---------------------------------------------------------------------------
// Over u = h + ph, v = w + pw a gx pixel is reached by the taps with
// r = u and s = v (mod 2), so the 2x2 quad (u, v) = (2a + du, 2b + dv) meets
// gy(a - i, b - j) * w(2i + du, 2j + dv): a compile-time tap list per quad
// member. A thread owns QS = 2 neighbouring quads of a row (2 x 4 pixels) and
// reads the QS + R/2 gy packs of a row once for both. The block stages
// QH + R/2 rows by DWF_QW + R/2 columns of gy (zero outside the map).
template <int R>
DWF_KERNEL void dwf_dgrad_s2_kernel(const float* __restrict__ gy,
                                    const float* __restrict__ w,
                                    float* __restrict__ gx, int N, int H,
                                    int W, int C, int Ho, int Wo, int ph,
                                    int pw, int QH, int CP, int tilesH,
                                    int tilesW, int nchunk) {
  constexpr int HL = R / 2;
  constexpr int QW = DWF_QW;
  constexpr int QS = 2;
  constexpr int PW = QW + HL;
  constexpr int XG = QS + HL;
  extern __shared__ f4 smem[];
  const int PH = QH + HL;
  f4* wl = smem;
  f4* gl = smem + R * R * CP;
  const DwfBlock b = decode_block(nchunk, tilesW, tilesH);
  const int n = b.ng;
  const int c0 = b.ck * CP * 4;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 4 < C;
  const int a0 = b.th * QH, b0 = b.tw * QW;

  stage_weights<R * R, false>(wl, w, C, c0, CP);
  if (active)
    stage_patch<PW>(gl,
                    ch_ok ? gy + (int64_t)n * Ho * Wo * C + c0 + pk * 4 : gy,
                    ch_ok, Ho, Wo, C, a0 - HL, b0 - HL, PH, CP, pk, lane,
                    nlanes);
  dwf_sync();
  if (!active || !ch_ok) return;

#pragma unroll 1
  for (int q = lane; q < QH * (QW / QS); q += nlanes) {
    const int a = q / (QW / QS), bq = (q % (QW / QS)) * QS;
    const int h0 = 2 * (a0 + a) - ph, w0 = 2 * (b0 + bq) - pw;
    if (h0 >= H || w0 >= W) continue;
    f4 acc[QS][2][2] = {};
#pragma unroll
    for (int i = 0; i <= HL; ++i) {
      asm volatile("" ::: "memory");  // one gy row and its weights at a time
      // g[c] = gy(a - i, bq + c - HL): quad k meets column j at c = k - j + HL
      f4 g[XG];
#pragma unroll
      for (int c = 0; c < XG; ++c)
        g[c] = gl[((a + HL - i) * PW + bq + c) * CP + pk];
#pragma unroll
      for (int j = 0; j <= HL; ++j) {
#pragma unroll
        for (int du = 0; du < 2; ++du) {
#pragma unroll
          for (int dv = 0; dv < 2; ++dv) {
            const int r = 2 * i + du, s = 2 * j + dv;
            if (r < R && s < R) {
              const f4 wv = wl[(r * R + s) * CP + pk];
#pragma unroll
              for (int k = 0; k < QS; ++k)
                fma4(acc[k][du][dv], g[k - j + HL], wv);
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < QS; ++k)
#pragma unroll
      for (int du = 0; du < 2; ++du)
#pragma unroll
        for (int dv = 0; dv < 2; ++dv) pin(acc[k][du][dv]);
#pragma unroll
    for (int k = 0; k < QS; ++k)
#pragma unroll
      for (int du = 0; du < 2; ++du)
#pragma unroll
        for (int dv = 0; dv < 2; ++dv) {
          const int h = h0 + du, w_ = w0 + 2 * k + dv;
          if (h >= 0 && h < H && w_ >= 0 && w_ < W)
            *reinterpret_cast<f4*>(gx + (((int64_t)n * H + h) * W + w_) * C +
                                   c0 + pk * 4) = acc[k][du][dv];
        }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: one pass over gy and x for all taps
// ---------------------------------------------------------------------------
// Block (chunk, slot) walks the slot's contiguous run of (image, tile) items.
// Per item it stages the x patch and the gy tile. A thread owns a pack and
// 1 x 4 pixel strips: per tap row it reads the strip's 3*STRIDE + R x packs
// once and feeds all R taps of the row from 4 pixels each, into R*R f4
// accumulators (36 or 100 VGPRs) that live across the run. At the end, one
// tap row at a time, every lane's partials meet in LDS and are summed in lane
// order; the sum goes into this slot of ws[slots][C*R*R] with plain stores.
// One writer per element and a fixed order: bit-reproducible.
template <int R, int STRIDE, int TW>
DWF_KERNEL void dwf_wgrad_kernel(const float* __restrict__ gy,
                                 const float* __restrict__ x,
                                 float* __restrict__ ws, int N, int H, int W,
                                 int C, int Ho, int Wo, int ph, int pw, int TH,
                                 int CP, int tilesH, int tilesW, int64_t per,
                                 int64_t items) {
  constexpr int WP = 4;
  constexpr int PW = (TW - 1) * STRIDE + R;
  constexpr int TWS = TW / WP;
  constexpr int XN = (WP - 1) * STRIDE + R;
  extern __shared__ f4 smem[];
  const int PH = (TH - 1) * STRIDE + R;
  f4* xl = smem;                 // [PH][PW][CP]
  f4* gl = smem + PH * PW * CP;  // [TH][TW][CP]
  const int ck = blockIdx.x, slot = blockIdx.y;
  const int c0 = ck * CP * 4;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 4 < C;

  f4 acc[R * R] = {};
  int64_t it1 = (int64_t)(slot + 1) * per;
  if (it1 > items) it1 = items;
  for (int64_t it = (int64_t)slot * per; it < it1; ++it) {
    const int tw = (int)(it % tilesW);
    const int64_t t2 = it / tilesW;
    const int th = (int)(t2 % tilesH);
    const int64_t n = t2 / tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    dwf_sync();  // the previous item's readers are done
    if (active) {
      stage_patch<PW>(xl, ch_ok ? x + n * H * W * C + c0 + pk * 4 : x, ch_ok,
                      H, W, C, oh0 * STRIDE - ph, ow0 * STRIDE - pw, PH, CP,
                      pk, lane, nlanes);
      stage_patch<TW>(gl, ch_ok ? gy + n * Ho * Wo * C + c0 + pk * 4 : gy,
                      ch_ok, Ho, Wo, C, oh0, ow0, TH, CP, pk, lane, nlanes);
    }
    dwf_sync();
    if (active && ch_ok) {
#pragma unroll 1
      for (int sidx = lane; sidx < TH * TWS; sidx += nlanes) {
        const int oh = sidx / TWS, os = (sidx % TWS) * WP;
        f4 g[WP];
#pragma unroll
        for (int k = 0; k < WP; ++k) g[k] = gl[(oh * TW + os + k) * CP + pk];
        const f4* xp = xl + (oh * STRIDE * PW + os * STRIDE) * CP + pk;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          f4 xf[XN];
#pragma unroll
          for (int i = 0; i < XN; ++i) xf[i] = xp[(r * PW + i) * CP];
#pragma unroll
          for (int s = 0; s < R; ++s)
#pragma unroll
            for (int k = 0; k < WP; ++k)
              fma4(acc[r * R + s], g[k], xf[k * STRIDE + s]);
        }
      }
    }
  }

  // red[lane][R][CP] f4: at most 256 threads x R x 16 B = dwf_red_bytes(R)
  float* red = reinterpret_cast<float*>(smem);
  const int row = R * CP * 4;
  float* wslot = ws + (int64_t)slot * C * R * R;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    dwf_sync();
    if (active) {
#pragma unroll
      for (int s = 0; s < R; ++s) smem[(lane * R + s) * CP + pk] = acc[r * R + s];
    }
    dwf_sync();
    for (int e = threadIdx.x; e < row; e += DW_THREADS) {
      float sum = 0.f;
      for (int pl = 0; pl < nlanes; ++pl) sum += red[pl * row + e];
      const int s = e / (CP * 4);
      const int c = c0 + e - s * CP * 4;
      if (c < C) wslot[(int64_t)c * R * R + r * R + s] = sum;
    }
  }
}

template <typename K, typename... A>
void dwf_launch(K kern, dim3 grid, int lds, A... args) {
  hipLaunchKernelGGL(kern, grid, dim3(DW_THREADS), lds, cur_stream(), args...);
}

DwPass pass_of(const std::string& pass) {
  TORCH_CHECK(pass == "fwd" || pass == "dgrad" || pass == "wgrad",
              "pass must be fwd, dgrad or wgrad, got ", pass);
  return pass == "fwd" ? DwPass::Fwd
                       : pass == "dgrad" ? DwPass::Dgrad : DwPass::Wgrad;
}

// the route of a pass over x [N, C, H, W], read off any fp32 NHWC operand t
DwRoute route_of(const at::Tensor& t, int64_t N, int64_t C, int64_t H,
                 int64_t W, int64_t R, int64_t S, int64_t sh, int64_t sw,
                 int64_t ph, int64_t pw, DwPass pass) {
  const bool ok = t.scalar_type() == at::kFloat && t.dim() == 4 &&
                  t.is_contiguous(at::MemoryFormat::ChannelsLast);
  return dwconv_f32_route(ok, N, C, H, W, (int)R, (int)S, (int)sh, (int)sw,
                          (int)ph, (int)pw, pass);
}

// an fp32 NHWC operand the kernels may read or write 16 bytes at a time
void check_operand(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  check_nhwc(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be fp32");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, name,
              " must be 16-byte aligned");
}

// w [C, 1, R, S] fp32, dense (contiguous and channels_last coincide)
void check_weight(const at::Tensor& w, int64_t C) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 &&
                  w.size(0) == C && w.size(1) == 1 &&
                  (w.is_contiguous() ||
                   w.is_contiguous(at::MemoryFormat::ChannelsLast)),
              "w must be a dense fp32 [C, 1, R, S] GPU tensor");
}

void launch_fwd(const DwRoute& rt, const at::Tensor& x, const at::Tensor& w,
                at::Tensor& y, int R, int st, int ph, int pw, bool flip) {
  const int N = x.size(0), C = x.size(1), IH = x.size(2), IW = x.size(3);
  const int OH = y.size(2), OW = y.size(3);
  const dim3 grid((unsigned)((int64_t)dw_ceil(N, rt.NB) * rt.tilesH *
                             rt.tilesW * rt.nchunk));
  auto go = [&](auto kern) {
    dwf_launch(kern, grid, rt.lds_bytes, x.data_ptr<float>(),
               w.data_ptr<float>(), y.data_ptr<float>(), N, IH, IW, C, OH, OW,
               ph, pw, rt.TH, rt.CP, rt.NB, rt.tilesH, rt.tilesW, rt.nchunk);
  };
  const int key = R * 1000 + st * 100 + rt.TW;
  if (flip) {
    switch (key) {
      case 3116: return go(dwf_fwd_kernel<3, 1, 16, true>);
      case 3108: return go(dwf_fwd_kernel<3, 1, 8, true>);
      case 5116: return go(dwf_fwd_kernel<5, 1, 16, true>);
      case 5108: return go(dwf_fwd_kernel<5, 1, 8, true>);
    }
  } else {
    switch (key) {
      case 3116: return go(dwf_fwd_kernel<3, 1, 16, false>);
      case 3108: return go(dwf_fwd_kernel<3, 1, 8, false>);
      case 5116: return go(dwf_fwd_kernel<5, 1, 16, false>);
      case 5108: return go(dwf_fwd_kernel<5, 1, 8, false>);
      case 3208: return go(dwf_fwd_kernel<3, 2, 8, false>);
      case 5208: return go(dwf_fwd_kernel<5, 2, 8, false>);
    }
  }
  TORCH_CHECK(false, "dwconv_f32: no forward kernel for R=", R, " stride=", st,
              " TW=", rt.TW, " flip=", flip);
}

}  // namespace

at::Tensor dwconv_f32_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                          int64_t ph, int64_t pw) {
  check_operand(x, "x");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  check_weight(w, C);
  const int64_t R = w.size(2), S = w.size(3);
  const DwRoute rt = route_of(x, N, C, H, W, R, S, sh, sw, ph, pw, DwPass::Fwd);
  TORCH_CHECK(rt.tiled, "dwconv_f32_fwd: outside the tiled fp32 range "
                        "(dwconv_f32_route answers generic)");
  auto y = at::empty({N, C, (H + 2 * ph - R) / sh + 1, (W + 2 * pw - S) / sw + 1},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  launch_fwd(rt, x, w, y, (int)R, (int)sh, (int)ph, (int)pw, false);
  return y;
}

at::Tensor dwconv_f32_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                            int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  check_operand(gy, "gy");
  const int64_t N = gy.size(0), C = gy.size(1);
  check_weight(w, C);
  const int64_t R = w.size(2), S = w.size(3);
  const DwRoute rt =
      route_of(gy, N, C, H, W, R, S, sh, sw, ph, pw, DwPass::Dgrad);
  TORCH_CHECK(rt.tiled, "dwconv_f32_dgrad: outside the tiled fp32 range "
                        "(dwconv_f32_route answers generic)");
  TORCH_CHECK(gy.size(2) == (H + 2 * ph - R) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - S) / sw + 1,
              "dwconv_f32_dgrad: gy does not match H x W and the geometry");
  auto gx = at::empty({N, C, H, W},
                      gy.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (sh == 1) {  // the forward machine over gy with the taps back to front
    launch_fwd(rt, gy, w, gx, (int)R, 1, (int)(R - 1 - ph), (int)(S - 1 - pw),
               true);
    return gx;
  }
  const dim3 grid(
      (unsigned)((int64_t)N * rt.tilesH * rt.tilesW * rt.nchunk));
  auto go = [&](auto kern) {
    dwf_launch(kern, grid, rt.lds_bytes, gy.data_ptr<float>(),
               w.data_ptr<float>(), gx.data_ptr<float>(), (int)N, (int)H,
               (int)W, (int)C, (int)gy.size(2), (int)gy.size(3), (int)ph,
               (int)pw, rt.TH / 2, rt.CP, rt.tilesH, rt.tilesW, rt.nchunk);
  };
  if (R == 3)
    go(dwf_dgrad_s2_kernel<3>);
  else
    go(dwf_dgrad_s2_kernel<5>);
  return gx;
}

at::Tensor dwconv_f32_wgrad(at::Tensor gy, at::Tensor x, int64_t R, int64_t S,
                            int64_t sh, int64_t sw, int64_t ph, int64_t pw) {
  check_operand(gy, "gy");
  check_operand(x, "x");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const DwRoute rt =
      route_of(x, N, C, H, W, R, S, sh, sw, ph, pw, DwPass::Wgrad);
  TORCH_CHECK(rt.tiled, "dwconv_f32_wgrad: outside the tiled fp32 range "
                        "(dwconv_f32_route answers generic)");
  TORCH_CHECK(gy.size(0) == N && gy.size(1) == C &&
                  gy.size(2) == (H + 2 * ph - R) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - S) / sw + 1,
              "dwconv_f32_wgrad: gy does not match x and the geometry");
  // one pass, one slot per block, summed in slot order: the same bits in
  // both determinism modes, so the flag is not read
  const int64_t n = C * R * S;
  auto ws = at::empty({(int64_t)rt.slots, n}, x.options());
  const int64_t items = N * rt.tilesH * rt.tilesW;
  const int64_t per = (items + rt.slots - 1) / rt.slots;
  const dim3 grid(rt.nchunk, rt.slots);
  auto go = [&](auto kern) {
    dwf_launch(kern, grid, rt.lds_bytes, gy.data_ptr<float>(),
               x.data_ptr<float>(), ws.data_ptr<float>(), (int)N, (int)H,
               (int)W, (int)C, (int)gy.size(2), (int)gy.size(3), (int)ph,
               (int)pw, rt.TH, rt.CP, rt.tilesH, rt.tilesW, per, items);
  };
  switch (R * 1000 + sh * 100 + rt.TW) {
    case 3116: go(dwf_wgrad_kernel<3, 1, 16>); break;
    case 3108: go(dwf_wgrad_kernel<3, 1, 8>); break;
    case 5116: go(dwf_wgrad_kernel<5, 1, 16>); break;
    case 5108: go(dwf_wgrad_kernel<5, 1, 8>); break;
    case 3208: go(dwf_wgrad_kernel<3, 2, 8>); break;
    case 5208: go(dwf_wgrad_kernel<5, 2, 8>); break;
    default:
      TORCH_CHECK(false, "dwconv_f32_wgrad: no kernel for R=", R, " stride=",
                  sh, " TW=", rt.TW);
  }
  auto gw = at::empty({C, 1, R, S}, x.options());
  ordered_reduce<float>(ws.data_ptr<float>(), gw.data_ptr<float>(), rt.slots,
                        n, 1.f);
  return gw;
}

// (route, TH, TW, CB, NB, slots, lds_bytes) of one pass ("fwd", "dgrad",
// "wgrad") over x [N, C, H, W]; classifies only, so meta tensors work.
std::tuple<std::string, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
dwconv_f32_route_py(at::Tensor x, int64_t R, int64_t S, int64_t sh, int64_t sw,
                    int64_t ph, int64_t pw, std::string pass) {
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  const DwRoute rt = route_of(x, x.size(0), x.size(1), x.size(2), x.size(3), R,
                              S, sh, sw, ph, pw, pass_of(pass));
  if (!rt.tiled) return {"generic", 0, 0, 0, 1, 0, 0};
  return {"tiled", rt.TH, rt.TW, rt.CP * 4, rt.NB, rt.slots, rt.lds_bytes};
}
