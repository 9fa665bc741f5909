// Exact-fp32 LDS-tiled MFMA kernels for narrow-group 3x3 convolutions on
// gfx950: fp32 NHWC, Cg == Kg == w in {4, 8, 16, 32}, stride 1 or 2, pad <= 1
// (gconv_f32_route in gconv_route.h decides; docs/ARCHITECTURE.md
// "Narrow-group conv, fp32" has the design). Every product and sum is fp32 on
// v_mfma_f32_16x16x4_f32; nothing on the path is rounded to a narrower type,
// and set_fp32_precision does not reach it.
//
// Common layout. A block of 256 threads works on a chunk of CW = 32 or 64
// channels. The LDS image of a pixel is CW floats plus 16 bytes of padding:
// 36 or 68 dwords. Sixteen lanes one pixel apart, each reading 16 bytes, start
// 4 * (9 i mod 16) or 4 * (i mod 16) dwords apart and cover the 64 banks once.
// At stride 2 the patch keeps its even and its odd columns in two halves, so
// the lanes of a tap are one LDS pixel apart there too. Out-of-image pixels
// and channels past C are WRITTEN as zeros on every tile (LDS is recycled) and
// no load leaves the tensor.
//
// MFMA operands (lane = 16 * kq + il): A row il, B column il, k = kq, one
// float each; D column il, rows 4 kq .. + 4.
//
// Forward / data gradient. The weight is the A operand and the pixels are B,
// so a lane ends up with four consecutive channels of one pixel: the result
// is stored as 16 bytes per lane with no restaging. A lane reads 16 bytes
// (channels 4 kq .. + 4 of a 16-channel block of one tap) once and feeds four
// MFMAs: sub-step j multiplies channel 4 kq + j on both sides, which only
// permutes the order of the fp32 sum. A wave owns one 16-channel column tile
// and keeps its 9 (w = 32: 18) weight fragments in registers for the run.
//
// Weight gradient. The reduction index is the pixel and each lane supplies
// ONE float per operand, so the pixel-major LDS images are read as they are,
// with no transposing pass: lane (il, kq) of k-step p reads channel il of
// tile pixel p + 4 kq. The sixteen il lanes read consecutive dwords and the
// four pixels p, p + 4, p + 8, p + 12 start 0, 16, 32, 48 banks apart
// (36 * 4 = 144 and 68 * 4 = 272 are both 16 mod 64), so a read covers the 64
// banks once. The bank arguments are reasoned, no counter run was taken.
#include "common.h"
#include "gconv_route.h"

// packed fp32 math (v_pk_*_f32) is kept out of this file's kernels. Header
// helpers lack the attribute and would be called, not inlined: builtins only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// what __syncthreads() does
DEV_INLINE void gcf_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

DEV_INLINE f4 gcf_mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// LDS column of patch column c, and the LDS pixel offset of tap t = 3 r + s
// from the patch pixel of an output's tap 0
template <int STRIDE>
DEV_INLINE constexpr int gcf_col(int c) {
  return STRIDE == 1 ? c : (c & 1) * 17 + (c >> 1);
}
template <int STRIDE>
DEV_INLINE constexpr int gcf_tap(int t) {
  return (t / 3) * (STRIDE == 1 ? 18 : 34) + gcf_col<STRIDE>(t % 3);
}

struct GcfItem {
  int n, th, tw;
};
// an item index is split once per block; the run then steps
DEV_INLINE GcfItem gcf_decode(int it, int tilesH, int tilesW) {
  GcfItem i;
  i.tw = it % tilesW;
  const int t2 = it / tilesW;
  i.th = t2 % tilesH;
  i.n = t2 / tilesH;
  return i;
}
DEV_INLINE void gcf_next(GcfItem& i, int tilesH, int tilesW) {
  if (++i.tw == tilesW) {
    i.tw = 0;
    if (++i.th == tilesH) i.th = 0, ++i.n;
  }
}

// Stage PH rows x (15 * STRIDE + 3) columns of image `src` [IH][IW][C] from
// (u0, v0) into the chunk's LDS patch, 16 bytes per thread. DILATE: (u, v)
// are coordinates of the zero-inserted canvas of a stride-2 gy, src pixel
// (u / 2, v / 2) where both are even and zeros elsewhere.
template <int STRIDE, bool DILATE>
DEV_INLINE void gcf_stage_patch(float* lds, const float* src, int IH, int IW,
                                int C, int c0, int CW, int u0, int v0,
                                int PH) {
  constexpr int PW = 15 * STRIDE + 3, PWP = STRIDE == 1 ? 18 : 34;
  const int lpk = CW == 64 ? 4 : 3;  // log2 of the packs of a pixel
  const int pk = threadIdx.x & ((1 << lpk) - 1);
  const int pitch = CW + GCF_PAD;
  const bool ch_ok = c0 + pk * 4 < C;
  for (int px = threadIdx.x >> lpk; px < PH * PW; px += GC_THREADS >> lpk) {
    const int row = px / PW, col = px - row * PW;
    int u = u0 + row, v = v0 + col;
    bool ok = ch_ok;
    if constexpr (DILATE) {
      ok = ok && u >= 0 && v >= 0 && ((u | v) & 1) == 0;
      u >>= 1, v >>= 1;
    }
    ok = ok && (unsigned)u < (unsigned)IH && (unsigned)v < (unsigned)IW;
    f4 val = {0.f, 0.f, 0.f, 0.f};
    if (ok)
      val = *reinterpret_cast<const f4*>(src + ((int64_t)u * IW + v) * C + c0 +
                                         pk * 4);
    *reinterpret_cast<f4*>(lds + (row * PWP + gcf_col<STRIDE>(col)) * pitch +
                           pk * 4) = val;
  }
}

// Weight fragment of the 16 output channels ct0 .. + 16 for tap t (w = 32:
// half h of the group's input channels), from the raw [K][9][w] weight:
// element j is input channel kl = 4 kq + j of the tile's 16-channel block,
// live where that channel and row il share a group, a literal zero elsewhere.
// FLIP builds the data gradient's operand [n = ci][tap, ko] =
// w[g w + ko][8 - tap][ci] by element gathers.
template <bool W32, bool FLIP>
DEV_INLINE f4 gcf_build_w(const float* wt, int C, int lw, int ct0, int t,
                          int h, int il, int kq) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  const int col = ct0 + il, kl = 4 * kq;
  if (col < C && (W32 || (kl >> lw) == (il >> lw))) {
    if constexpr (FLIP) {
      const int ci = col & ((1 << lw) - 1);
      const int ko = (W32 ? (ct0 & ~31) + 16 * h : ct0) + kl;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = wt[(((int64_t)(ko + j) * 9 + 8 - t) << lw) + ci];
    } else {
      const int off = W32 ? 16 * h + kl : (kl & ((1 << lw) - 1));
      v = *reinterpret_cast<const f4*>(wt + (((int64_t)col * 9 + t) << lw) +
                                       off);
    }
  }
  return v;
}

struct GcfParams {
  const float* x;  // the staged operand [N, IH, IW, C] (dgrad: gy)
  const float* w;  // raw weight [K][3][3][w]
  float* y;        // [N, OH, OW, C]
  float* part;     // EMIT: [gridDim.y][2 * C] BN sum / sum-of-squares rows
  int N, IH, IW, C, OH, OW;
  int oy, ox;  // patch origin of output (0, 0): -pad (dgrad: pad - 2)
  int lw;      // log2 of the group width
  int TH, CW, tilesH, tilesW, per, items;
};

// ---------------------------------------------------------------------------
// forward, and the data gradient (FLIP; DILATE for stride 2)
// ---------------------------------------------------------------------------
// grid (chunk, slot). Wave wv is pinned to the 16-channel tile nt of the
// chunk and walks the tile's pixel rows rw, rw + nrw, ...: the 16 pixels of
// one output row are the MFMA's columns. MFMAs per 16 x 16 output tile: 36
// (w = 32: 72) against an ideal 9 w / 4: the zero-filled fragments of w = 4
// and w = 8 spend three quarters and half of them on zeros.
template <bool W32, int STRIDE, bool FLIP, bool DILATE, bool EMIT>
__global__ __launch_bounds__(GC_THREADS) void gconv_f32_kernel(GcfParams p) {
  constexpr int PWP = STRIDE == 1 ? 18 : 34;
  constexpr int NH = W32 ? 2 : 1;
  extern __shared__ f4 gcf_smem[];
  float* lds = reinterpret_cast<float*>(gcf_smem);
  const int pitch = p.CW + GCF_PAD;
  const int PH = (p.TH - 1) * STRIDE + 3;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int lnt = p.CW == 64 ? 2 : 1;  // log2 of the chunk's 16-channel tiles
  const int nt = wv & ((1 << lnt) - 1), rw = wv >> lnt, nrw = 4 >> lnt;
  const int c0 = blockIdx.x * p.CW;
  const int ct0 = c0 + nt * 16;

  f4 Wf[9][NH];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int h = 0; h < NH; ++h)
      Wf[t][h] = gcf_build_w<W32, FLIP>(p.w, p.C, p.lw, ct0, t, h, il, kq);

  // this lane's pixel operand: pixel il of the row, 4 channels of its quad
  const int b_lane = il * pitch + (W32 ? (nt & ~1) : nt) * 16 + kq * 4;
  const int ech = ct0 + kq * 4;  // the lane's four output channels
  float ps[4] = {0.f, 0.f, 0.f, 0.f}, pq[4] = {0.f, 0.f, 0.f, 0.f};

  int it = blockIdx.y * p.per;
  const int it1 = it + p.per < p.items ? it + p.per : p.items;
  GcfItem item = gcf_decode(it, p.tilesH, p.tilesW);
  for (; it < it1; ++it, gcf_next(item, p.tilesH, p.tilesW)) {
    const int oh0 = item.th * p.TH, ow0 = item.tw * GC_TW;
    gcf_sync();  // the previous item's readers are done
    gcf_stage_patch<STRIDE, DILATE>(
        lds, p.x + (int64_t)item.n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, c0,
        p.CW, oh0 * STRIDE + p.oy, ow0 * STRIDE + p.ox, PH);
    gcf_sync();
    for (int row = rw; row < p.TH && oh0 + row < p.OH; row += nrw) {
      const float* bp = lds + row * STRIDE * PWP * pitch + b_lane;
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          const f4 xv = *reinterpret_cast<const f4*>(
              bp + gcf_tap<STRIDE>(t) * pitch + h * 16);
          acc = gcf_mfma(Wf[t][h][0], xv[0], acc);
          acc = gcf_mfma(Wf[t][h][1], xv[1], acc);
          acc = gcf_mfma(Wf[t][h][2], xv[2], acc);
          acc = gcf_mfma(Wf[t][h][3], xv[3], acc);
        }
      if (ow0 + il < p.OW && ech < p.C) {
        *reinterpret_cast<f4*>(
            p.y + (((int64_t)item.n * p.OH + oh0 + row) * p.OW + ow0 + il) *
                      p.C + ech) = acc;
        if constexpr (EMIT) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            ps[rr] += acc[rr];
            pq[rr] = __builtin_fmaf(acc[rr], acc[rr], pq[rr]);
          }
        }
      }
    }
  }

  if constexpr (EMIT) {
    // the block's row of the partial tensor: per channel the lanes' sums in
    // (row walker, pixel lane) order, one plain store each
    gcf_sync();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      lds[threadIdx.x * 8 + rr] = ps[rr];
      lds[threadIdx.x * 8 + 4 + rr] = pq[rr];
    }
    gcf_sync();
    const int c = threadIdx.x;
    if (c < p.CW && c0 + c < p.C) {
      float s = 0.f, q = 0.f;
      for (int r = 0; r < nrw; ++r)
        for (int i = 0; i < 16; ++i) {
          const int t = (((r << lnt) + (c >> 4)) * 4 + ((c >> 2) & 3)) * 16 + i;
          s += lds[t * 8 + (c & 3)];
          q += lds[t * 8 + 4 + (c & 3)];
        }
      float* prow = p.part + (int64_t)blockIdx.y * 2 * p.C;
      prow[c0 + c] = s;
      prow[p.C + c0 + c] = q;
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: one pass over gy and x for all nine taps
// ---------------------------------------------------------------------------
struct GwfParams {
  const float* gy;  // [N, Ho, Wo, C]
  const float* x;   // [N, H, W, C]
  float* ws;        // [gridDim.y << split][C * 9 * w]
  int N, H, W, C, Ho, Wo, ph, pw, lw;
  int TH, CW, tilesH, tilesW, per, items;
};

// grid (chunk, slot): the block walks the slot's run of (image, tile) items
// and stages the x patch and the gy tile of each. A k-step is four pixels of
// a tile row. Wave unit un owns the 16 gy channels un * 16 .. of the chunk
// (w = 32: one ko half of a group) and their group's x channels; per tap one
// MFMA per 16 x channels into its own accumulator, the gy value shared by the
// nine taps, a tap being an address offset. With two units (CW = 32) the wave
// pairs split the tile rows and each pair writes a workspace slot of its own,
// so nothing is merged in the block. The diagonal w x w blocks go to the slot
// with plain stores: one writer per element, a fixed order.
template <bool W32, int STRIDE>
__global__ __launch_bounds__(GC_THREADS) void gconv_f32_wgrad_kernel(
    GwfParams p) {
  constexpr int PWP = STRIDE == 1 ? 18 : 34;
  constexpr int NX = W32 ? 2 : 1;
  extern __shared__ f4 gcf_smem[];
  float* lds = reinterpret_cast<float*>(gcf_smem);
  const int pitch = p.CW + GCF_PAD;
  const int PH = (p.TH - 1) * STRIDE + 3;
  float* gl = lds + PH * PWP * pitch;  // [TH][16] pixels of gy
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int split = gcf_wgrad_split(p.CW);
  const int lnu = 2 - split;  // log2 of the units: 2 or 4 of them
  const int un = wv & ((1 << lnu) - 1), ks = wv >> lnu, nks = 1 << split;
  const int c0 = blockIdx.x * p.CW;
  const int lpk = p.CW == 64 ? 4 : 3;

  // k = kq of k-step q is tile pixel q + 4 kq
  const int g_lane = kq * 4 * pitch + un * 16 + il;
  const int x_lane = kq * 4 * pitch + (W32 ? (un & ~1) : un) * 16 + il;

  f4 acc[NX][9];
#pragma unroll
  for (int xt = 0; xt < NX; ++xt)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[xt][t] = f4{0.f, 0.f, 0.f, 0.f};

  int it = blockIdx.y * p.per;
  const int it1 = it + p.per < p.items ? it + p.per : p.items;
  GcfItem item = gcf_decode(it, p.tilesH, p.tilesW);
  for (; it < it1; ++it, gcf_next(item, p.tilesH, p.tilesW)) {
    const int oh0 = item.th * p.TH, ow0 = item.tw * GC_TW;
    gcf_sync();  // the previous item's readers are done
    gcf_stage_patch<STRIDE, false>(
        lds, p.x + (int64_t)item.n * p.H * p.W * p.C, p.H, p.W, p.C, c0, p.CW,
        oh0 * STRIDE - p.ph, ow0 * STRIDE - p.pw, PH);
    {
      const float* src = p.gy + (int64_t)item.n * p.Ho * p.Wo * p.C;
      const int pk = threadIdx.x & ((1 << lpk) - 1);
      for (int px = threadIdx.x >> lpk; px < p.TH * GC_TW;
           px += GC_THREADS >> lpk) {
        const int oh = oh0 + (px >> 4), ow = ow0 + (px & 15);
        f4 val = {0.f, 0.f, 0.f, 0.f};
        if (oh < p.Ho && ow < p.Wo && c0 + pk * 4 < p.C)
          val = *reinterpret_cast<const f4*>(
              src + ((int64_t)oh * p.Wo + ow) * p.C + c0 + pk * 4);
        *reinterpret_cast<f4*>(gl + px * pitch + pk * 4) = val;
      }
    }
    gcf_sync();
    for (int row = ks; row < p.TH && oh0 + row < p.Ho; row += nks) {
      const float* gp = gl + row * GC_TW * pitch + g_lane;
      const float* xp = lds + row * STRIDE * PWP * pitch + x_lane;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gv = gp[q * pitch];
#pragma unroll
        for (int xt = 0; xt < NX; ++xt)
#pragma unroll
          for (int t = 0; t < 9; ++t)
            acc[xt][t] = gcf_mfma(
                xp[(q + gcf_tap<STRIDE>(t)) * pitch + xt * 16], gv,
                acc[xt][t]);
      }
    }
  }

  // D row 4 kq + rr is the x channel, column il the gy channel
  float* wslot = p.ws + (((int64_t)blockIdx.y << split) + ks) * p.C *
                            (9 << p.lw);
  const int k = c0 + un * 16 + il;
  if (k < p.C) {
#pragma unroll
    for (int xt = 0; xt < NX; ++xt)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ct = kq * 4 + rr;
          if (W32 || (ct >> p.lw) == (il >> p.lw))
            wslot[(((int64_t)k * 9 + t) << p.lw) +
                  (W32 ? xt * 16 + ct : ct & ((1 << p.lw) - 1))] =
                acc[xt][t][rr];
        }
  }
}

int gcf_lw(int64_t gw) { return gw == 4 ? 2 : gw == 8 ? 3 : gw == 16 ? 4 : 5; }

GcfParams gcf_params(const GcRoute& rt, const at::Tensor& x,
                     const at::Tensor& w, at::Tensor& y, int oy, int ox) {
  GcfParams p{};
  p.x = x.data_ptr<float>();
  p.w = w.data_ptr<float>();
  p.y = y.data_ptr<float>();
  p.N = x.size(0), p.C = x.size(1), p.IH = x.size(2), p.IW = x.size(3);
  p.OH = y.size(2), p.OW = y.size(3);
  p.oy = oy, p.ox = ox;
  p.lw = gcf_lw(w.size(1));
  p.TH = rt.TH, p.CW = rt.CW, p.tilesH = rt.tilesH, p.tilesW = rt.tilesW;
  p.per = rt.per, p.items = (int)(x.size(0) * rt.tilesH * rt.tilesW);
  return p;
}

template <typename K, typename P>
void gcf_launch(K kern, const GcRoute& rt, const P& p) {
  hipLaunchKernelGGL(kern, dim3(rt.nchunk, rt.slots), dim3(GC_THREADS),
                     rt.lds_bytes, cur_stream(), p);
}

// Forward over x [N, C, H, W] into y; part != nullptr: the [rt.slots][2 C]
// BN partial rows as well.
void gcf_fwd(const GcRoute& rt, const at::Tensor& x, const at::Tensor& w,
             at::Tensor& y, int st, int ph, int pw, float* part) {
  GcfParams p = gcf_params(rt, x, w, y, -ph, -pw);
  p.part = part;
  const int key = (p.lw == 5) * 4 + (st == 2) * 2 + (part != nullptr);
  switch (key) {
    case 0: return gcf_launch(gconv_f32_kernel<false, 1, false, false, false>, rt, p);
    case 1: return gcf_launch(gconv_f32_kernel<false, 1, false, false, true>, rt, p);
    case 2: return gcf_launch(gconv_f32_kernel<false, 2, false, false, false>, rt, p);
    case 3: return gcf_launch(gconv_f32_kernel<false, 2, false, false, true>, rt, p);
    case 4: return gcf_launch(gconv_f32_kernel<true, 1, false, false, false>, rt, p);
    case 5: return gcf_launch(gconv_f32_kernel<true, 1, false, false, true>, rt, p);
    case 6: return gcf_launch(gconv_f32_kernel<true, 2, false, false, false>, rt, p);
    case 7: return gcf_launch(gconv_f32_kernel<true, 2, false, false, true>, rt, p);
  }
}

GcRoute gcf_route_of(const at::Tensor& t, int64_t C, int64_t K, int64_t H,
                     int64_t W, int64_t groups, int64_t R, int64_t S,
                     int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                     int64_t dh, int64_t dw, GcPass pass) {
  const bool ok = t.scalar_type() == at::kFloat && t.dim() == 4 &&
                  t.is_contiguous(at::MemoryFormat::ChannelsLast);
  return gconv_f32_route(ok, t.size(0), C, K, H, W, groups, (int)R, (int)S,
                         (int)sh, (int)sw, (int)ph, (int)pw, (int)dh, (int)dw,
                         pass);
}

// staging and weight loads are 16-byte vector loads from data_ptr()
void gcf_check_aligned(const at::Tensor& t, const char* who,
                       const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, ": ",
              name, " must start 16-byte aligned");
}

void gcf_check_weight(const at::Tensor& w, int64_t C, int64_t groups,
                      const char* who) {
  CHECK_GPU(w);
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.dim() == 4 &&
                  w.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  w.size(0) == C && w.size(1) * groups == C &&
                  w.size(2) == 3 && w.size(3) == 3,
              who, ": weight must be fp32 channels_last [C, C/groups, 3, 3], "
              "got ", w.sizes());
  gcf_check_aligned(w, who, "weight");
}

std::tuple<at::Tensor, at::Tensor> gcf_forward(at::Tensor x, at::Tensor w,
                                               int64_t sh, int64_t sw,
                                               int64_t ph, int64_t pw,
                                               int64_t groups, bool emit) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "gconv_f32_fwd: 4-D operands");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const GcRoute rt =
      gcf_route_of(x, C, w.size(0), H, W, groups, w.size(2), w.size(3), sh, sw,
                   ph, pw, 1, 1, GcPass::Fwd);
  TORCH_CHECK(rt.tile,
              "gconv_f32_fwd: outside the tiled range (gconv_f32_route)");
  gcf_check_weight(w, C, groups, "gconv_f32_fwd");
  gcf_check_aligned(x, "gconv_f32_fwd", "x");
  const int64_t Ho = (H + 2 * ph - 3) / sh + 1, Wo = (W + 2 * pw - 3) / sw + 1;
  auto y = at::empty({N, C, Ho, Wo},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor part;
  if (emit) part = at::empty({(int64_t)rt.slots, 2 * C}, x.options());
  gcf_fwd(rt, x, w, y, (int)sh, (int)ph, (int)pw,
          emit ? part.data_ptr<float>() : nullptr);
  return {y, part};
}

}  // namespace

at::Tensor gconv_f32_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                         int64_t ph, int64_t pw, int64_t groups) {
  return std::get<0>(gcf_forward(x, w, sh, sw, ph, pw, groups, false));
}

// -> (y, part [blocks, 2 K] fp32): batch_norm_act's _bn_partials format
std::tuple<at::Tensor, at::Tensor> gconv_f32_fwd_bn(at::Tensor x, at::Tensor w,
                                                    int64_t sh, int64_t sw,
                                                    int64_t ph, int64_t pw,
                                                    int64_t groups) {
  return gcf_forward(x, w, sh, sw, ph, pw, groups, true);
}

// The forward machine over gy with the flipped operand and pad' = 2 - pad;
// stride 2 stages gy's zero-inserted canvas.
at::Tensor gconv_f32_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                           int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                           int64_t groups) {
  CHECK_GPU(gy);
  TORCH_CHECK(gy.dim() == 4 && w.dim() == 4, "gconv_f32_dgrad: 4-D operands");
  const int64_t N = gy.size(0), C = gy.size(1);
  const GcRoute rt =
      gcf_route_of(gy, C, w.size(0), H, W, groups, w.size(2), w.size(3), sh,
                   sw, ph, pw, 1, 1, GcPass::Dgrad);
  TORCH_CHECK(rt.tile && gy.size(2) == (H + 2 * ph - 3) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - 3) / sw + 1,
              "gconv_f32_dgrad: outside the tiled range (gconv_f32_route)");
  gcf_check_weight(w, C, groups, "gconv_f32_dgrad");
  gcf_check_aligned(gy, "gconv_f32_dgrad", "gy");
  auto gx = at::empty({N, C, H, W},
                      gy.options().memory_format(at::MemoryFormat::ChannelsLast));
  const GcfParams p = gcf_params(rt, gy, w, gx, (int)ph - 2, (int)pw - 2);
  const bool w32 = p.lw == 5;
  if (sh == 1) {
    if (w32)
      gcf_launch(gconv_f32_kernel<true, 1, true, false, false>, rt, p);
    else
      gcf_launch(gconv_f32_kernel<false, 1, true, false, false>, rt, p);
  } else if (w32) {
    gcf_launch(gconv_f32_kernel<true, 1, true, true, false>, rt, p);
  } else {
    gcf_launch(gconv_f32_kernel<false, 1, true, true, false>, rt, p);
  }
  return gx;
}

// The gradient in the shape and strides conv2d_wgrad returns.
at::Tensor gconv_f32_wgrad(at::Tensor gy, at::Tensor x, int64_t sh, int64_t sw,
                           int64_t ph, int64_t pw, int64_t groups) {
  CHECK_GPU(gy);
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 4 && gy.dim() == 4, "gconv_f32_wgrad: 4-D operands");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const GcRoute rt = gcf_route_of(x, C, gy.size(1), H, W, groups, 3, 3, sh, sw,
                                  ph, pw, 1, 1, GcPass::Wgrad);
  TORCH_CHECK(rt.tile && gy.scalar_type() == at::kFloat &&
                  gy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  gy.size(0) == N &&
                  gy.size(2) == (H + 2 * ph - 3) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - 3) / sw + 1,
              "gconv_f32_wgrad: outside the tiled range (gconv_f32_route)");
  gcf_check_aligned(x, "gconv_f32_wgrad", "x");
  gcf_check_aligned(gy, "gconv_f32_wgrad", "gy");
  const int64_t gw_ = C / groups, n = C * 9 * gw_;
  // one slot per wave group of a block, summed in slot order: the same bits
  // in both determinism modes, so the flag is not read
  const int64_t rows = (int64_t)rt.slots << gcf_wgrad_split(rt.CW);
  auto ws = at::empty({rows, n}, x.options());
  GwfParams p{};
  p.gy = gy.data_ptr<float>();
  p.x = x.data_ptr<float>();
  p.ws = ws.data_ptr<float>();
  p.N = N, p.C = C, p.H = H, p.W = W;
  p.Ho = gy.size(2), p.Wo = gy.size(3);
  p.ph = ph, p.pw = pw;
  p.lw = gcf_lw(gw_);
  p.TH = rt.TH, p.CW = rt.CW, p.tilesH = rt.tilesH, p.tilesW = rt.tilesW;
  p.per = rt.per, p.items = (int)(N * rt.tilesH * rt.tilesW);
  const bool w32 = p.lw == 5;
  if (sh == 1) {
    if (w32)
      gcf_launch(gconv_f32_wgrad_kernel<true, 1>, rt, p);
    else
      gcf_launch(gconv_f32_wgrad_kernel<false, 1>, rt, p);
  } else if (w32) {
    gcf_launch(gconv_f32_wgrad_kernel<true, 2>, rt, p);
  } else {
    gcf_launch(gconv_f32_wgrad_kernel<false, 2>, rt, p);
  }
  auto gw = at::empty({C, gw_, 3, 3},
                      x.options().memory_format(at::MemoryFormat::ChannelsLast));
  ordered_reduce<float>(ws.data_ptr<float>(), gw.data_ptr<float>(), (int)rows,
                        n, 1.f);
  return gw;
}

// (route, TH, chunk width, chunks, items per block, blocks per chunk,
// lds_bytes) of one pass ("fwd", "dgrad", "wgrad") over x [N, C, H, W] with a
// [K, C / groups, R, S] weight; classifies only, so meta tensors work.
std::tuple<std::string, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
gconv_f32_route_py(at::Tensor x, int64_t K, int64_t groups, int64_t R,
                   int64_t S, int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                   int64_t dh, int64_t dw, std::string pass) {
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  TORCH_CHECK(pass == "fwd" || pass == "dgrad" || pass == "wgrad",
              "pass must be fwd, dgrad or wgrad, got ", pass);
  TORCH_CHECK(groups >= 1, "groups must be positive");
  const GcPass p = pass == "fwd"     ? GcPass::Fwd
                   : pass == "dgrad" ? GcPass::Dgrad
                                     : GcPass::Wgrad;
  const GcRoute rt = gcf_route_of(x, x.size(1), K, x.size(2), x.size(3),
                                  groups, R, S, sh, sw, ph, pw, dh, dw, p);
  if (!rt.tile) return {"generic", 0, 0, 0, 0, 0, 0};
  return {"tile", rt.TH, rt.CW, rt.nchunk, rt.per, rt.slots, rt.lds_bytes};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
