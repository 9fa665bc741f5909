// LDS-tiled depthwise convolution for gfx950: bf16 NHWC, square 3x3 / 5x5,
// stride 1 or 2, pad <= R/2 (dwconv_route.h decides; docs/ARCHITECTURE.md
// "Depthwise" has the design). A depthwise conv's only lever is spatial
// reuse, so every kernel here stages an input patch in LDS once and reads
// each tap from there.
//
// Common layout. A block of 256 threads works on a chunk of CP <= 8 packs of
// 8 channels. Thread t is (pack pk = t % CP, lane = t / CP): lanes run
// fastest over packs, so a staging load is 16 B per thread and contiguous
// over the chunk in global memory, and the LDS word a thread touches is
// t * 16 B from its neighbour's. A patch is [rows][PW][CP] uint4 with PW
// compile-time; out-of-image pixels are WRITTEN as zeros (LDS is recycled).
// All tap loops are compile-time; the only runtime divisions decode a block
// or a strip, never a tap.
#include "common.h"
#include "dwconv_route.h"

namespace {

using BF = __hip_bfloat16;

// fp32 adds and multiplies stay scalar: no packed-fp32 forms
#define DW_KERNEL \
  __global__ __launch_bounds__(DW_THREADS) __attribute__((target("no-packed-fp32-ops")))
#define DW_DEV DEV_INLINE __attribute__((target("no-packed-fp32-ops")))

// Header helpers (__syncthreads, __uint_as_float, __float2bfloat16, min) lack the target
// attribute and so would be CALLED, not inlined: builtins only in here.
// what __syncthreads() does
DW_DEV void dw_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

DW_DEV float bf_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
DW_DEV float bf_hi(unsigned u) {
  return __builtin_bit_cast(float, u & 0xffff0000u);
}

DW_DEV void unpack8(const uint4& u, float* f) {
  f[0] = bf_lo(u.x);
  f[1] = bf_hi(u.x);
  f[2] = bf_lo(u.y);
  f[3] = bf_hi(u.y);
  f[4] = bf_lo(u.z);
  f[5] = bf_hi(u.z);
  f[6] = bf_lo(u.w);
  f[7] = bf_hi(u.w);
}

// fp32 -> bf16 bits, round to nearest even; NaN stays a quiet NaN
DW_DEV unsigned bf_round(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the one rounding of an output: 8 fp32 -> one 16-byte bf16 pack
DW_DEV void store8(BF* dst, const float* f) {
  uint4 p;
  p.x = bf_round(f[0]) | (bf_round(f[1]) << 16);
  p.y = bf_round(f[2]) | (bf_round(f[3]) << 16);
  p.z = bf_round(f[4]) | (bf_round(f[5]) << 16);
  p.w = bf_round(f[6]) | (bf_round(f[7]) << 16);
  *reinterpret_cast<uint4*>(dst) = p;
}

// Stage rows [h0, h0 + PH) x cols [w0, w0 + PW) of one image's pack column
// (src already points at the image and the pack) into lds[px * CP + pk].
// ok = false (image or pack past the end) stages zeros.
template <int PW>
DW_DEV void stage_patch(uint4* lds, const BF* src, bool ok, int IH, int IW,
                        int C, int h0, int w0, int PH, int CP, int pk,
                        int lane, int nlanes) {
  for (int px = lane; px < PH * PW; px += nlanes) {
    const int row = px / PW, col = px - row * PW;
    const int h = h0 + row, w = w0 + col;
    uint4 v = {0u, 0u, 0u, 0u};
    if (ok && (unsigned)h < (unsigned)IH && (unsigned)w < (unsigned)IW)
      v = *reinterpret_cast<const uint4*>(src + ((int64_t)h * IW + w) * C);
    lds[px * CP + pk] = v;
  }
}

// Chunk weights [C][R*R] -> LDS [tap][CP * 8] bf16 (a uint4 per (tap, pack)),
// back to front when FLIP. Coalesced over the chunk's contiguous weights.
template <int RS, bool FLIP>
DW_DEV void stage_weights(uint4* wl, const BF* w, int C, int c0, int CP) {
  unsigned short* dst = reinterpret_cast<unsigned short*>(wl);
  const unsigned short* src = reinterpret_cast<const unsigned short*>(w);
  for (int i = threadIdx.x; i < CP * 8 * RS; i += DW_THREADS) {
    const int cl = i / RS, tap = i - cl * RS;
    const int c = c0 + cl;
    dst[(FLIP ? RS - 1 - tap : tap) * CP * 8 + cl] =
        c < C ? src[(int64_t)c * RS + tap] : (unsigned short)0;
  }
}

struct DwBlock {
  int ck, tw, th, ng;
};

// grid order (image group, tile row, tile col, chunk): a tile's chunks and an
// image's neighbouring tiles are adjacent blocks
DW_DEV DwBlock decode_block(int nchunk, int tilesW, int tilesH) {
  DwBlock b;
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
// A thread owns a pack and 1 x SW strips of outputs: per tap row it reads the
// (SW-1)*STRIDE + R input packs of the strip once and feeds SW outputs.
// Accumulation per output is r-major then s-major in fp32.
template <int R, int STRIDE, int TW, int SW, bool FLIP>
DW_KERNEL void dw_tile_fwd_kernel(const BF* __restrict__ x,
                                  const BF* __restrict__ w,
                                  BF* __restrict__ y, int N, int IH, int IW,
                                  int C, int OH, int OW, int ph, int pw,
                                  int TH, int CP, int NB, int tilesH,
                                  int tilesW, int nchunk) {
  constexpr int PW = (TW - 1) * STRIDE + R;
  constexpr int TWS = TW / SW;
  constexpr int XN = (SW - 1) * STRIDE + R;
  extern __shared__ uint4 smem[];
  const int PH = (TH - 1) * STRIDE + R;
  uint4* wl = smem;               // [R*R][CP]
  uint4* xl = smem + R * R * CP;  // [NB][PH][PW][CP]
  const DwBlock b = decode_block(nchunk, tilesW, tilesH);
  const int c0 = b.ck * CP * 8;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 8 < C;
  const int oh0 = b.th * TH, ow0 = b.tw * TW;

  stage_weights<R * R, FLIP>(wl, w, C, c0, CP);
  if (active) {
    for (int img = 0; img < NB; ++img) {
      const int n = b.ng * NB + img;
      const bool ok = ch_ok && n < N;
      const BF* src = ok ? x + (int64_t)n * IH * IW * C + c0 + pk * 8 : x;
      stage_patch<PW>(xl + img * PH * PW * CP, src, ok, IH, IW, C,
                      oh0 * STRIDE - ph, ow0 * STRIDE - pw, PH, CP, pk, lane,
                      nlanes);
    }
  }
  dw_sync();
  if (!active || !ch_ok) return;

  const int per = TH * TWS;
#pragma unroll 1
  for (int sidx = lane; sidx < NB * per; sidx += nlanes) {
    const int img = sidx / per, rem = sidx - img * per;
    const int oh = rem / TWS, os = (rem % TWS) * SW;
    const int n = b.ng * NB + img;
    if (n >= N || oh0 + oh >= OH || ow0 + os >= OW) continue;
    float acc[SW][8] = {};
    const uint4* xp =
        xl + ((img * PH + oh * STRIDE) * PW + os * STRIDE) * CP + pk;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // re-read this tap row's weights from LDS: hoisting all R*R unpacked
      // weight packs out of the strip loop costs 200 VGPRs for a 5x5
      asm volatile("" ::: "memory");
      float xf[XN][8];
#pragma unroll
      for (int i = 0; i < XN; ++i) unpack8(xp[(r * PW + i) * CP], xf[i]);
#pragma unroll
      for (int s = 0; s < R; ++s) {
        float wf[8];
        unpack8(wl[(r * R + s) * CP + pk], wf);
#pragma unroll
        for (int o = 0; o < SW; ++o)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            acc[o][j] += xf[o * STRIDE + s][j] * wf[j];
      }
    }
    BF* yp = y + (((int64_t)n * OH + oh0 + oh) * OW + ow0 + os) * C + c0 +
             pk * 8;
#pragma unroll
    for (int o = 0; o < SW; ++o)
      if (ow0 + os + o < OW) store8(yp + (int64_t)o * C, acc[o]);
  }
}

// ---------------------------------------------------------------------------
// stride-2 dgrad
// ---------------------------------------------------------------------------
// Over u = h + ph, v = w + pw a gx pixel is reached by the taps with
// r = u and s = v (mod 2), so a thread owns the 2x2 quad
// (u, v) = (2a + du, 2b + dv): gy(a - i, b - j) meets w(2i + du, 2j + dv), a
// compile-time list per quad member. The block stages QH + R/2 rows by
// 8 + R/2 columns of gy (zero outside the map).
template <int R>
DW_KERNEL void dw_tile_dgrad_s2_kernel(const BF* __restrict__ gy,
                                       const BF* __restrict__ w,
                                       BF* __restrict__ gx, int N, int H,
                                       int W, int C, int Ho, int Wo, int ph,
                                       int pw, int QH, int CP, int tilesH,
                                       int tilesW, int nchunk) {
  constexpr int HL = R / 2;
  constexpr int QW = 8;
  constexpr int PW = QW + HL;
  extern __shared__ uint4 smem[];
  const int PH = QH + HL;
  uint4* wl = smem;
  uint4* gl = smem + R * R * CP;
  const DwBlock b = decode_block(nchunk, tilesW, tilesH);
  const int n = b.ng;
  const int c0 = b.ck * CP * 8;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 8 < C;
  const int a0 = b.th * QH, b0 = b.tw * QW;

  stage_weights<R * R, false>(wl, w, C, c0, CP);
  if (active)
    stage_patch<PW>(gl,
                    ch_ok ? gy + (int64_t)n * Ho * Wo * C + c0 + pk * 8 : gy,
                    ch_ok, Ho, Wo, C, a0 - HL, b0 - HL, PH, CP, pk, lane,
                    nlanes);
  dw_sync();
  if (!active || !ch_ok) return;

#pragma unroll 1
  for (int q = lane; q < QH * QW; q += nlanes) {
    const int a = q / QW, bq = q % QW;
    const int h0 = 2 * (a0 + a) - ph, w0 = 2 * (b0 + bq) - pw;
    if (h0 >= H || w0 >= W) continue;
    float acc[2][2][8] = {};
#pragma unroll
    for (int i = 0; i <= HL; ++i) {
      asm volatile("" ::: "memory");  // weights re-read per gy row, as above
#pragma unroll
      for (int jx = 0; jx <= HL; ++jx) {
        float gf[8];
        unpack8(gl[((a + HL - i) * PW + (bq + HL - jx)) * CP + pk], gf);
#pragma unroll
        for (int du = 0; du < 2; ++du) {
#pragma unroll
          for (int dv = 0; dv < 2; ++dv) {
            const int r = 2 * i + du, s = 2 * jx + dv;
            if (r < R && s < R) {
              float wf[8];
              unpack8(wl[(r * R + s) * CP + pk], wf);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[du][dv][j] += gf[j] * wf[j];
            }
          }
        }
      }
    }
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int dv = 0; dv < 2; ++dv) {
        const int h = h0 + du, w_ = w0 + dv;
        if (h >= 0 && h < H && w_ >= 0 && w_ < W)
          store8(gx + (((int64_t)n * H + h) * W + w_) * C + c0 + pk * 8,
                 acc[du][dv]);
      }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: one pass over gy and x for all taps
// ---------------------------------------------------------------------------
// Block (chunk, slot) walks the slot's contiguous run of (image, tile) items.
// Per item it stages the x patch and the gy tile; a thread owns a pack and
// every nplanes-th pixel of the tile. 3x3: all 9 taps x 8 channels in fp32
// registers; 5x5: lanes also split over the tap row (G = 5), 5 x 8 each.
// Accumulators live across the run. At the end, per tap (5x5: per tap
// column), the pixel planes' partials meet in LDS and are summed in plane
// order; the sum goes into this slot of ws[slots][C*R*R] with plain stores.
// One writer per element and a fixed order: bit-reproducible.
template <int R, int STRIDE, int TW>
DW_KERNEL void dw_tile_wgrad_kernel(const BF* __restrict__ gy,
                                    const BF* __restrict__ x,
                                    float* __restrict__ ws, int N, int H,
                                    int W, int C, int Ho, int Wo, int ph,
                                    int pw, int TH, int CP, int tilesH,
                                    int tilesW, int64_t per, int64_t items) {
  constexpr int PW = (TW - 1) * STRIDE + R;
  constexpr int G = R == 5 ? 5 : 1;
  constexpr int NT = R == 5 ? 5 : 9;
  extern __shared__ uint4 smem[];
  const int PH = (TH - 1) * STRIDE + R;
  uint4* xl = smem;                 // [PH][PW][CP]
  uint4* gl = smem + PH * PW * CP;  // [TH][TW][CP]
  float* red = reinterpret_cast<float*>(smem);  // after the run
  const int ck = blockIdx.x, slot = blockIdx.y;
  const int c0 = ck * CP * 8;
  const int nlanes = DW_THREADS / CP;
  const int lane = threadIdx.x / CP, pk = threadIdx.x - lane * CP;
  const bool active = lane < nlanes;
  const bool ch_ok = c0 + pk * 8 < C;
  const int nplanes = nlanes / G;
  const int g = lane % G, plane = lane / G;
  const bool computes = active && plane < nplanes;

  float acc[NT][8] = {};
  int64_t it1 = (int64_t)(slot + 1) * per;
  if (it1 > items) it1 = items;
  for (int64_t it = (int64_t)slot * per; it < it1; ++it) {
    const int tw = (int)(it % tilesW);
    const int64_t t2 = it / tilesW;
    const int th = (int)(t2 % tilesH);
    const int64_t n = t2 / tilesH;
    const int oh0 = th * TH, ow0 = tw * TW;
    dw_sync();  // the previous item's readers are done
    if (active) {
      stage_patch<PW>(xl, ch_ok ? x + n * H * W * C + c0 + pk * 8 : x, ch_ok,
                      H, W, C, oh0 * STRIDE - ph, ow0 * STRIDE - pw, PH, CP,
                      pk, lane, nlanes);
      stage_patch<TW>(gl, ch_ok ? gy + n * Ho * Wo * C + c0 + pk * 8 : gy,
                      ch_ok, Ho, Wo, C, oh0, ow0, TH, CP, pk, lane, nlanes);
    }
    dw_sync();
    if (computes && ch_ok) {
      for (int p = plane; p < TH * TW; p += nplanes) {
        const int oh = p / TW, ow = p % TW;
        float gf[8];
        unpack8(gl[p * CP + pk], gf);
        const uint4* xp = xl + (oh * STRIDE * PW + ow * STRIDE) * CP + pk;
        if constexpr (R == 5) {
#pragma unroll
          for (int s = 0; s < R; ++s) {
            float xf[8];
            unpack8(xp[(g * PW + s) * CP], xf);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[s][j] += gf[j] * xf[j];
          }
        } else {
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int s = 0; s < R; ++s) {
              float xf[8];
              unpack8(xp[(r * PW + s) * CP], xf);
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[r * R + s][j] += gf[j] * xf[j];
            }
        }
      }
    }
  }

  // red[plane][G][CP][8]: at most 256 threads x 32 B = DW_RED_BYTES
  const int row = G * CP * 8;
  float* wslot = ws + (int64_t)slot * C * R * R;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    dw_sync();
    if (computes) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        red[plane * row + (g * CP + pk) * 8 + j] = acc[q][j];
    }
    dw_sync();
    for (int e = threadIdx.x; e < row; e += DW_THREADS) {
      float sum = 0.f;
      for (int pl = 0; pl < nplanes; ++pl) sum += red[pl * row + e];
      const int gg = e / (CP * 8);
      const int c = c0 + e - gg * CP * 8;
      const int tap = R == 5 ? gg * R + q : q;
      if (c < C) wslot[(int64_t)c * R * R + tap] = sum;
    }
  }
}

template <typename K, typename... A>
void dw_launch(K kern, dim3 grid, int lds, A... args) {
  hipLaunchKernelGGL(kern, grid, dim3(DW_THREADS), lds, cur_stream(), args...);
}

}  // namespace

// Forward over x [N, C, IH, IW] into y [N, C, OH, OW]; flip = stride-1 dgrad
// (x = gy, ph / pw already R-1-pad).
void dw_tile_fwd(const DwRoute& rt, const at::Tensor& x, const at::Tensor& w,
                 at::Tensor& y, int R, int st, int ph, int pw, bool flip) {
  const int N = x.size(0), C = x.size(1), IH = x.size(2), IW = x.size(3);
  const int OH = y.size(2), OW = y.size(3);
  const dim3 grid((unsigned)((int64_t)dw_ceil(N, rt.NB) * rt.tilesH *
                             rt.tilesW * rt.nchunk));
  auto go = [&](auto kern) {
    dw_launch(kern, grid, rt.lds_bytes, (const BF*)x.data_ptr(),
              (const BF*)w.data_ptr(), (BF*)y.data_ptr(), N, IH, IW, C, OH, OW,
              ph, pw, rt.TH, rt.CP, rt.NB, rt.tilesH, rt.tilesW, rt.nchunk);
  };
  const int key = R * 1000 + st * 100 + rt.TW;
  if (flip) {
    TORCH_CHECK(st == 1, "dw_tile_fwd: flip is the stride-1 dgrad");
    switch (key) {
      case 3116: return go(dw_tile_fwd_kernel<3, 1, 16, 4, true>);
      case 3108: return go(dw_tile_fwd_kernel<3, 1, 8, 4, true>);
      case 5116: return go(dw_tile_fwd_kernel<5, 1, 16, 4, true>);
      case 5108: return go(dw_tile_fwd_kernel<5, 1, 8, 4, true>);
    }
  } else {
    switch (key) {
      case 3116: return go(dw_tile_fwd_kernel<3, 1, 16, 4, false>);
      case 3108: return go(dw_tile_fwd_kernel<3, 1, 8, 4, false>);
      case 5116: return go(dw_tile_fwd_kernel<5, 1, 16, 4, false>);
      case 5108: return go(dw_tile_fwd_kernel<5, 1, 8, 4, false>);
      case 3208: return go(dw_tile_fwd_kernel<3, 2, 8, 2, false>);
      case 5208: return go(dw_tile_fwd_kernel<5, 2, 8, 2, false>);
    }
  }
  TORCH_CHECK(false, "dw_tile_fwd: no kernel for R=", R, " stride=", st,
              " TW=", rt.TW);
}

void dw_tile_dgrad_s2(const DwRoute& rt, const at::Tensor& gy,
                      const at::Tensor& w, at::Tensor& gx, int R, int ph,
                      int pw) {
  const int N = gy.size(0), C = gy.size(1), Ho = gy.size(2), Wo = gy.size(3);
  const int H = gx.size(2), W = gx.size(3);
  const dim3 grid(
      (unsigned)((int64_t)N * rt.tilesH * rt.tilesW * rt.nchunk));
  auto go = [&](auto kern) {
    dw_launch(kern, grid, rt.lds_bytes, (const BF*)gy.data_ptr(),
              (const BF*)w.data_ptr(), (BF*)gx.data_ptr(), N, H, W, C, Ho, Wo,
              ph, pw, rt.TH / 2, rt.CP, rt.tilesH, rt.tilesW, rt.nchunk);
  };
  if (R == 3) return go(dw_tile_dgrad_s2_kernel<3>);
  if (R == 5) return go(dw_tile_dgrad_s2_kernel<5>);
  TORCH_CHECK(false, "dw_tile_dgrad_s2: no kernel for R=", R);
}

// Partials into ws [rt.slots][C*R*R] fp32 (every element written).
void dw_tile_wgrad(const DwRoute& rt, const at::Tensor& gy,
                   const at::Tensor& x, at::Tensor& ws, int R, int st, int ph,
                   int pw) {
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int Ho = gy.size(2), Wo = gy.size(3);
  const int64_t items = (int64_t)N * rt.tilesH * rt.tilesW;
  const int64_t per = (items + rt.slots - 1) / rt.slots;
  const dim3 grid(rt.nchunk, rt.slots);
  auto go = [&](auto kern) {
    dw_launch(kern, grid, rt.lds_bytes, (const BF*)gy.data_ptr(),
              (const BF*)x.data_ptr(), ws.data_ptr<float>(), N, H, W, C, Ho,
              Wo, ph, pw, rt.TH, rt.CP, rt.tilesH, rt.tilesW, per, items);
  };
  switch (R * 1000 + st * 100 + rt.TW) {
    case 3116: return go(dw_tile_wgrad_kernel<3, 1, 16>);
    case 3108: return go(dw_tile_wgrad_kernel<3, 1, 8>);
    case 5116: return go(dw_tile_wgrad_kernel<5, 1, 16>);
    case 5108: return go(dw_tile_wgrad_kernel<5, 1, 8>);
    case 3208: return go(dw_tile_wgrad_kernel<3, 2, 8>);
    case 5208: return go(dw_tile_wgrad_kernel<5, 2, 8>);
  }
  TORCH_CHECK(false, "dw_tile_wgrad: no kernel for R=", R, " stride=", st,
              " TW=", rt.TW);
}
