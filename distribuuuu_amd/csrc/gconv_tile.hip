// LDS-tiled MFMA kernels for narrow-group 3x3 convolutions on gfx950: bf16
// NHWC, Cg == Kg == w in {4, 8, 16, 32}, stride 1 or 2, pad <= 1
// (gconv_route.h decides; docs/ARCHITECTURE.md "Narrow-group conv" has the
// design). These convs are bandwidth-bound, so every kernel stages the input
// patch in LDS once and takes all nine taps from there; the per-pixel work is
// a small matrix product and runs on v_mfma_f32_16x16x32_bf16.
//
// Common layout. A block of 256 threads works on a chunk of CW = 32 or 64
// channels. The LDS image of a pixel is CW bf16 plus 16 bytes of padding, so
// the pixel pitch is 80 or 144 bytes = 20 or 36 dwords: sixteen lanes one
// pixel apart, each reading 16 bytes, start 4 * (5 i mod 16) or
// 4 * (9 i mod 16) dwords apart and cover the 64 banks once. At stride 2 the
// patch keeps its even and its odd columns in two halves, so the lanes of a
// tap are one LDS pixel apart there too. Out-of-image pixels and channels
// past C are WRITTEN as zeros on every tile (LDS is recycled).
//
// MFMA operands (lane = 16 * kq + il): A row il / B column il, k = 8 kq .. + 8;
// D column il, rows 4 kq .. + 4.
#include "common.h"
#include "gconv_route.h"

// packed fp32 math (v_pk_*_f32) is kept out of this file's kernels. Header
// helpers lack the attribute and would be called, not inlined: builtins only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4g;
typedef __bf16 bf16x8g __attribute__((ext_vector_type(8)));
typedef unsigned short bfraw;

// 16 bytes of LDS as an MFMA operand
DEV_INLINE bf16x8g gc_lds_frag(const char* p) {
  return __builtin_bit_cast(bf16x8g, *reinterpret_cast<const uint4*>(p));
}

// what __syncthreads() does
DEV_INLINE void gc_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// fp32 -> bf16 bits, round to nearest even; NaN stays a quiet NaN
DEV_INLINE unsigned gc_round(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
DEV_INLINE float gc_f32(unsigned bf) {
  return __builtin_bit_cast(float, bf << 16);
}

// LDS column of patch column c, and the LDS pixel offset of tap t = 3 r + s
// from the patch pixel of an output's tap 0
template <int STRIDE>
DEV_INLINE constexpr int gc_col(int c) {
  return STRIDE == 1 ? c : (c & 1) * 17 + (c >> 1);
}
template <int STRIDE>
DEV_INLINE constexpr int gc_tap(int t) {
  return (t / 3) * (STRIDE == 1 ? 18 : 34) + gc_col<STRIDE>(t % 3);
}

struct GcItem {
  int n, th, tw;
};
// an item index is split once per block; the run then steps
DEV_INLINE GcItem gc_decode(int it, int tilesH, int tilesW) {
  GcItem i;
  i.tw = it % tilesW;
  const int t2 = it / tilesW;
  i.th = t2 % tilesH;
  i.n = t2 / tilesH;
  return i;
}
DEV_INLINE void gc_next(GcItem& i, int tilesH, int tilesW) {
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
DEV_INLINE void gc_stage_patch(char* lds, const bfraw* src, int IH, int IW,
                               int C, int c0, int CW, int u0, int v0, int PH) {
  constexpr int PW = 15 * STRIDE + 3, PWP = STRIDE == 1 ? 18 : 34;
  const int lpk = CW == 64 ? 3 : 2;  // log2 of the packs of a pixel
  const int pk = threadIdx.x & ((1 << lpk) - 1);
  const int pitch = (CW + GC_PAD) * 2;
  const bool ch_ok = c0 + pk * 8 < C;
  for (int px = threadIdx.x >> lpk; px < PH * PW; px += GC_THREADS >> lpk) {
    const int row = px / PW, col = px - row * PW;
    int u = u0 + row, v = v0 + col;
    bool ok = ch_ok;
    if constexpr (DILATE) {
      ok = ok && u >= 0 && v >= 0 && ((u | v) & 1) == 0;
      u >>= 1, v >>= 1;
    }
    ok = ok && (unsigned)u < (unsigned)IH && (unsigned)v < (unsigned)IW;
    uint4 val = {0u, 0u, 0u, 0u};
    if (ok)
      val = *reinterpret_cast<const uint4*>(src + ((int64_t)u * IW + v) * C +
                                            c0 + pk * 8);
    *reinterpret_cast<uint4*>(lds + (row * PWP + gc_col<STRIDE>(col)) * pitch +
                              pk * 16) = val;
  }
}

// B fragment of the 16 output channels ct0 .. + 16 at k-step st, from the raw
// [K][9][w] weight. w <= 16: k = 8 kq + i is tap 2 st + kq / 2, tile-local
// input channel 8 (kq % 2) + i, live where that channel and column il share a
// group; the tenth tap and everything dead are literal zeros. w = 32: tap st,
// input channel 8 kq + i of the group. FLIP builds the data gradient's
// operand B[n = ci][tap, ko] = w[g w + ko][8 - tap][ci] by element gathers.
template <bool W32, bool FLIP>
DEV_INLINE bf16x8g gc_build_b(const bfraw* wt, int C, int lw, int ct0, int st,
                              int il, int kq) {
  uint4 b = {0u, 0u, 0u, 0u};
  const int col = ct0 + il;
  const int t = W32 ? st : 2 * st + (kq >> 1);
  const int h = kq & 1;
  if (col < C && t <= 8) {
    if constexpr (FLIP) {
      const int ci = col & ((1 << lw) - 1);
      auto e = [&](int i) -> unsigned {
        // gy channel of this k, and whether it is in the column's group
        const int kl = W32 ? 8 * kq + i : 8 * h + i;
        const int ko = W32 ? (ct0 & ~31) + kl : ct0 + kl;
        if (W32 || (kl >> lw) == (il >> lw))
          return wt[(((int64_t)ko * 9 + 8 - t) << lw) + ci];
        return 0u;
      };
      b.x = e(0) | (e(1) << 16);
      b.y = e(2) | (e(3) << 16);
      b.z = e(4) | (e(5) << 16);
      b.w = e(6) | (e(7) << 16);
    } else if constexpr (W32) {
      b = *reinterpret_cast<const uint4*>(wt + ((int64_t)col * 9 + t) * 32 +
                                          8 * kq);
    } else {
      const bfraw* row = wt + (((int64_t)col * 9 + t) << lw);
      if (lw == 4) {
        b = *reinterpret_cast<const uint4*>(row + 8 * h);
      } else if (h == (il >> 3)) {
        if (lw == 3) {
          b = *reinterpret_cast<const uint4*>(row);
        } else {
          const uint2 v = *reinterpret_cast<const uint2*>(row);
          const bool hi = ((il >> 2) & 1) != 0;
          b.x = hi ? 0u : v.x, b.y = hi ? 0u : v.y;
          b.z = hi ? v.x : 0u, b.w = hi ? v.y : 0u;
        }
      }
    }
  }
  return __builtin_bit_cast(bf16x8g, b);
}

struct GcParams {
  const bfraw* x;  // the staged operand [N, IH, IW, C] (dgrad: gy)
  const bfraw* w;  // raw weight [K][3][3][w]
  bfraw* y;        // [N, OH, OW, C]
  float* part;     // EMIT: [gridDim.y][2 * C] BN sum / sum-of-squares rows
  int N, IH, IW, C, OH, OW;
  int oy, ox;  // patch origin of output (0, 0): -pad (dgrad: pad - 2)
  int lw;      // log2 of the group width
  int TH, CW, tilesH, tilesW, per, items;
};

// ---------------------------------------------------------------------------
// forward, and the data gradient (FLIP; DILATE for stride 2)
// ---------------------------------------------------------------------------
// grid (chunk, slot). Wave wv is pinned to the 32-channel block cb of the
// chunk, keeps that block's B fragments in registers for the whole run and
// walks the tile's pixel rows rw, rw + nrw, ...: an M tile is the 16 pixels
// of one output row. The 16 x 32 fp32 result is restaged through the wave's
// private slab, rounded to bf16 once and stored as 16 bytes per lane.
template <bool W32, int STRIDE, bool FLIP, bool DILATE, bool EMIT>
__global__ __launch_bounds__(GC_THREADS) void gconv_tile_kernel(GcParams p) {
  constexpr int PWP = STRIDE == 1 ? 18 : 34;
  constexpr int NS = W32 ? 9 : 5;  // k-steps
  extern __shared__ uint4 gc_smem[];
  char* lds = reinterpret_cast<char*>(gc_smem);
  const int pitch = (p.CW + GC_PAD) * 2;
  const int PH = (p.TH - 1) * STRIDE + 3;
  float* slabs = reinterpret_cast<float*>(lds + PH * PWP * pitch);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int nblk = p.CW >> 5;  // 32-channel blocks of the chunk: 1 or 2
  const int cb = wv & (nblk - 1), rw = wv >> (nblk - 1), nrw = 4 >> (nblk - 1);
  const int c0 = blockIdx.x * p.CW;
  const int cw0 = c0 + cb * 32;

  bf16x8g B[2][NS];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int st = 0; st < NS; ++st)
      B[j][st] = gc_build_b<W32, FLIP>(p.w, p.C, p.lw, cw0 + j * 16, st, il, kq);

  // this lane's A chunk: pixel il of the row, 8 channels of its quad
  const int a_lane = il * pitch + (cb * 32 + (W32 ? kq * 8 : (kq & 1) * 8)) * 2;
  const bool odd_tap = (kq >> 1) != 0;
  float* slab = slabs + wv * 16 * GC_SLAB_STRIDE;
  const int epx = lane >> 2, ech = cw0 + (lane & 3) * 8;
  float ps = 0.f, pq = 0.f;

  int it = blockIdx.y * p.per;
  const int it1 = it + p.per < p.items ? it + p.per : p.items;
  GcItem item = gc_decode(it, p.tilesH, p.tilesW);
  for (; it < it1; ++it, gc_next(item, p.tilesH, p.tilesW)) {
    const int oh0 = item.th * p.TH, ow0 = item.tw * GC_TW;
    gc_sync();  // the previous item's readers are done
    gc_stage_patch<STRIDE, DILATE>(
        lds, p.x + (int64_t)item.n * p.IH * p.IW * p.C, p.IH, p.IW, p.C, c0,
        p.CW, oh0 * STRIDE + p.oy, ow0 * STRIDE + p.ox, PH);
    gc_sync();
    for (int row = rw; row < p.TH && oh0 + row < p.OH; row += nrw) {
      const char* ap = lds + row * STRIDE * PWP * pitch + a_lane;
      f32x4g acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        if constexpr (W32) {
          const bf16x8g a = gc_lds_frag(ap + gc_tap<STRIDE>(st) * pitch);
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B[0][st], acc[0],
                                                           0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B[1][st], acc[1],
                                                           0, 0, 0);
        } else {
          // quads 2, 3 take the odd tap; the tenth re-reads tap 8 against a
          // zero B chunk
          const int T0 = gc_tap<STRIDE>(2 * st);
          const int T1 = gc_tap<STRIDE>(st == 4 ? 8 : 2 * st + 1);
          const char* tp = ap + (odd_tap ? T1 : T0) * pitch;
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                gc_lds_frag(tp + j * 32), B[j][st], acc[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          slab[(kq * 4 + rr) * GC_SLAB_STRIDE + j * 16 + il] = acc[j][rr];
      __builtin_amdgcn_wave_barrier();
      if (ow0 + epx < p.OW && ech < p.C) {
        const f32x4g lo = *reinterpret_cast<const f32x4g*>(
            slab + epx * GC_SLAB_STRIDE + (lane & 3) * 8);
        const f32x4g hi = *reinterpret_cast<const f32x4g*>(
            slab + epx * GC_SLAB_STRIDE + (lane & 3) * 8 + 4);
        uint4 o;
        o.x = gc_round(lo[0]) | (gc_round(lo[1]) << 16);
        o.y = gc_round(lo[2]) | (gc_round(lo[3]) << 16);
        o.z = gc_round(hi[0]) | (gc_round(hi[1]) << 16);
        o.w = gc_round(hi[2]) | (gc_round(hi[3]) << 16);
        *reinterpret_cast<uint4*>(
            p.y + (((int64_t)item.n * p.OH + oh0 + row) * p.OW + ow0 + epx) *
                      p.C + ech) = o;
      }
      if constexpr (EMIT) {
        // column lane % 32 of the slab, eight pixels per half-wave
        const int col = lane & 31, px0 = (lane >> 5) * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (ow0 + px0 + r < p.OW) {
            const float v =
                gc_f32(gc_round(slab[(px0 + r) * GC_SLAB_STRIDE + col]));
            ps += v;
            pq += v * v;
          }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  if constexpr (EMIT) {
    // the block's row of the partial tensor: per channel the lanes' sums in
    // (row walker, half-wave) order, one plain store each
    gc_sync();
    slabs[threadIdx.x * 2] = ps;
    slabs[threadIdx.x * 2 + 1] = pq;
    gc_sync();
    const int c = threadIdx.x;
    if (c < p.CW && c0 + c < p.C) {
      float s = 0.f, q = 0.f;
      for (int r = 0; r < nrw; ++r)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int t = (r * nblk + (c >> 5)) * 64 + half * 32 + (c & 31);
          s += slabs[t * 2];
          q += slabs[t * 2 + 1];
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
// Transposed fragment of a pixel-major LDS image: this lane supplies the
// addresses of 4 channels of pixels p and p + 4 and receives 8 pixels of one
// channel (lane semantics: docs/ARCHITECTURE.md "Weight gradient").
DEV_INLINE bf16x8g gc_tr_read(unsigned a0, unsigned a1) {
  union {
    uint2 h[2];
    bf16x8g v;
  } u;
  asm volatile(
      "s_waitcnt lgkmcnt(0)\n\t"
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(u.h[0]), "=&v"(u.h[1])
      : "v"(a0), "v"(a1)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  return u.v;
}

struct GwParams {
  const bfraw* gy;  // [N, Ho, Wo, C]
  const bfraw* x;   // [N, H, W, C]
  float* ws;        // [gridDim.y][C * 9 * w]
  int N, H, W, C, Ho, Wo, ph, pw, lw;
  int TH, CW, tilesH, tilesW, per, items;
};

// grid (chunk, slot): the block walks the slot's run of (image, tile) items
// and stages the x patch and the gy tile of each. The reduction index is the
// pixel, a k-step two tile rows of 16. Wave unit u owns the 16 gy channels
// u * 16 .. of the chunk (w = 32: one ko half of a group) and their group's x
// channels; per tap one MFMA per 16 x channels into its own accumulator, the
// gy fragment shared by the nine taps, a tap being an address offset. With
// two units (CW = 32) the wave pairs split the k-steps and meet in LDS in
// wave order. The diagonal w x w blocks go to this slot of ws with plain
// stores: one writer per element, a fixed order.
template <bool W32, int STRIDE>
__global__ __launch_bounds__(GC_THREADS) void gconv_tile_wgrad_kernel(
    GwParams p) {
  constexpr int PWP = STRIDE == 1 ? 18 : 34;
  constexpr int NX = W32 ? 2 : 1;
  extern __shared__ uint4 gc_smem[];
  char* lds = reinterpret_cast<char*>(gc_smem);
  const int pitch = (p.CW + GC_PAD) * 2;
  const int PH = (p.TH - 1) * STRIDE + 3;
  char* gl = lds + PH * PWP * pitch;  // [TH][16] pixels of gy
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = lane & 15, kq = lane >> 4;
  const int nun = p.CW >> 4;  // units: 2 or 4
  const int un = wv & (nun - 1), ks = nun == 4 ? 0 : wv >> 1, nks = 4 / nun;
  const int c0 = blockIdx.x * p.CW;
  const int lpk = p.CW == 64 ? 3 : 2;

  // k = 8 kq + i is pixel (row kq / 2, column 8 (kq % 2) + i) of a row pair;
  // the lane addresses 4 channels of pixel column 8 (kq % 2) + il / 4
  const int prow = kq >> 1, pcol = (kq & 1) * 8 + (il >> 2);
  const unsigned lds0 = (unsigned)(unsigned long long)lds;
  const unsigned g_lane =
      lds0 + PH * PWP * pitch + pcol * pitch + un * 32 + (il & 3) * 8;
  const unsigned x_lane =
      lds0 + pcol * pitch + (W32 ? (un & ~1) : un) * 32 + (il & 3) * 8;

  f32x4g acc[NX][9];
#pragma unroll
  for (int xt = 0; xt < NX; ++xt)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[xt][t] = f32x4g{0.f, 0.f, 0.f, 0.f};

  int it = blockIdx.y * p.per;
  const int it1 = it + p.per < p.items ? it + p.per : p.items;
  GcItem item = gc_decode(it, p.tilesH, p.tilesW);
  for (; it < it1; ++it, gc_next(item, p.tilesH, p.tilesW)) {
    const int oh0 = item.th * p.TH, ow0 = item.tw * GC_TW;
    gc_sync();  // the previous item's readers are done
    gc_stage_patch<STRIDE, false>(
        lds, p.x + (int64_t)item.n * p.H * p.W * p.C, p.H, p.W, p.C, c0, p.CW,
        oh0 * STRIDE - p.ph, ow0 * STRIDE - p.pw, PH);
    {
      const bfraw* src = p.gy + (int64_t)item.n * p.Ho * p.Wo * p.C;
      const int pk = threadIdx.x & ((1 << lpk) - 1);
      for (int px = threadIdx.x >> lpk; px < p.TH * GC_TW;
           px += GC_THREADS >> lpk) {
        const int oh = oh0 + (px >> 4), ow = ow0 + (px & 15);
        uint4 val = {0u, 0u, 0u, 0u};
        if (oh < p.Ho && ow < p.Wo && c0 + pk * 8 < p.C)
          val = *reinterpret_cast<const uint4*>(
              src + ((int64_t)oh * p.Wo + ow) * p.C + c0 + pk * 8);
        *reinterpret_cast<uint4*>(gl + px * pitch + pk * 16) = val;
      }
    }
    gc_sync();
    for (int kk = ks; 2 * kk < p.TH && oh0 + 2 * kk < p.Ho; kk += nks) {
      const int row = 2 * kk + prow;
      const unsigned ga = g_lane + row * GC_TW * pitch;
      const bf16x8g gf = gc_tr_read(ga, ga + 4 * pitch);
      const unsigned xa = x_lane + row * STRIDE * PWP * pitch;
#pragma unroll
      for (int xt = 0; xt < NX; ++xt)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const unsigned a = xa + xt * 32 + gc_tap<STRIDE>(t) * pitch;
          const bf16x8g xf = gc_tr_read(a, a + 4 * pitch);
          acc[xt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xf, gf, acc[xt][t], 0, 0, 0);
        }
    }
  }

  // D row 4 kq + rr is the x channel, column il the gy channel
  float* red = reinterpret_cast<float*>(lds);  // [wave][lane][4]
  float* wslot = p.ws + (int64_t)blockIdx.y * p.C * (9 << p.lw);
  const int k = c0 + un * 16 + il;
#pragma unroll
  for (int xt = 0; xt < NX; ++xt)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      f32x4g a = acc[xt][t];
      if (nks > 1) {
        gc_sync();
        if (ks > 0)
          *reinterpret_cast<f32x4g*>(red + threadIdx.x * 4) = a;
        gc_sync();
        if (ks == 0) {
          const f32x4g o = *reinterpret_cast<const f32x4g*>(
              red + (threadIdx.x + 2 * 64) * 4);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) a[rr] += o[rr];
        }
      }
      if (ks == 0 && k < p.C) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ct = kq * 4 + rr;
          if (W32 || (ct >> p.lw) == (il >> p.lw))
            wslot[(((int64_t)k * 9 + t) << p.lw) +
                  (W32 ? xt * 16 + ct : ct & ((1 << p.lw) - 1))] = a[rr];
        }
      }
    }
}

GcParams gc_params(const GcRoute& rt, const at::Tensor& x, const at::Tensor& w,
                   at::Tensor& y, int oy, int ox) {
  GcParams p{};
  p.x = reinterpret_cast<const bfraw*>(x.data_ptr());
  p.w = reinterpret_cast<const bfraw*>(w.data_ptr());
  p.y = reinterpret_cast<bfraw*>(y.data_ptr());
  p.N = x.size(0), p.C = x.size(1), p.IH = x.size(2), p.IW = x.size(3);
  p.OH = y.size(2), p.OW = y.size(3);
  p.oy = oy, p.ox = ox;
  const int gw = w.size(1);
  p.lw = gw == 4 ? 2 : gw == 8 ? 3 : gw == 16 ? 4 : 5;
  p.TH = rt.TH, p.CW = rt.CW, p.tilesH = rt.tilesH, p.tilesW = rt.tilesW;
  p.per = rt.per, p.items = (int)(x.size(0) * rt.tilesH * rt.tilesW);
  return p;
}

template <typename K, typename P>
void gc_launch(K kern, const GcRoute& rt, const P& p) {
  hipLaunchKernelGGL(kern, dim3(rt.nchunk, rt.slots), dim3(GC_THREADS),
                     rt.lds_bytes, cur_stream(), p);
}

}  // namespace

// Forward over x [N, C, H, W] into y; part != nullptr: the [rt.slots][2 C]
// BN partial rows as well.
void gconv_tile_fwd(const GcRoute& rt, const at::Tensor& x,
                    const at::Tensor& w, at::Tensor& y, int st, int ph, int pw,
                    float* part) {
  GcParams p = gc_params(rt, x, w, y, -ph, -pw);
  p.part = part;
  const int key = (p.lw == 5) * 4 + (st == 2) * 2 + (part != nullptr);
  switch (key) {
    case 0: return gc_launch(gconv_tile_kernel<false, 1, false, false, false>, rt, p);
    case 1: return gc_launch(gconv_tile_kernel<false, 1, false, false, true>, rt, p);
    case 2: return gc_launch(gconv_tile_kernel<false, 2, false, false, false>, rt, p);
    case 3: return gc_launch(gconv_tile_kernel<false, 2, false, false, true>, rt, p);
    case 4: return gc_launch(gconv_tile_kernel<true, 1, false, false, false>, rt, p);
    case 5: return gc_launch(gconv_tile_kernel<true, 1, false, false, true>, rt, p);
    case 6: return gc_launch(gconv_tile_kernel<true, 2, false, false, false>, rt, p);
    case 7: return gc_launch(gconv_tile_kernel<true, 2, false, false, true>, rt, p);
  }
}

// Data gradient: the forward machine over gy with the flipped operand and
// pad' = 2 - pad; stride 2 stages gy's zero-inserted canvas.
void gconv_tile_dgrad(const GcRoute& rt, const at::Tensor& gy,
                      const at::Tensor& w, at::Tensor& gx, int st, int ph,
                      int pw) {
  const GcParams p = gc_params(rt, gy, w, gx, ph - 2, pw - 2);
  const bool w32 = p.lw == 5;
  if (st == 1) {
    if (w32) return gc_launch(gconv_tile_kernel<true, 1, true, false, false>, rt, p);
    return gc_launch(gconv_tile_kernel<false, 1, true, false, false>, rt, p);
  }
  if (w32) return gc_launch(gconv_tile_kernel<true, 1, true, true, false>, rt, p);
  return gc_launch(gconv_tile_kernel<false, 1, true, true, false>, rt, p);
}

// Partials into ws [rt.slots][C * 9 * w] fp32 (every element written).
void gconv_tile_wgrad(const GcRoute& rt, const at::Tensor& gy,
                      const at::Tensor& x, at::Tensor& ws, int gw, int st,
                      int ph, int pw) {
  GwParams p{};
  p.gy = reinterpret_cast<const bfraw*>(gy.data_ptr());
  p.x = reinterpret_cast<const bfraw*>(x.data_ptr());
  p.ws = ws.data_ptr<float>();
  p.N = x.size(0), p.C = x.size(1), p.H = x.size(2), p.W = x.size(3);
  p.Ho = gy.size(2), p.Wo = gy.size(3);
  p.ph = ph, p.pw = pw;
  p.lw = gw == 4 ? 2 : gw == 8 ? 3 : gw == 16 ? 4 : 5;
  p.TH = rt.TH, p.CW = rt.CW, p.tilesH = rt.tilesH, p.tilesW = rt.tilesW;
  p.per = rt.per, p.items = (int)(x.size(0) * rt.tilesH * rt.tilesW);
  const bool w32 = p.lw == 5;
  if (st == 1) {
    if (w32) return gc_launch(gconv_tile_wgrad_kernel<true, 1>, rt, p);
    return gc_launch(gconv_tile_wgrad_kernel<false, 1>, rt, p);
  }
  if (w32) return gc_launch(gconv_tile_wgrad_kernel<true, 2>, rt, p);
  return gc_launch(gconv_tile_wgrad_kernel<false, 2>, rt, p);
}

// ---------------------------------------------------------------------------
// entry points: each asks the route and refuses what it does not admit
// ---------------------------------------------------------------------------
namespace {

GcRoute gc_route_of(const at::Tensor& t, int64_t C, int64_t K, int64_t H,
                    int64_t W, int64_t groups, int64_t R, int64_t S,
                    int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                    int64_t dw, GcPass pass) {
  const bool ok = t.scalar_type() == at::kBFloat16 && t.dim() == 4 &&
                  t.is_contiguous(at::MemoryFormat::ChannelsLast);
  return gconv_route(ok, t.size(0), C, K, H, W, groups, (int)R, (int)S,
                     (int)sh, (int)sw, (int)ph, (int)pw, (int)dh, (int)dw,
                     pass);
}

// staging and weight loads are 16-byte vector loads from data_ptr()
void gc_check_aligned(const at::Tensor& t, const char* who, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, ": ",
              name, " must start 16-byte aligned");
}

void gc_check_weight(const at::Tensor& w, int64_t C, int64_t groups,
                     const char* who) {
  CHECK_GPU(w);
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.dim() == 4 &&
                  w.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  w.size(0) == C && w.size(1) * groups == C &&
                  w.size(2) == 3 && w.size(3) == 3,
              who, ": weight must be bf16 channels_last [C, C/groups, 3, 3], "
              "got ", w.sizes());
  gc_check_aligned(w, who, "weight");
}

std::tuple<at::Tensor, at::Tensor> gc_forward(at::Tensor x, at::Tensor w,
                                              int64_t sh, int64_t sw,
                                              int64_t ph, int64_t pw,
                                              int64_t groups, bool emit) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 4, "gconv_fwd: x must be 4-D");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const GcRoute rt =
      gc_route_of(x, C, w.size(0), H, W, groups, w.size(2), w.size(3), sh, sw,
                  ph, pw, 1, 1, GcPass::Fwd);
  TORCH_CHECK(rt.tile, "gconv_fwd: outside the tiled range (gconv_route)");
  gc_check_weight(w, C, groups, "gconv_fwd");
  gc_check_aligned(x, "gconv_fwd", "x");
  const int64_t Ho = (H + 2 * ph - 3) / sh + 1, Wo = (W + 2 * pw - 3) / sw + 1;
  auto y = at::empty({N, C, Ho, Wo},
                     x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor part;
  if (emit)
    part = at::empty({(int64_t)rt.slots, 2 * C}, x.options().dtype(at::kFloat));
  gconv_tile_fwd(rt, x, w, y, (int)sh, (int)ph, (int)pw,
                 emit ? part.data_ptr<float>() : nullptr);
  return {y, part};
}

}  // namespace

at::Tensor gconv_fwd(at::Tensor x, at::Tensor w, int64_t sh, int64_t sw,
                     int64_t ph, int64_t pw, int64_t groups) {
  return std::get<0>(gc_forward(x, w, sh, sw, ph, pw, groups, false));
}

// -> (y, part [blocks, 2 K] fp32): batch_norm_act's _bn_partials format
std::tuple<at::Tensor, at::Tensor> gconv_fwd_bn(at::Tensor x, at::Tensor w,
                                                int64_t sh, int64_t sw,
                                                int64_t ph, int64_t pw,
                                                int64_t groups) {
  return gc_forward(x, w, sh, sw, ph, pw, groups, true);
}

at::Tensor gconv_dgrad(at::Tensor gy, at::Tensor w, int64_t H, int64_t W,
                       int64_t sh, int64_t sw, int64_t ph, int64_t pw,
                       int64_t groups) {
  CHECK_GPU(gy);
  TORCH_CHECK(gy.dim() == 4, "gconv_dgrad: gy must be 4-D");
  const int64_t N = gy.size(0), C = gy.size(1);
  const GcRoute rt =
      gc_route_of(gy, C, w.size(0), H, W, groups, w.size(2), w.size(3), sh, sw,
                  ph, pw, 1, 1, GcPass::Dgrad);
  TORCH_CHECK(rt.tile && gy.size(2) == (H + 2 * ph - 3) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - 3) / sw + 1,
              "gconv_dgrad: outside the tiled range (gconv_route)");
  gc_check_weight(w, C, groups, "gconv_dgrad");
  gc_check_aligned(gy, "gconv_dgrad", "gy");
  auto gx = at::empty({N, C, H, W},
                      gy.options().memory_format(at::MemoryFormat::ChannelsLast));
  gconv_tile_dgrad(rt, gy, w, gx, (int)sh, (int)ph, (int)pw);
  return gx;
}

// The gradient in the shape and strides conv2d_wgrad returns.
at::Tensor gconv_wgrad(at::Tensor gy, at::Tensor x, int64_t sh, int64_t sw,
                       int64_t ph, int64_t pw, int64_t groups) {
  CHECK_GPU(gy);
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 4 && gy.dim() == 4, "gconv_wgrad: 4-D operands");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const GcRoute rt = gc_route_of(x, C, gy.size(1), H, W, groups, 3, 3, sh, sw,
                                 ph, pw, 1, 1, GcPass::Wgrad);
  TORCH_CHECK(rt.tile && gy.scalar_type() == at::kBFloat16 &&
                  gy.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  gy.size(0) == N &&
                  gy.size(2) == (H + 2 * ph - 3) / sh + 1 &&
                  gy.size(3) == (W + 2 * pw - 3) / sw + 1,
              "gconv_wgrad: outside the tiled range (gconv_route)");
  gc_check_aligned(x, "gconv_wgrad", "x");
  gc_check_aligned(gy, "gconv_wgrad", "gy");
  const int64_t gw_ = C / groups, n = C * 9 * gw_;
  // one slot per block, summed in slot order: the same bits in both
  // determinism modes, so the flag is not read
  auto ws = at::empty({(int64_t)rt.slots, n}, x.options().dtype(at::kFloat));
  gconv_tile_wgrad(rt, gy, x, ws, (int)gw_, (int)sh, (int)ph, (int)pw);
  auto gw = at::empty({C, gw_, 3, 3},
                      x.options().memory_format(at::MemoryFormat::ChannelsLast));
  ordered_reduce<__hip_bfloat16>(ws.data_ptr<float>(),
                                 (__hip_bfloat16*)gw.data_ptr(), rt.slots, n,
                                 1.f);
  return gw;
}

// (route, TH, chunk width, chunks, items per block, blocks per chunk,
// lds_bytes) of one pass ("fwd", "dgrad", "wgrad") over x [N, C, H, W] with a
// [K, C / groups, R, S] weight; classifies only, so meta tensors work.
std::tuple<std::string, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>
gconv_route_py(at::Tensor x, int64_t K, int64_t groups, int64_t R, int64_t S,
               int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
               int64_t dw, std::string pass) {
  TORCH_CHECK(x.dim() == 4, "x must be 4-D");
  TORCH_CHECK(pass == "fwd" || pass == "dgrad" || pass == "wgrad",
              "pass must be fwd, dgrad or wgrad, got ", pass);
  TORCH_CHECK(groups >= 1, "groups must be positive");
  const GcPass p = pass == "fwd"     ? GcPass::Fwd
                   : pass == "dgrad" ? GcPass::Dgrad
                                     : GcPass::Wgrad;
  const GcRoute rt = gc_route_of(x, x.size(1), K, x.size(2), x.size(3), groups,
                                 R, S, sh, sw, ph, pw, dh, dw, p);
  if (!rt.tile) return {"generic", 0, 0, 0, 0, 0, 0};
  return {"tile", rt.TH, rt.CW, rt.nchunk, rt.per, rt.slots, rt.lds_bytes};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
