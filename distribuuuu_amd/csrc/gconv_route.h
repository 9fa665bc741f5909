// Narrow-group conv routing: the ONE place that decides, per pass, whether a
// grouped 3x3 conv runs the LDS-tiled MFMA kernels (gconv_tile.hip) or the
// implicit-GEMM path (conv2d_fwd / conv2d_dgrad / conv2d_wgrad), and with
// which tile geometry. Plain C++17, no torch / HIP includes, so it can be
// compiled and swept on a CPU. docs/ARCHITECTURE.md "Narrow-group conv"
// states the range and the budget.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

constexpr int GC_THREADS = 256;
constexpr int GC_TW = 16;      // output pixels of an M tile (one MFMA's rows)
constexpr int GC_MAX_TH = 8;   // output rows per tile
constexpr int GC_MAX_CW = 64;  // channels per chunk: 128 B per pixel
constexpr int GC_PAD = 8;      // bf16 of padding per LDS pixel (16 bytes)
// Per-block LDS budget: four blocks fit a CU's 160 KiB (the depthwise rule).
constexpr int GC_LDS_BUDGET = 40 * 1024;
// fwd / dgrad epilogue: per wave a 16 pixel x 32 channel fp32 slab, row
// stride 36 floats
constexpr int GC_SLAB_STRIDE = 36;
constexpr int GC_SLAB_BYTES = 4 * 16 * GC_SLAB_STRIDE * 4;
constexpr int GC_FILL_BLOCKS = 1024;  // fwd / dgrad: four blocks per CU
constexpr int GC_WGRAD_BLOCKS = 512;  // wgrad: a slot costs K*9*Cg*4 bytes
constexpr int GC_MAX_SLOTS = 512;
// wgrad, w = 32, stride 2: output maps of this many pixels or more go back
constexpr int GC_W32_S2_WGRAD_OUT = 14 * 14;

enum class GcPass { Fwd, Dgrad, Wgrad };

struct GcRoute {
  bool tile = false;
  // Output tile TH x 16 of the pass (dgrad: gx pixels), chunk width CW
  // channels, `slots` persistent blocks per chunk of `per` items each.
  int TH = 0, CW = 0, nchunk = 0, tilesH = 0, tilesW = 0;
  int per = 0, slots = 0, lds_bytes = 0;
};

inline int gc_ceil(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// DISTRIBUUUU_GCONV_TILE=0 forces the implicit-GEMM path; re-read per call.
inline bool gconv_tile_enabled() {
  const char* e = getenv("DISTRIBUUUU_GCONV_TILE");
  return !(e && e[0] == '0');
}

// LDS columns of a patch row. Stride 2 keeps even and odd input columns in
// two halves of 17, so the 16 lanes of an A read are neighbours either way.
inline int gc_patch_cols(int st) { return st == 1 ? 18 : 34; }

// x is [N, C, H, W], the weight [K, C / groups, R, S].
inline GcRoute gconv_route(bool bf16_nhwc, int64_t N, int64_t C, int64_t K,
                           int64_t H, int64_t W, int64_t groups, int R, int S,
                           int sh, int sw, int ph, int pw, int dh, int dw,
                           GcPass pass, bool enabled = gconv_tile_enabled()) {
  GcRoute r;
  if (!enabled || !bf16_nhwc || N < 1 || groups < 2 || R != 3 || S != 3 ||
      dh != 1 || dw != 1 || sh != sw || (sh != 1 && sh != 2) || ph < 0 ||
      pw < 0 || ph > 1 || pw > 1 || C < 8 || C % 8 != 0 || K != C ||
      C % groups != 0 || H + 2 * ph < 3 || W + 2 * pw < 3 ||
      H > (1 << 20) || W > (1 << 20) || N > (1 << 24) || C > (1 << 20))
    return r;
  const int64_t w = C / groups;
  if (w != 4 && w != 8 && w != 16 && w != 32) return r;
  const int st = sh;
  const int Ho = (int)((H + 2 * ph - 3) / st + 1);
  const int Wo = (int)((W + 2 * pw - 3) / st + 1);
  // The one measured loser (docs/ARCHITECTURE.md "Narrow-group conv"): the
  // stride-2 weight gradient at w = 32 fits only two output rows per tile,
  // and from a 14x14 output map on the tr128 split-m kernel is faster.
  if (pass == GcPass::Wgrad && w == 32 && st == 2 &&
      (int64_t)Ho * Wo >= GC_W32_S2_WGRAD_OUT)
    return r;
  // the fewest equal chunks of at most 64 channels, a multiple of 32 wide
  r.nchunk = gc_ceil(C, GC_MAX_CW);
  r.CW = gc_ceil(gc_ceil(C, r.nchunk), 32) * 32;
  const int pitch = (r.CW + GC_PAD) * 2;

  // dgrad is the stride-1 machine over gy (stride 2: over its zero-inserted
  // canvas) with gx as the output; fwd and wgrad tile the conv's output
  const bool dg = pass == GcPass::Dgrad;
  const int ms = dg ? 1 : st;
  const int OH = dg ? (int)H : Ho, OW = dg ? (int)W : Wo;
  auto lds = [&](int th) {
    const int patch = ((th - 1) * ms + 3) * gc_patch_cols(ms) * pitch;
    if (pass == GcPass::Wgrad) return patch + th * GC_TW * pitch;
    return patch + GC_SLAB_BYTES;
  };
  int th = gc_ceil(OH, gc_ceil(OH, GC_MAX_TH));
  if (pass == GcPass::Wgrad) {
    // a k-step is two tile rows: TH even, the odd map's last row is zeros
    th += th & 1;
    while (th > 2 && lds(th) > GC_LDS_BUDGET) th -= 2;
  } else {
    while (th > 1 && lds(th) > GC_LDS_BUDGET) --th;
  }
  r.TH = th;
  r.lds_bytes = lds(th);
  if (r.lds_bytes > GC_LDS_BUDGET) return r;
  r.tilesH = gc_ceil(OH, th);
  r.tilesW = gc_ceil(OW, GC_TW);
  const int64_t items = N * r.tilesH * r.tilesW;
  if (items >= ((int64_t)1 << 30)) return r;
  // enough persistent blocks to fill the chip; each takes a contiguous run
  // of `per` (image, tile row, tile column) items
  const int fill = pass == GcPass::Wgrad ? GC_WGRAD_BLOCKS : GC_FILL_BLOCKS;
  const int64_t cap = pass == GcPass::Wgrad ? GC_MAX_SLOTS : GC_FILL_BLOCKS;
  const int64_t want = std::clamp<int64_t>(gc_ceil(fill, r.nchunk), 1,
                                           std::min<int64_t>(cap, items));
  r.per = (int)((items + want - 1) / want);
  r.slots = (int)((items + r.per - 1) / r.per);
  r.tile = true;
  return r;
}

// ---------------------------------------------------------------------------
// fp32 family (gconv_tile_f32.hip): the same range on fp32 NHWC tensors with
// C % 4 == 0. An fp32 pixel is CW floats plus GCF_PAD: 36 or 68 dwords, so
// sixteen lanes one pixel apart, 16 bytes each, start 4 * (9 i mod 16) or
// 4 * (i mod 16) dwords apart and cover the 64 banks once.
// ---------------------------------------------------------------------------
constexpr int GCF_PAD = 4;  // floats of padding per LDS pixel (16 bytes)
// the BN-partial epilogue meets in LDS: 256 threads x 8 floats
constexpr int GCF_MIN_LDS = GC_THREADS * 8 * 4;
// wgrad gates, in output pixels: stride 2 goes back from this size on at
// w = 32 and w = 16, stride 1 at w = 32 below this size
constexpr int GCF_W32_S2_WGRAD_OUT = 7 * 7;
constexpr int GCF_W16_S2_WGRAD_OUT = 28 * 28;
constexpr int GCF_W32_S1_WGRAD_OUT = 14 * 14;

// log2 of the wave groups that split a wgrad block's tile rows; each writes
// a workspace slot of its own, so the workspace has slots << this rows
constexpr int gcf_wgrad_split(int CW) { return CW == 32 ? 1 : 0; }

inline GcRoute gconv_f32_route(bool f32_nhwc, int64_t N, int64_t C, int64_t K,
                               int64_t H, int64_t W, int64_t groups, int R,
                               int S, int sh, int sw, int ph, int pw, int dh,
                               int dw, GcPass pass,
                               bool enabled = gconv_tile_enabled()) {
  GcRoute r;
  if (!enabled || !f32_nhwc || N < 1 || groups < 2 || R != 3 || S != 3 ||
      dh != 1 || dw != 1 || sh != sw || (sh != 1 && sh != 2) || ph < 0 ||
      pw < 0 || ph > 1 || pw > 1 || C < 8 || C % 4 != 0 || K != C ||
      C % groups != 0 || H + 2 * ph < 3 || W + 2 * pw < 3 ||
      H > (1 << 20) || W > (1 << 20) || N > (1 << 24) || C > (1 << 20))
    return r;
  const int64_t w = C / groups;
  if (w != 4 && w != 8 && w != 16 && w != 32) return r;
  const int st = sh;
  const int Ho = (int)((H + 2 * ph - 3) / st + 1);
  const int Wo = (int)((W + 2 * pw - 3) / st + 1);
  // The measured losers (docs/ARCHITECTURE.md "Narrow-group conv, fp32"),
  // all weight gradients, go back to conv2d_wgrad: a stride-2 patch leaves
  // two output rows per tile, and at C = 1024 a 7x7 map has too few items
  // per workspace slot.
  if (pass == GcPass::Wgrad) {
    const int64_t out = (int64_t)Ho * Wo;
    if ((w == 32 && st == 2 && out >= GCF_W32_S2_WGRAD_OUT) ||
        (w == 16 && st == 2 && out >= GCF_W16_S2_WGRAD_OUT) ||
        (w == 32 && st == 1 && out < GCF_W32_S1_WGRAD_OUT))
      return r;
  }
  // dgrad is the stride-1 machine over gy (stride 2: over its zero-inserted
  // canvas) with gx as the output; fwd and wgrad tile the conv's output
  const bool dg = pass == GcPass::Dgrad;
  const int ms = dg ? 1 : st;
  const int OH = dg ? (int)H : Ho, OW = dg ? (int)W : Wo;
  // 64-channel chunks (256 B of a pixel) where the stride-1 patch leaves
  // room for several tile rows; a stride-2 patch row is twice as long and
  // the weight gradient holds the gy tile as well: 32
  const int maxcw = (ms == 1 && pass != GcPass::Wgrad) ? 64 : 32;
  r.nchunk = gc_ceil(C, maxcw);
  r.CW = gc_ceil(gc_ceil(C, r.nchunk), 32) * 32;
  const int pitch = (r.CW + GCF_PAD) * 4;
  auto lds = [&](int th) {
    int b = ((th - 1) * ms + 3) * gc_patch_cols(ms) * pitch;
    if (pass == GcPass::Wgrad) b += th * GC_TW * pitch;
    return std::max(b, GCF_MIN_LDS);
  };
  int th = gc_ceil(OH, gc_ceil(OH, GC_MAX_TH));
  while (th > 1 && lds(th) > GC_LDS_BUDGET) --th;
  r.TH = th;
  r.lds_bytes = lds(th);
  if (r.lds_bytes > GC_LDS_BUDGET) return r;
  r.tilesH = gc_ceil(OH, th);
  r.tilesW = gc_ceil(OW, GC_TW);
  const int64_t items = N * r.tilesH * r.tilesW;
  if (items >= ((int64_t)1 << 30)) return r;
  const bool wg = pass == GcPass::Wgrad;
  const int fill = wg ? GC_WGRAD_BLOCKS >> gcf_wgrad_split(r.CW)
                      : GC_FILL_BLOCKS;
  const int64_t cap = wg ? GC_MAX_SLOTS >> gcf_wgrad_split(r.CW)
                         : GC_FILL_BLOCKS;
  const int64_t want = std::clamp<int64_t>(gc_ceil(fill, r.nchunk), 1,
                                           std::min<int64_t>(cap, items));
  r.per = (int)((items + want - 1) / want);
  r.slots = (int)((items + r.per - 1) / r.per);
  r.tile = true;
  return r;
}
