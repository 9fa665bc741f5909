// Depthwise-conv routing: the ONE place that decides, per pass, whether a
// depthwise conv runs the LDS-tiled kernels (depthwise_tile.hip) or the
// generic grid-stride kernels (depthwise.hip), and with which tile geometry.
// Plain C++17, no torch / HIP includes, so it can be compiled and swept on a
// CPU. docs/ARCHITECTURE.md "Depthwise" states the range and the budget.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

constexpr int DW_THREADS = 256;
constexpr int DW_MAX_CP = 8;  // 16-byte packs per chunk: 64 channels = 128 B
// Per-block LDS budget: four blocks fit a CU's 160 KiB.
constexpr int DW_LDS_BUDGET = 40 * 1024;
constexpr int DW_MAX_TH = 8;      // output rows per tile (stride-2 dgrad: quads)
constexpr int DW_FILL_BLOCKS = 1024;  // wgrad: blocks wanted over all chunks
constexpr int DW_MAX_SLOTS = 512;
constexpr int DW_RED_BYTES = DW_THREADS * 8 * 4;  // wgrad's end-of-run tree

enum class DwPass { Fwd, Dgrad, Wgrad };

struct DwRoute {
  bool tiled = false;
  // Output tile TH x TW of the pass (dgrad: gx pixels), CP packs of 8
  // channels per chunk, NB images per block, wgrad slots.
  int TH = 0, TW = 0, CP = 0, NB = 1, slots = 0;
  int nchunk = 0, tilesH = 0, tilesW = 0;
  int lds_bytes = 0;
};

inline int dw_ceil(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// DISTRIBUUUU_DW_TILE=0 forces the generic kernels; re-read on every call.
inline bool dw_tile_enabled() {
  const char* e = getenv("DISTRIBUUUU_DW_TILE");
  return !(e && e[0] == '0');
}

// Rows of a tile: the map's rows split evenly over the fewest tiles of at
// most DW_MAX_TH rows, then shrunk until lds(th) fits the budget.
template <typename F>
inline int dw_pick_rows(int rows, F lds) {
  int th = dw_ceil(rows, dw_ceil(rows, DW_MAX_TH));
  while (th > 1 && lds(th) > DW_LDS_BUDGET) --th;
  return th;
}

// x is [N, C, H, W]; the pass's other operand follows from the geometry.
inline DwRoute dwconv_route(bool bf16_nhwc, int64_t N, int64_t C, int64_t H,
                            int64_t W, int R, int S, int sh, int sw, int ph,
                            int pw, DwPass pass,
                            bool enabled = dw_tile_enabled()) {
  DwRoute r;
  if (!enabled || !bf16_nhwc || N < 1 || C < 8 || C % 8 != 0 || R != S ||
      (R != 3 && R != 5) || sh != sw || (sh != 1 && sh != 2) || ph < 0 ||
      pw < 0 || ph > R / 2 || pw > R / 2 || H + 2 * ph < R || W + 2 * pw < S ||
      H > (1 << 20) || W > (1 << 20))
    return r;
  const int st = sh;
  const int Ho = (int)((H + 2 * ph - R) / st + 1);
  const int Wo = (int)((W + 2 * pw - S) / st + 1);
  const int cpacks = (int)(C / 8);
  r.nchunk = dw_ceil(cpacks, DW_MAX_CP);
  r.CP = dw_ceil(cpacks, r.nchunk);
  const int nlanes = DW_THREADS / r.CP;
  const int wbytes = R * S * r.CP * 16;

  if (pass == DwPass::Dgrad && st == 2) {
    // 2x2 parity quads of gx over u = h + ph, v = w + pw; 8 quads wide
    const int qrows = dw_ceil(H + ph, 2), qcols = dw_ceil(W + pw, 2);
    auto lds = [&](int qh) {
      return wbytes + (qh + R / 2) * (8 + R / 2) * r.CP * 16;
    };
    const int qh = dw_pick_rows(qrows, lds);
    r.TH = 2 * qh;
    r.TW = 16;
    r.tilesH = dw_ceil(qrows, qh);
    r.tilesW = dw_ceil(qcols, 8);
    r.lds_bytes = lds(qh);
  } else {
    // fwd, stride-1 dgrad (the forward machine over gy) and wgrad share the
    // output-tile geometry; wgrad stages the gy tile next to the x patch
    const bool dg = pass == DwPass::Dgrad;
    const int OH = dg ? (int)H : Ho, OW = dg ? (int)W : Wo;
    r.TW = (st == 1 && OW > 8) ? 16 : 8;
    const int PW = (r.TW - 1) * st + R;
    auto lds = [&](int th, int nb = 1) {
      const int patch = ((th - 1) * st + R) * PW * r.CP * 16;
      if (pass == DwPass::Wgrad)
        return std::max(patch + th * r.TW * r.CP * 16, DW_RED_BYTES);
      return wbytes + nb * patch;
    };
    r.TH = dw_pick_rows(OH, [&](int th) { return lds(th); });
    r.tilesH = dw_ceil(OH, r.TH);
    r.tilesW = dw_ceil(OW, r.TW);
    // a map that is one tile: several images per block until the strips
    // cover the block's lanes
    const int strips = r.TH * (r.TW / (st == 1 ? 4 : 2));
    if (pass != DwPass::Wgrad && r.tilesH == 1 && r.tilesW == 1)
      while (r.NB < N && r.NB * strips < nlanes &&
             lds(r.TH, r.NB + 1) <= DW_LDS_BUDGET)
        ++r.NB;
    r.lds_bytes = lds(r.TH, r.NB);
  }
  if (r.lds_bytes > DW_LDS_BUDGET) return r;

  const int64_t items = (int64_t)dw_ceil(N, r.NB) * r.tilesH * r.tilesW;
  if (items * r.nchunk >= ((int64_t)1 << 31)) return r;
  if (pass == DwPass::Wgrad) {
    // enough blocks to fill the chip, a few hundred slots at the most; each
    // slot is a contiguous run of `per` (image, tile) items
    const int64_t want = std::clamp<int64_t>(
        dw_ceil(DW_FILL_BLOCKS, r.nchunk), 1, std::min<int64_t>(DW_MAX_SLOTS, items));
    const int64_t per = (items + want - 1) / want;
    r.slots = (int)((items + per - 1) / per);
  }
  r.tiled = true;
  return r;
}

// ---------------------------------------------------------------------------
// fp32 (depthwise_f32.hip; docs/ARCHITECTURE.md "Depthwise", fp32 subsection)
// ---------------------------------------------------------------------------
// A pack is four fp32 channels. 8 packs per chunk: 32 channels, one 128 B
// line per pixel, so the 40 KiB budget holds twice the pixels a 16-pack chunk
// would and a 5x5 tile keeps 8 output rows, not 2.
constexpr int DWF_MAX_CP = 8;
constexpr int DWF_MAX_TH = 16;  // two 1 x TW/2 strips per row: 32 per tile
constexpr int DWF_QW = 8;       // stride-2 dgrad: quads per tile row

// wgrad's end-of-run tree holds one tap row of every lane
constexpr int dwf_red_bytes(int R) { return DW_THREADS * R * 16; }

// Rows per tile as dw_pick_rows, then evened out again over the tiles left.
template <typename F>
inline int dwf_pick_rows(int rows, int max_th, F lds) {
  int th = dw_ceil(rows, dw_ceil(rows, max_th));
  while (th > 1 && lds(th) > DW_LDS_BUDGET) --th;
  return dw_ceil(rows, dw_ceil(rows, th));
}

// As dwconv_route, for fp32 NHWC x [N, C, H, W]. CP counts packs of 4
// channels; TW / 2 is the forward strip, TH / 2 the stride-2 dgrad's quad
// rows. The three passes of a conv are routed together (functional.conv2d
// asks all three), so a shape that loses is sent back here for every pass.
inline DwRoute dwconv_f32_route(bool f32_nhwc, int64_t N, int64_t C, int64_t H,
                                int64_t W, int R, int S, int sh, int sw,
                                int ph, int pw, DwPass pass,
                                bool enabled = dw_tile_enabled()) {
  DwRoute r;
  if (!enabled || !f32_nhwc || N < 1 || C < 4 || C % 4 != 0 || R != S ||
      (R != 3 && R != 5) || sh != sw || (sh != 1 && sh != 2) || ph < 0 ||
      pw < 0 || ph > R / 2 || pw > R / 2 || H + 2 * ph < R || W + 2 * pw < S ||
      H > (1 << 20) || W > (1 << 20))
    return r;
  const int st = sh;
  const int Ho = (int)((H + 2 * ph - R) / st + 1);
  const int Wo = (int)((W + 2 * pw - S) / st + 1);
  const int cpacks = (int)(C / 4);
  r.nchunk = dw_ceil(cpacks, DWF_MAX_CP);
  r.CP = dw_ceil(cpacks, r.nchunk);
  const int nlanes = DW_THREADS / r.CP;
  const int wbytes = R * S * r.CP * 16;

  if (pass == DwPass::Dgrad && st == 2) {
    // 2x2 parity quads of gx over u = h + ph, v = w + pw; a thread owns two
    // neighbouring quads, a tile is DWF_QW quads wide
    const int qrows = dw_ceil(H + ph, 2), qcols = dw_ceil(W + pw, 2);
    auto lds = [&](int qh) {
      return wbytes + (qh + R / 2) * (DWF_QW + R / 2) * r.CP * 16;
    };
    const int qh = dwf_pick_rows(qrows, DW_MAX_TH, lds);
    r.TH = 2 * qh;
    r.TW = 2 * DWF_QW;
    r.tilesH = dw_ceil(qrows, qh);
    r.tilesW = dw_ceil(qcols, DWF_QW);
    r.lds_bytes = lds(qh);
  } else {
    const bool dg = pass == DwPass::Dgrad;
    const int OH = dg ? (int)H : Ho, OW = dg ? (int)W : Wo;
    r.TW = (st == 1 && OW > 8) ? 16 : 8;
    const int PW = (r.TW - 1) * st + R;
    auto lds = [&](int th, int nb = 1) {
      const int patch = ((th - 1) * st + R) * PW * r.CP * 16;
      if (pass == DwPass::Wgrad)
        return std::max(patch + th * r.TW * r.CP * 16, dwf_red_bytes(R));
      return wbytes + nb * patch;
    };
    // wgrad's 1x4 pixel strips fill the lanes at 8 rows already
    r.TH = dwf_pick_rows(OH, pass == DwPass::Wgrad ? DW_MAX_TH : DWF_MAX_TH,
                         [&](int th) { return lds(th); });
    r.tilesH = dw_ceil(OH, r.TH);
    r.tilesW = dw_ceil(OW, r.TW);
    // a map that is one tile: several images per block until the strips
    // (two per row) cover the block's lanes
    if (pass != DwPass::Wgrad && r.tilesH == 1 && r.tilesW == 1)
      while (r.NB < N && r.NB * r.TH * 2 < nlanes &&
             lds(r.TH, r.NB + 1) <= DW_LDS_BUDGET)
        ++r.NB;
    r.lds_bytes = lds(r.TH, r.NB);
  }
  if (r.lds_bytes > DW_LDS_BUDGET) return r;

  const int64_t items = (int64_t)dw_ceil(N, r.NB) * r.tilesH * r.tilesW;
  if (items * r.nchunk >= ((int64_t)1 << 31)) return r;
  if (pass == DwPass::Wgrad) {
    const int64_t want = std::clamp<int64_t>(
        dw_ceil(DW_FILL_BLOCKS, r.nchunk), 1, std::min<int64_t>(DW_MAX_SLOTS, items));
    const int64_t per = (items + want - 1) / want;
    r.slots = (int)((items + per - 1) / per);
  }
  r.tiled = true;
  return r;
}
