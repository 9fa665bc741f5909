// Weight-gradient routing: the ONE place that decides how a bf16 wgrad is
// launched — tile family, split-m chunk length, chunk count and how the
// chunks' fp32 partial tiles meet. Plain C++17, no torch / HIP includes, so
// the table can be compiled and swept on a CPU. wgrad.hip executes what this
// header decides; docs/ARCHITECTURE.md "Weight gradient" prints the table.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>

constexpr int WG_STEP_PIX = 64;     // output pixels per k-step
constexpr int WG_CHUNK_STEPS = 64;  // k-steps per split-m chunk (4096 pixels)
constexpr int WG_MIN_CSTEPS = 8;    // floor of the runtime-csteps kernels
constexpr int WG_FILL_BLOCKS = 512; // shrink csteps until this many blocks
// Workspace cap of a [chunks][Kt*RSC] fp32 slab. Deterministic mode grows
// csteps of the runtime-csteps kernels (tr128, ring128) until it fits; the
// default mode keeps such a launch on the atomic accumulator instead.
constexpr int64_t WG_WS_CAP = (int64_t)64 << 20;

// Default-mode slab rule, set from the alternated kbench sweep of ResNet-50's
// batch-256 wgrad shapes (docs/ARCHITECTURE.md status entry 14 has the table).
// Slab traffic grows with chunks, so a slab launch stops shrinking csteps at
// 384 blocks (512 lost or tied on every shape, 256 lost 40 % on the 7x7 1x1s).
// With that, every tr128 / ring128 launch of the sweep, from 196 chunks x
// 128 KB (-3 %) over 98 x 256 KB (-29 %) down to 4 chunks x 9 MB (-6 %), beat
// the atomic chain in every pass; the two thresholds are the outermost of
// those values. The 64x64 tile's launches (196 chunks x 16-144 KB) lost by
// 3-6 %; that tile was measured at those small slots only, so it stays
// atomic whatever its shape.
constexpr int WG_SLAB_BLOCKS = 384;
constexpr int WG_SLAB_MAX_CHUNKS = 196;
constexpr int64_t WG_SLAB_MIN_SLOT_BYTES = (int64_t)128 << 10;

enum class WgradFamily { T64, Tr128, Ring128, Ring };
enum class WgradAcc { Atomic, Slab };

inline const char* wgrad_family_name(WgradFamily f) {
  switch (f) {
    case WgradFamily::T64: return "64x64";
    case WgradFamily::Tr128: return "tr128";
    case WgradFamily::Ring128: return "ring128";
    default: return "ring";
  }
}

inline const char* wgrad_acc_name(WgradAcc a) {
  return a == WgradAcc::Atomic ? "atomic" : "slab";
}

// DISTRIBUUUU_WGRAD_* switches, re-read on every call (A/B probes and tests
// flip them inside one process).
struct WgradGates {
  bool ring = false;  // WGRAD_RING=1: the opt-in 64x64 glds ring
  int f128 = -1;      // WGRAD_128: 1 forces ring128, 0 disables it
  int t128 = -1;      // WGRAD_T128: 1 forces tr128, 0 disables it
  // WGRAD_ACC: -1 auto, 0 atomic, 1 slab, -2 unknown value (the caller
  // rejects it). Ignored in deterministic mode.
  int acc = -1;
  // WGRAD_SLAB_BLOCKS: block-count target of the csteps shrink loop for a
  // slab launch (slab traffic grows with chunks, atomic traffic does not)
  int slab_blocks = WG_SLAB_BLOCKS;
};

inline WgradGates read_wgrad_gates() {
  WgradGates g;
  const char* e = getenv("DISTRIBUUUU_WGRAD_RING");
  g.ring = e && e[0] == '1';
  e = getenv("DISTRIBUUUU_WGRAD_128");
  g.f128 = e ? atoi(e) : -1;
  e = getenv("DISTRIBUUUU_WGRAD_T128");
  g.t128 = e ? atoi(e) : -1;
  e = getenv("DISTRIBUUUU_WGRAD_ACC");
  if (!e || !e[0] || strcmp(e, "auto") == 0) g.acc = -1;
  else if (strcmp(e, "atomic") == 0) g.acc = 0;
  else if (strcmp(e, "slab") == 0) g.acc = 1;
  else g.acc = -2;
  e = getenv("DISTRIBUUUU_WGRAD_SLAB_BLOCKS");
  if (e && atoi(e) > 0) g.slab_blocks = atoi(e);
  return g;
}

struct WgradRoute {
  WgradFamily family;
  int csteps;  // k-steps per chunk
  int chunks;  // split-m chunks = partial tiles per output element
  WgradAcc acc;
  int ktiles, ntiles;  // per group
};

inline int wgrad_chunks(int64_t M, int csteps) {
  const int64_t px = (int64_t)csteps * WG_STEP_PIX;
  return (int)((M + px - 1) / px);
}

// Deterministic mode: double csteps until the slab fits WG_WS_CAP (or one
// chunk is left).
inline int wgrad_grow_csteps(int csteps, int64_t M, int64_t slot_elems) {
  while (wgrad_chunks(M, csteps) > 1 &&
         (int64_t)wgrad_chunks(M, csteps) * slot_elems * 4 > WG_WS_CAP)
    csteps *= 2;
  return csteps;
}

// M = N*Ho*Wo output pixels; Kg / Cg per-group widths (multiples of 8).
inline WgradRoute wgrad_route(int64_t M, int Kg, int Cg, int R, int S,
                              int64_t groups, bool det,
                              const WgradGates& g = read_wgrad_gates()) {
  const int64_t RSC = (int64_t)R * S * Cg;
  const int64_t slot_elems = (int64_t)Kg * groups * RSC;
  const int chunks64 = wgrad_chunks(M, WG_CHUNK_STEPS);

  // ---- tile family -------------------------------------------------------
  WgradFamily fam = WgradFamily::T64;
  // measured: the 64x64 ring trails the tr-staged kernel on most shapes (its
  // 8-MFMA k-steps don't cover the pipeline); opt-in only
  const bool ring_ok = (M % 64 == 0) && (Kg % 64 == 0) &&
                       ((S * Cg) % 64 == 0) && (Cg % 8 == 0) &&
                       (RSC % 16 == 0);
  // 128x128 ring kernel where it measured faster (tools/probes/convmap.py):
  // 1x1 convolutions (no pad pass, B columns are plain channels) whose
  // launch has enough tiles+chunks to fill the 256 CUs, and GROUPED deep
  // 3x3s (RegNetY 232-wide groups — Kg tails are clamped/dropped). Dense 3x3
  // keeps the tr-staged kernels: pad pass + tap-spanning B columns cost more
  // than the glds staging saves.
  const int64_t blocks128 =
      (((int64_t)Kg + 127) / 128) * ((RSC + 127) / 128) * chunks64;
  const bool dense1x1 = R == 1 && S == 1 && Kg % 128 == 0 && Cg >= 128;
  // M >= 8192: measured crossover (tools/probes/wgrad_group_ab.py) — the
  // 7x7 grouped shapes stay on the 64x64 kernel (85 vs 118 us)
  const bool grouped_deep =
      groups > 1 && Kg >= 96 && RSC >= 512 && M >= 8192;
  const bool gate128 = (dense1x1 || grouped_deep) && blocks128 * groups >= 320;
  // measured (tools/probes/wgrad_dense_ab.py): tr128 wins/ties every dense
  // 3x3 with Kg >= 128 (512-deep: -13%), loses at Kg = 64 (half-empty tiles)
  const bool gate_t128 = Kg >= 128 && RSC >= 128;
  if (ring_ok && g.ring)
    fam = WgradFamily::Ring;
  else if (g.f128 != 0 && M % 64 == 0 && Cg % 8 == 0 &&
           (gate128 || g.f128 == 1))
    fam = WgradFamily::Ring128;
  else if (g.t128 == 1 || (g.t128 == -1 && gate_t128))
    fam = WgradFamily::Tr128;

  WgradRoute r;
  r.family = fam;
  const bool big = fam == WgradFamily::Tr128 || fam == WgradFamily::Ring128;
  const int tile = big ? 128 : 64;
  r.ktiles = (Kg + tile - 1) / tile;
  r.ntiles = (int)((RSC + tile - 1) / tile);

  // ---- split-m chunk -----------------------------------------------------
  // tr128 / ring128 take csteps at run time: shrink the chunk until the
  // launch fills the 256 CUs. The 64x64 kernels' chunk is a compile-time 64.
  auto shrink = [&](int target) {
    int cs = WG_CHUNK_STEPS;
    while (cs > WG_MIN_CSTEPS &&
           (int64_t)r.ktiles * r.ntiles * wgrad_chunks(M, cs) * groups < target)
      cs /= 2;
    return cs;
  };
  r.csteps = big ? shrink(WG_FILL_BLOCKS) : WG_CHUNK_STEPS;
  r.chunks = wgrad_chunks(M, r.csteps);
  r.acc = WgradAcc::Atomic;

  if (det) {  // slots + ordered_reduce always; the workspace is bounded
    if (big) {
      r.csteps = wgrad_grow_csteps(r.csteps, M, slot_elems);
      r.chunks = wgrad_chunks(M, r.csteps);
    }
    r.acc = WgradAcc::Slab;
    return r;
  }

  // ---- accumulate mode (default mode only) -------------------------------
  if (g.acc == 0) return r;
  const int cs = big ? shrink(g.slab_blocks) : WG_CHUNK_STEPS;
  const int ch = wgrad_chunks(M, cs);
  if ((int64_t)ch * slot_elems * 4 > WG_WS_CAP) return r;  // never grown here
  const bool pick =
      g.acc == 1 || (big && ch <= WG_SLAB_MAX_CHUNKS &&
                     slot_elems * 4 >= WG_SLAB_MIN_SLOT_BYTES);
  if (pick) {
    r.csteps = cs;
    r.chunks = ch;
    r.acc = WgradAcc::Slab;
  }
  return r;
}
