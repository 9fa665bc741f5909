// Conv routing: the environment gates and the ONE place that decides how a
// data-gradient is computed. Plain C++17, no torch / HIP includes, so the
// table can be compiled and swept on a CPU. conv.hip executes what this
// header decides; docs/ARCHITECTURE.md "Convolution" prints the table.
#pragma once

#include <cstdint>
#include <cstdlib>

// DISTRIBUUUU_* conv switches, read once per process (conv_gates()).
struct ConvGates {
  bool v2 = true;      // CONV_V2: the 3-slot glds ring kernel (conv2.hip)
  int v2_mink = 192;   // V2_MINK: ring minimum per-group output width
  // V2_MINRSC: ring minimum reduction depth R*S*Cg; below this the 3-slot
  // ring has too few k-steps to spin up
  int v2_minrsc = 512;
  // V2INTO_MINRSC: separate depth floor for the scatter/accumulate fwd_into
  // route (proj and residual-fork dgrads) so it can be swept independently
  // of the main forward dispatch; defaults to V2_MINRSC
  int v2into_minrsc = 512;
  bool v2into = true;  // CONV_V2INTO: ring for pad-free scatter windows
  bool small = true;   // CONV_SMALL: small 1x1 GEMM / K=64 patch kernels
  bool halo = true;    // CONV_HALO: LDS-staged 3x3 64->64 (conv_halo.hip)
};

inline ConvGates read_conv_gates() {
  auto on = [](const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
  };
  auto num = [](const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
  };
  ConvGates g;
  g.v2 = on("DISTRIBUUUU_CONV_V2");
  g.v2_mink = num("DISTRIBUUUU_V2_MINK", g.v2_mink);
  g.v2_minrsc = num("DISTRIBUUUU_V2_MINRSC", g.v2_minrsc);
  g.v2into_minrsc = num("DISTRIBUUUU_V2INTO_MINRSC", g.v2_minrsc);
  g.v2into = on("DISTRIBUUUU_CONV_V2INTO");
  g.small = on("DISTRIBUUUU_CONV_SMALL");
  g.halo = on("DISTRIBUUUU_CONV_HALO");
  return g;
}

inline const ConvGates& conv_gates() {
  static const ConvGates g = read_conv_gates();
  return g;
}

// Depth/width predicate of the v2 ring, shared by the forward gate and the
// dgrad gates: a per-group output wide enough for the 256x128 tile and a
// reduction deep enough to fill the pipeline (RegNetY's 232-wide groups
// qualify: Kg = 232, R*S*Cg = 2088).
inline bool v2_ring_ok(int Kg, int Cg, int R, int S, bool bf16,
                       const ConvGates& g = conv_gates()) {
  return g.v2 && Kg >= g.v2_mink && (int64_t)R * S * Cg >= g.v2_minrsc &&
         Cg % 8 == 0 && bf16;
}

enum class DgradKind { V2Same, Same, Strided1x1, Parity3x3, Dilate };

inline const char* dgrad_kind_name(DgradKind k) {
  switch (k) {
    case DgradKind::V2Same: return "V2Same";
    case DgradKind::Same: return "Same";
    case DgradKind::Strided1x1: return "Strided1x1";
    case DgradKind::Parity3x3: return "Parity3x3";
    default: return "Dilate";
  }
}

struct DgradRoute {
  DgradKind kind;
  int wkind;  // weight transform: 1 = span-padded flat flip, 0 = flipT
  bool acc;   // the epilogue adds into the caller's buffer
};

// The dgrad of a conv with weight [Kt0, Cg, R, S] is itself a conv over gy
// with per-group input width Kt0/groups and per-group output width Cg.
// `bf16` is the dtype of gy / w; `into_ok` says the caller offers a bf16
// channels_last accumulate buffer of exactly gx's shape.
inline DgradRoute dgrad_route(int64_t Kt0, int Cg, int R, int S, int sh,
                              int sw, int ph, int pw, int dh, int dw,
                              int64_t groups, bool bf16, bool into_ok,
                              const ConvGates& g = conv_gates()) {
  const int fCg = (int)(Kt0 / groups);  // the as-forward conv's Cg
  // stride 1 and any pad <= d*(R-1): the as-forward conv with pad
  // d*(R-1)-pad lands on the conv-input size exactly (pad 0 included: an
  // unpadded RxS conv's dgrad stays on the ring)
  const bool fits =
      sh == 1 && sw == 1 && dh * (R - 1) >= ph && dw * (S - 1) >= pw;
  // Kept difference: the v2 gate takes every `fits` shape, while the plain
  // Same route and every ACC epilogue also ask for R > 1 or zero padding.
  // The two differ only for R == 1, S > 1, pw > 0 (a 1x3 conv with pw = 1).
  const bool same_size = fits && (R > 1 || (ph == 0 && pw == 0));
  // Kept difference: the ACC epilogues are only offered to ungrouped bf16
  // convs (with groups == 1, fCg % 8 == 0 is also Kt0 % 8 == 0)
  const bool acc_ok = into_ok && bf16 && groups == 1 && fCg % 8 == 0;
  if (fits && Kt0 % (8 * groups) == 0 && v2_ring_ok(Cg, fCg, R, S, bf16, g))
    return {DgradKind::V2Same, 1, acc_ok && same_size};
  if (R == 1 && S == 1 && (sh > 1 || sw > 1) && ph == 0 && pw == 0)
    return {DgradKind::Strided1x1, 0, acc_ok};
  if (R == 3 && S == 3 && sh == 2 && sw == 2 && dh == 1 && dw == 1 &&
      ph == 1 && pw == 1)
    return {DgradKind::Parity3x3, 0, acc_ok};
  if (same_size && (groups == 1 || Kt0 % (8 * groups) == 0))
    return {DgradKind::Same, 0, acc_ok};
  return {DgradKind::Dilate, 0, false};
}
