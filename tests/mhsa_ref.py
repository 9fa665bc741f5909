"""float64 reference, derived componentwise bounds and a rounding emulator for
the MHSA kernels (csrc/attention.hip). Shared by test_mhsa_ref_cpu.py (which
proves on the CPU that the bounds hold for correct rounding and catch the
known error classes) and test_mhsa_gpu.py (which holds the kernels to them).

Everything is written out from the formulas in the header of attention.hip:

  RW = scale q rel_w^T, RH = scale q rel_h^T              (fp32 tables)
  S[x, y] = scale q[x].k[y] + RW[x][wy-wx+W-1] + RH[x][hy-hx+H-1]
  P = softmax(S), O = P v
  dV = P^T dO, dP = dO v^T, dS = P (dP - rowsum(dP P))
  dRW[x, m] = sum_{y: wy-wx+W-1 == m} dS[x, y]   (G_w; dRH / G_h likewise)
  dQ = scale (dS k + dRW rel_w + dRH rel_h), dK = scale dS^T q
  grw = scale dRW^T q, grh = scale dRH^T q                (summed over B too)

with pixel x = hx * W + wx. Logical tensors are [B, L, D], B = N * heads.

Bounds. u = 2^-9 is the bf16 round-to-nearest unit, g(n) = n 2^-24 the
first-order bound of an n-term fp32 accumulation. Each bound is built from the
reference's own absolute-value sums at the points where the kernels round
(docs/ARCHITECTURE.md, Attention, has the table); every assertion is
err <= MARGIN * bound with MARGIN = 2 for the first-order terms dropped.
One term is added to the P bound of the derivation: 2^-126 absolute, because
__expf flushes results below the smallest normal fp32 to zero, so a reference
probability below it legitimately comes back as 0 (reached only by the
large-logit cases, where exp(-120) is a possible probability).
"""

import math
from dataclasses import dataclass

import numpy as np
import torch

U = 2.0 ** -9
MARGIN = 2.0
FP32_TINY = 2.0 ** -126

# softmax spread every ordinary case must have (checked in the CPU tests):
# the median over rows of max_y P[x, y] lies in this range, so the softmax is
# neither one-hot (every bound would collapse onto one term) nor flat.
ROWMAX_MEDIAN_RANGE = (0.05, 0.6)
LARGE_LOGIT = 60.0


def g(n):
    return n * 2.0 ** -24


# (H, W, D): every tile shape the kernels can take a different path at
SHAPES = [
    (2, 3, 32),      # one partial 16-tile, M = 3 and 5
    (4, 4, 32),      # LT 4, lpad 32: full-row spill before the fix
    (1, 16, 32),     # M = 1 (rel_grad upper half has no columns) and 31
    (16, 1, 32),
    (3, 11, 32),     # non-square both ways, lpad 64
    (11, 3, 32),
    (7, 7, 64),      # known-good length, nd = 2
    (8, 8, 32),      # exactly one q-tile, lpad = 16*LT
    (5, 13, 32),     # second q-tile has one row; LT 8, lpad 96
    (9, 9, 96),      # nd = 3, lpad 96
    (12, 12, 32),    # LT 13, lpad 160
    (13, 13, 32),    # LT 13, lpad 192
    (14, 14, 128),   # the flagship shape
    (13, 16, 32),    # LT 13 exactly full
    (14, 15, 64),    # LT 16, lpad 224
    (16, 16, 32),    # the maximum; M = 31 on both axes
]
LARGE_LOGIT_SHAPES = [(14, 14, 128), (4, 4, 32)]


def shape_id(s):
    return f"{s[0]}x{s[1]}-d{s[2]}"


def tile_geometry(L):
    """(LT, lpad) as the host code picks them."""
    lt16 = (L + 15) // 16
    LT = 4 if lt16 <= 4 else 8 if lt16 <= 8 else 13 if lt16 <= 13 else 16
    return LT, ((L + 31) // 32) * 32


def spill_cols(L):
    """Columns of the next LDS row an unguarded 16*LT-wide row store hits."""
    LT, lpad = tile_geometry(L)
    return max(0, 16 * LT - lpad)


_IDX = {}


def rel_index(H, W, row_stride=None):
    """Brute-force gather maps iw[x, y] = wy - wx + W - 1 and
    ih[x, y] = hy - hx + H - 1 for pixel x = hx * W + wx. row_stride = H
    decodes pixels with H and W confused (the injected error of the
    sensitivity tests); out-of-table indices are clamped, where a kernel
    would read its neighbour's memory."""
    rs = W if row_stride is None else row_stride
    key = (H, W, rs)
    if key not in _IDX:
        L = H * W
        iw = np.zeros((L, L), dtype=np.int64)
        ih = np.zeros((L, L), dtype=np.int64)
        for x in range(L):
            hx, wx = divmod(x, rs)
            for y in range(L):
                hy, wy = divmod(y, rs)
                iw[x, y] = min(max(wy - wx + W - 1, 0), 2 * W - 2)
                ih[x, y] = min(max(hy - hx + H - 1, 0), 2 * H - 2)
        _IDX[key] = (torch.from_numpy(iw), torch.from_numpy(ih))
    return _IDX[key]


def gather_rel(tab, idx):
    """tab [B, L, M], idx [L, L] -> [B, L, L]: out[b, x, y] = tab[b, x, idx[x, y]]"""
    return torch.gather(tab, 2, idx.unsqueeze(0).expand(tab.shape[0], -1, -1))


def scatter_rel(ds, idx, M):
    """The gather-sum G: out[b, x, m] = sum_{y: idx[x, y] == m} ds[b, x, y]."""
    out = torch.zeros(ds.shape[0], ds.shape[1], M, dtype=ds.dtype)
    return out.scatter_add_(2, idx.unsqueeze(0).expand(ds.shape[0], -1, -1), ds)


@dataclass
class Case:
    H: int
    W: int
    D: int
    B: int
    scale: float          # exactly the fp32 value the kernels get
    q: torch.Tensor       # bf16 [B, L, D]
    k: torch.Tensor
    v: torch.Tensor
    dO: torch.Tensor
    rel_h: torch.Tensor   # bf16 [2H-1, D]
    rel_w: torch.Tensor   # bf16 [2W-1, D]

    @property
    def L(self):
        return self.H * self.W

    def f64(self):
        return tuple(t.double() for t in (self.q, self.k, self.v, self.dO,
                                          self.rel_h, self.rel_w))


def _logits64(q, k, rel_h, rel_w, scale, H, W):
    iw, ih = rel_index(H, W)
    RW = scale * q @ rel_w.t()
    RH = scale * q @ rel_h.t()
    S = scale * q @ k.transpose(1, 2) + gather_rel(RW, iw) + gather_rel(RH, ih)
    return RW, RH, S


def make_case(H, W, D, B, seed, large=False):
    """randn inputs in bf16. q carries a gain that puts the softmax in
    ROWMAX_MEDIAN_RANGE at every listed L (a longer row needs larger logits
    to be as far from flat), or, with large=True, the largest |S| at
    LARGE_LOGIT."""
    gen = torch.Generator().manual_seed(seed)
    L = H * W

    def rn(*s):
        return torch.randn(*s, generator=gen)

    q, k, v, dO = rn(B, L, D), rn(B, L, D), rn(B, L, D), rn(B, L, D)
    rel_h, rel_w = 0.5 * rn(2 * H - 1, D), 0.5 * rn(2 * W - 1, D)
    scale = float(np.float32(D ** -0.5))
    k, v, dO, rel_h, rel_w = (t.bfloat16() for t in (k, v, dO, rel_h, rel_w))
    if large:
        _, _, S = _logits64(q.double(), k.double(), rel_h.double(),
                            rel_w.double(), scale, H, W)
        q = q * (LARGE_LOGIT / S.abs().max().item())
    else:
        q = q * (0.5 + 0.25 * math.log2(L))
    return Case(H, W, D, B, scale, q.bfloat16(), k, v, dO, rel_h, rel_w)


def ref_forward(c):
    q, k, v, _, rel_h, rel_w = c.f64()
    RW, RH, S = _logits64(q, k, rel_h, rel_w, c.scale, c.H, c.W)
    P = torch.softmax(S, dim=-1)
    return {"rw": RW, "rh": RH, "S": S, "P": P, "O": P @ v,
            "rw_abs": c.scale * q.abs() @ rel_w.abs().t(),
            "rh_abs": c.scale * q.abs() @ rel_h.abs().t(),
            "O_abs": P @ v.abs()}


def _ratio(got, ref, bound):
    """Worst err / bound over the elements (0/0 counts as 0)."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.nan_to_num(r, nan=math.inf, posinf=math.inf).max().item()


def forward_ratios(c, ref, got):
    """got: rw, rh (fp32 [B, L, M]), P (bf16 [B, L, L]), O (bf16 [B, L, D]).
    Returns the worst err / bound per output."""
    v = c.v.double()
    L, D = c.L, c.D
    Pk = got["P"].double()
    Ostar = Pk @ v
    return {
        "rw": _ratio(got["rw"], ref["rw"], g(D) * ref["rw_abs"]),
        "rh": _ratio(got["rh"], ref["rh"], g(D) * ref["rh_abs"]),
        "P": _ratio(got["P"], ref["P"], 2 * U * ref["P"] + FP32_TINY),
        "O_given_P": _ratio(got["O"], Ostar,
                            U * Ostar.abs() + g(L) * (Pk @ v.abs())),
        "O": _ratio(got["O"], ref["O"], 3 * U * ref["O_abs"]),
    }


def ref_backward(c, P):
    """Backward from the given probabilities (the kernel's own bf16 pout), in
    float64, plus the bounds of every output."""
    q, k, v, dO, rel_h, rel_w = c.f64()
    H, W, L, D, B, sc = c.H, c.W, c.L, c.D, c.B, c.scale
    iw, ih = rel_index(H, W)
    MW, MH = 2 * W - 1, 2 * H - 1
    P = P.double()
    dV = P.transpose(1, 2) @ dO
    dP = dO @ v.transpose(1, 2)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dRW, dRH = scatter_rel(dS, iw, MW), scatter_rel(dS, ih, MH)
    dQ = sc * (dS @ k + dRW @ rel_w + dRH @ rel_h)
    dK = sc * dS.transpose(1, 2) @ q
    qf = q.reshape(B * L, D)
    grw = sc * dRW.reshape(B * L, MW).t() @ qf
    grh = sc * dRH.reshape(B * L, MH).t() @ qf

    E_S = U * dS.abs() + g(D + L) * P * (
        dO.abs() @ v.abs().transpose(1, 2)
        + (dP.abs() * P).sum(-1, keepdim=True))
    GwE, GhE = scatter_rel(E_S, iw, MW), scatter_rel(E_S, ih, MH)
    qa = qf.abs()
    bounds = {
        "dv": U * dV.abs() + g(L) * (P.transpose(1, 2) @ dO.abs()),
        "dk": sc * (E_S.transpose(1, 2) @ q.abs()) + U * dK.abs(),
        "dq": sc * (E_S @ k.abs() + (GwE + U * dRW.abs()) @ rel_w.abs()
                    + (GhE + U * dRH.abs()) @ rel_h.abs()) + U * dQ.abs(),
        "grw": sc * (GwE.reshape(B * L, MW).t() @ qa)
               + g(B * L) * sc * (dRW.abs().reshape(B * L, MW).t() @ qa),
        "grh": sc * (GhE.reshape(B * L, MH).t() @ qa)
               + g(B * L) * sc * (dRH.abs().reshape(B * L, MH).t() @ qa),
    }
    return {"dv": dV, "dk": dK, "dq": dQ, "grw": grw, "grh": grh}, bounds


def backward_ratios(c, P, got):
    """got: dq, dk, dv (bf16 [B, L, D]), grw, grh (fp32 [M, D])."""
    ref, bounds = ref_backward(c, P)
    return {n: _ratio(got[n], ref[n], bounds[n]) for n in ref}


def failures(ratios):
    return {n: r for n, r in ratios.items() if not r <= MARGIN}


def fmt(ratios):
    return " ".join(f"{n}={r:.3f}" for n, r in ratios.items())


# ---------------------------------------------------------------------------
# Rounding emulator: the kernels' arithmetic in torch fp32 on the CPU, rounded
# where they round (bf16 at P, dS, the LDS copies of dRW/dRH and the outputs;
# fp32 tables, drw/drh and grw/grh).
# ---------------------------------------------------------------------------
def _clobber(t, L):
    """What the unguarded LDS row store did: rows 3, 7, 11 of each 16-row
    wave tile wrote their zero pad columns over the first 16*LT - lpad
    columns of rows 4, 8, 12, which were already in place."""
    n = spill_cols(L)
    t = t.clone()
    rows = [r for r in range(L) if r % 16 in (4, 8, 12)]
    if n and rows:
        t[:, rows, :min(n, L)] = 0
    return t


def emulate(c, clobber=False, swap_hw=False):
    H, W, L, D, B, sc = c.H, c.W, c.L, c.D, c.B, np.float32(c.scale).item()
    q, k, v, dO, rel_h, rel_w = (t.float() for t in (c.q, c.k, c.v, c.dO,
                                                     c.rel_h, c.rel_w))
    iw, ih = rel_index(H, W, row_stride=H if swap_hw else None)
    MW, MH = 2 * W - 1, 2 * H - 1
    rw = (q @ rel_w.t()) * sc
    rh = (q @ rel_h.t()) * sc
    S = (q @ k.transpose(1, 2)) * sc + (gather_rel(rw, iw) + gather_rel(rh, ih))
    e = torch.exp(S - S.max(-1, keepdim=True).values)
    P = (e * (1.0 / e.sum(-1, keepdim=True))).bfloat16()
    P_lds = _clobber(P, L) if clobber else P
    O = (P_lds.float() @ v).bfloat16()

    Pf = P.float()
    dP = dO @ v.transpose(1, 2)
    dS = (Pf * (dP - (dP * Pf).sum(-1, keepdim=True))).bfloat16()
    dS_lds = (_clobber(dS, L) if clobber else dS).float()
    drw, drh = scatter_rel(dS_lds, iw, MW), scatter_rel(dS_lds, ih, MH)
    dq = ((dS_lds @ k + drw.bfloat16().float() @ rel_w
           + drh.bfloat16().float() @ rel_h) * sc).bfloat16()
    dk = ((dS.float().transpose(1, 2) @ q) * sc).bfloat16()
    dv = (Pf.transpose(1, 2) @ dO).bfloat16()
    qf = q.reshape(B * L, D)
    grw = (drw.reshape(B * L, MW).t() @ qf) * sc
    grh = (drh.reshape(B * L, MH).t() @ qf) * sc
    return {"rw": rw, "rh": rh, "P": P, "O": O, "dq": dq, "dk": dk, "dv": dv,
            "grw": grw, "grh": grh}
