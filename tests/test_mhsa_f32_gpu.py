"""The exact-fp32 MHSA kernels (csrc/attention_fp32.hip, maps up to 32x32)
against a float64 reference built from the same fp32 inputs: entry points
called directly in the dense and the in-place NHWC layout, then through the
MHSA module.

Bounds (docs/ARCHITECTURE.md, "fp32 attention"): elementwise, from the
reference's own absolute-value sums, with g(n) = n 2^-24 the first-order bound
of an n-term fp32 accumulation and no bf16 term anywhere:
  relP = g(D+3) S_abs + g(L) + g(4) (|S| + |lse|),  E_P = P relP
  O    E_P |v| + g(L + T + 2) O_abs              T = number of streamed tiles
  dV   E_P^T |dO| + g(L + 1) P^T |dO|
  dS   E_S = P (relP |dP - delta| + g(D+1) (|dO| |v|^T + sum_d |dO| O_abs))
             + g(2) |dS|
  dK, dQ, grw, grh: E_S through the backward's linear maps with every factor
       replaced by its absolute value, plus g(L + 1) (g(B L) for the table
       grads) times the same maps applied to |dS|
and err <= MARGIN * bound with mhsa_ref's MARGIN = 2. They are about 2^-15 of
the bf16 kernels' bounds: a path that rounds P or dS to bf16 fails by orders
of magnitude."""

import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhsa_ref as R  # noqa: E402
from test_mhsa_gpu import _from_nhwc, _nan, _to_nhwc  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, W, D, B, large): the smallest shapes at which each piece can go wrong
SHAPES = [
    (2, 3, 32, 2, False),      # one partial tile, M = 3 and 5
    (1, 16, 32, 2, False),     # a one-column table on one axis
    (16, 1, 32, 2, False),     # ... and on the other
    (8, 8, 32, 2, False),      # exactly one 64-row tile
    (5, 13, 64, 2, False),     # second tile has one row; two D blocks
    (17, 3, 96, 2, False),     # a side above 16 with L <= 256, 2H-1 = 33
    (14, 14, 128, 2, False),   # the flagship shape, D at maximum
    (32, 9, 32, 2, False),     # 2H-1 = 63, the widest table
    (32, 32, 32, 1, False),    # the upper edge; NHWC runs it with B = 2
    (17, 16, 32, 2, True),     # max |S| = 60: the row max moves between tiles
]
_CASES = {}


def _sid(s):
    return f"{s[0]}x{s[1]}-d{s[2]}{'-large' if s[4] else ''}"


def make_case(H, W, D, B, large):
    """fp32 randn inputs (mhsa_ref.make_case rounds to bf16), same gains."""
    gen = torch.Generator().manual_seed(3000 + 10 * B + H + W + D)
    L = H * W
    q, k, v, dO = (torch.randn(B, L, D, generator=gen) for _ in range(4))
    rel_h = 0.5 * torch.randn(2 * H - 1, D, generator=gen)
    rel_w = 0.5 * torch.randn(2 * W - 1, D, generator=gen)
    scale = float(np.float32(D ** -0.5))
    if large:
        S = R._logits64(q.double(), k.double(), rel_h.double(), rel_w.double(),
                        scale, H, W)[2]
        q = q * (R.LARGE_LOGIT / S.abs().max().item())
    else:
        q = q * (0.5 + 0.25 * math.log2(L))
    return R.Case(H, W, D, B, scale, q.float(), k, v, dO, rel_h, rel_w)


def reference(c):
    """float64 outputs and their bounds (module docstring) for a Case."""
    q, k, v, dO, rel_h, rel_w = c.f64()
    H, W, L, D, B, sc = c.H, c.W, c.L, c.D, c.B, c.scale
    iw, ih = R.rel_index(H, W)
    MW, MH = 2 * W - 1, 2 * H - 1
    g, t = R.g, lambda x: x.transpose(1, 2)  # noqa: E731
    S = R._logits64(q, k, rel_h, rel_w, sc, H, W)[2]
    P = torch.softmax(S, dim=-1)
    lse = torch.logsumexp(S, -1, keepdim=True)
    O_abs = P @ v.abs()
    S_abs = (sc * q.abs() @ t(k.abs())
             + R.gather_rel(sc * q.abs() @ rel_w.abs().t(), iw)
             + R.gather_rel(sc * q.abs() @ rel_h.abs().t(), ih))
    relP = g(D + 3) * S_abs + g(L) + g(4) * (S.abs() + lse.abs())
    EP = P * relP
    dP = dO @ t(v)
    delta = (dO * (P @ v)).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    ES = P * (relP * (dP - delta).abs() + g(D + 1) * (
        dO.abs() @ t(v.abs()) + (dO.abs() * O_abs).sum(-1, keepdim=True))
    ) + g(2) * dS.abs()

    def maps(x, q_, k_, rw_, rh_):  # the backward's linear maps of a dS
        Gw = R.scatter_rel(x, iw, MW).reshape(B * L, MW)
        Gh = R.scatter_rel(x, ih, MH).reshape(B * L, MH)
        dq = x @ k_ + (Gw @ rw_ + Gh @ rh_).reshape(B, L, D)
        return {"dk": sc * t(x) @ q_, "dq": sc * dq,
                "grw": sc * Gw.t() @ q_.reshape(B * L, D),
                "grh": sc * Gh.t() @ q_.reshape(B * L, D)}

    ref = maps(dS, q, k, rel_w, rel_h)
    absin = (q.abs(), k.abs(), rel_w.abs(), rel_h.abs())
    err, mag = maps(ES, *absin), maps(dS.abs(), *absin)
    bounds = {n: err[n] + g(B * L if n[0] == "g" else L + 1) * mag[n]
              for n in ref}
    ref.update(O=P @ v, dv=t(P) @ dO)
    bounds.update(O=EP @ v.abs() + g(L + (L + 63) // 64 + 2) * O_abs,
                  dv=t(EP) @ dO.abs() + g(L + 1) * (t(P) @ dO.abs()))
    return ref, bounds


def check(where, got, ref, bounds):
    ratios = {n: R._ratio(got[n], ref[n], bounds[n]) for n in ref}
    print(f"{where} err/bound: {R.fmt(ratios)}")
    assert not R.failures(ratios), (where, R.failures(ratios))


def _case(shape, layout="dense"):
    """Inputs and the float64 reference: computed once per shape, shared by
    the tests, never modified. The B = 1 shape runs with B = 2 in the
    two-head NHWC layout."""
    if layout == "nhwc" and shape[3] % 2:
        shape = shape[:3] + (2,) + shape[4:]
    if shape not in _CASES:
        c = make_case(*shape)
        _CASES[shape] = (c,) + reference(c)
    return _CASES[shape]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(t, heads, H, W):
    """logical [N*heads, L, D] -> channels_last-contiguous [N, heads*D, H, W]"""
    t = _to_nhwc(t.cuda(), heads, H, W)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _run(c, layout):
    """fwd + bwd through the entry points; results as logical [B, L, D]."""
    e = _ext()
    B, L, D, H, W = c.B, c.L, c.D, c.H, c.W
    f32 = torch.float32
    rel_h, rel_w = c.rel_h.cuda(), c.rel_w.cuda()
    if layout == "dense":
        heads, qpix, vpix, kqoff = 1, D, D, B * L * D
        q, k, v, dO = (t.cuda() for t in (c.q, c.k, c.v, c.dO))
        dqk, dv = _nan(2, B, L, D, dtype=f32), _nan(B, L, D, dtype=f32)
        back = lambda t: t  # noqa: E731
    else:
        heads = 2
        n, qpix, vpix, kqoff = B // heads, 2 * heads * D, heads * D, heads * D
        q = torch.cat([_cl(c.q, heads, H, W), _cl(c.k, heads, H, W)], dim=1)
        q = q.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        k = q.permute(0, 2, 3, 1).reshape(n * L, qpix)[:, heads * D:]
        v, dO = _cl(c.v, heads, H, W), _cl(c.dO, heads, H, W)
        dqk = _nan(n, H, W, qpix, dtype=f32).permute(0, 3, 1, 2)
        dv = _nan(n, H, W, vpix, dtype=f32).permute(0, 3, 1, 2)
        back = lambda t: _from_nhwc(t, heads)  # noqa: E731
    o, lse = e.mhsa_f32_fwd(q, k, v, rel_w, rel_h, L, H, W, heads, qpix, qpix,
                            vpix, c.scale, True)
    o2, none = e.mhsa_f32_fwd(q, k, v, rel_w, rel_h, L, H, W, heads, qpix,
                              qpix, vpix, c.scale, False)
    assert lse.shape == (B, L) and none.numel() == 0 and torch.equal(o, o2)
    dqk, dv, grw, grh = e.mhsa_f32_bwd(
        dO, o, lse, q, k, v, rel_w, rel_h, H, W, heads, qpix, kqoff, vpix,
        vpix, c.scale, dqk, dv)
    if layout == "dense":
        dq, dk = dqk[0], dqk[1]
    else:
        dq, dk = back(dqk[:, :heads * D]), back(dqk[:, heads * D:])
    got = {"O": back(o), "dq": dq, "dk": dk, "dv": back(dv), "grw": grw,
           "grh": grh}
    return {n: t.cpu() for n, t in got.items()}


@pytest.mark.parametrize("layout", ["dense", "nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_f32_vs_fp64(shape, layout):
    """Worst err / bound on MI355X over all shapes and both layouts: see the
    table in docs/ARCHITECTURE.md, "fp32 attention"."""
    c, ref, bounds = _case(shape, layout)
    check(f"{_sid(shape)}/{layout}", _run(c, layout), ref, bounds)


@pytest.mark.parametrize("fmap", [(14, 14), (17, 16)])
def test_module_routes_fp32_to_the_kernels(fmap):
    """An fp32 MHSA module: no fallback warning, and the attention it runs
    between its qkv convs and its output meets the bounds: the convs' outputs
    (and their grads) are captured, and the float64 reference starts from
    those very fp32 values."""
    from distribuuuu_amd.models.botnet import MHSA

    (H, W), heads, D, n = fmap, 2, 32, 2
    torch.manual_seed(31)
    m = MHSA(64, fmap, heads=heads, dim_qk=D, dim_v=D).cuda()
    x = torch.randn(n, 64, H, W, device="cuda").contiguous(
        memory_format=torch.channels_last).requires_grad_()
    kept = {}

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            kept[name] = out
        return hook

    m.to_qk.register_forward_hook(keep("qk"))
    m.to_v.register_forward_hook(keep("v"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = m(x)
        gout = torch.randn_like(out)
        out.backward(gout)
    assert not [w for w in rec if "falling back" in str(w.message)]
    assert x.grad is not None and torch.isfinite(x.grad).all()
    qk, v, hd = kept["qk"], kept["v"], heads * D
    lg = lambda t: _from_nhwc(t.detach().cpu(), heads)  # noqa: E731
    c = R.Case(H, W, D, n * heads, float(np.float32(m.scale)), lg(qk[:, :hd]),
               lg(qk[:, hd:]), lg(v), lg(gout), m.rel_h.detach().cpu(),
               m.rel_w.detach().cpu())
    got = {"O": lg(out), "dq": lg(qk.grad[:, :hd]), "dk": lg(qk.grad[:, hd:]),
           "dv": lg(v.grad), "grw": m.rel_w.grad.cpu(),
           "grh": m.rel_h.grad.cpu()}
    check(f"module {fmap}", got, *reference(c))


def test_f32_bwd_bit_reproducible():
    from distribuuuu_amd import ops

    c = _case(SHAPES[4])[0]
    ops.set_deterministic(True)
    try:
        a, b = _run(c, "dense"), _run(c, "dense")
    finally:
        ops.set_deterministic(False)
    for n in ("dq", "dk", "dv", "grw", "grh"):
        assert torch.equal(a[n], b[n]), n


def _args(fn, H=5, W=13, D=32, L=None, MW=None, qdtype=torch.float32):
    """Consistent zero arguments of mhsa_f32_fwd / _bwd, B = 1, dense."""
    L = H * W if L is None else L
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    q, t = z(1, L, D, dt=qdtype), z(1, L, D)
    rel_w, rel_h = z(2 * W - 1 if MW is None else MW, D), z(2 * H - 1, D)
    if fn == "fwd":
        return (q, t, t, rel_w, rel_h, L, H, W, 1, D, D, D, 1.0, True)
    return (t, t, z(1, L), q, t, t, rel_w, rel_h, H, W, 1, D, L * D, D, D, 1.0,
            z(2, 1, L, D), z(1, L, D))


REJECTS = {
    "q_bf16": (dict(qdtype=torch.bfloat16), "q must be an fp32"),
    "d_16": (dict(D=16), "D must be 32, 64, 96 or 128"),
    "d_160": (dict(D=160), "D must be 32, 64, 96 or 128"),
    "h_33": (dict(H=33, W=8), r"H and W must be in \[1, 32\]"),
    "l_ne_hw": (dict(L=66), r"L = 66 != H\*W = 65"),
    "rel_rows": (dict(MW=26), r"rel_w must be \[2W-1, D\]"),
}


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("name", list(REJECTS))
def test_f32_rejects(name, fn):
    """Every TORCH_CHECK precedes the first allocation and launch."""
    f = getattr(_ext(), f"mhsa_f32_{fn}")
    kw, msg = REJECTS[name]
    with pytest.raises(RuntimeError, match=f"mhsa_f32_{fn}: {msg}"):
        f(*_args(fn, **kw))
    f(*_args(fn))  # the unmodified call is accepted
    torch.cuda.synchronize()
