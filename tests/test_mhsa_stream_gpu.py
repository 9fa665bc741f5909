"""The streaming MHSA kernels (csrc/attention_stream.hip, 256 < L <= 1024)
against the float64 reference of mhsa_ref.py, entry points called directly in
the dense and the in-place NHWC layout, then through the MHSA module.

Forward: err(O) <= MARGIN * 3 U * O_abs, the bound mhsa_ref derives. Backward:
mhsa_ref's bounds at the exact float64 softmax plus the first-order terms of
recomputing P and of forming delta from the bf16 O (stream_bounds below;
derivation in docs/ARCHITECTURE.md, "Streaming attention")."""

import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhsa_ref as R  # noqa: E402
from test_mhsa_gpu import (_from_nhwc, _module_check, _nan,  # noqa: E402
                           _to_nhwc)

pytestmark = pytest.mark.gpu

# (H, W, D, B, large)
SHAPES = [
    (17, 16, 32, 2, False),   # L = 272: last q and key tile hold 16 rows; MH = 33
    (9, 29, 32, 2, False),    # L = 261: key tail of 5, non-square, MW = 57
    (32, 9, 64, 2, False),    # MH = 63, the widest table; two MFMA K-steps
    (24, 24, 128, 2, False),  # the 384 px shape: 9 full tiles, D at maximum
    (32, 32, 32, 1, False),   # the upper edge of the range
    (17, 16, 32, 2, True),    # row max moves from tile to tile: the rescale
]
_CASES = {}


def _sid(s):
    return f"{s[0]}x{s[1]}-d{s[2]}{'-large' if s[4] else ''}"


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _case(shape, layout="dense"):
    """Inputs, fp64 forward and backward reference with the streaming bounds:
    computed once per shape, shared by both layouts, never modified. The
    B = 1 shape runs with B = 2 in the two-head NHWC layout."""
    if layout == "nhwc" and shape[3] % 2:
        shape = shape[:3] + (2,) + shape[4:]
    if shape not in _CASES:
        H, W, D, B, large = shape
        c = R.make_case(H, W, D, B=B, seed=2000 + 10 * B + H + W + D,
                        large=large)
        ref = R.ref_forward(c)
        bref, bounds = R.ref_backward(c, ref["P"])
        _CASES[shape] = (c, ref, bref, stream_bounds(c, ref, bounds))
    return _CASES[shape]


def stream_bounds(c, ref, bounds):
    """mhsa_ref's backward bounds hold for an exact P. The streaming kernels
    use P^ = exp(S^ - lse^) = P (1 + relP) and delta^ = dO . O^ instead:
      relP   = g(D+3) S_abs + g(L) + g(4) (|S| + |lse|)
               (fp32 logit of D products, a scale and two adds; the L-term
               sum in lse; log, m + log l, S - lse and exp's argument)
      Edelta = (2 U + g(D)) sum_d |dO| O_abs   (O^: one rounding of P~, one
               of O, both within P |v|; the D-term fp32 dot)
      ES     = P (relP |dP - delta| + Edelta)  added to the error of dS
    and ES runs through the same linear maps as mhsa_ref's E_S. dV also takes
    P^ rounded to bf16: (P (U + relP))^T |dO|."""
    q, k, v, dO, rel_h, rel_w = c.f64()
    H, W, L, D, B, sc = c.H, c.W, c.L, c.D, c.B, c.scale
    iw, ih = R.rel_index(H, W)
    MW, MH = 2 * W - 1, 2 * H - 1
    U, g = R.U, R.g
    P, S = ref["P"], ref["S"]
    lse = torch.logsumexp(S, -1, keepdim=True)
    S_abs = (sc * q.abs() @ k.abs().transpose(1, 2)
             + R.gather_rel(ref["rw_abs"], iw) + R.gather_rel(ref["rh_abs"], ih))
    relP = g(D + 3) * S_abs + g(L) + g(4) * (S.abs() + lse.abs())
    dP = dO @ v.transpose(1, 2)
    delta = (dO * ref["O"]).sum(-1, keepdim=True)
    Edelta = ((2 * U + g(D)) * dO.abs() * ref["O_abs"]).sum(-1, keepdim=True)
    ES = P * (relP * (dP - delta).abs() + Edelta)
    Gw, Gh = R.scatter_rel(ES, iw, MW), R.scatter_rel(ES, ih, MH)
    qa = q.abs().reshape(B * L, D)
    extra = {
        "dv": (P * (U + relP)).transpose(1, 2) @ dO.abs(),
        "dk": sc * ES.transpose(1, 2) @ q.abs(),
        "dq": sc * (ES @ k.abs() + Gw @ rel_w.abs() + Gh @ rel_h.abs()),
        "grw": sc * Gw.reshape(B * L, MW).t() @ qa,
        "grh": sc * Gh.reshape(B * L, MH).t() @ qa,
    }
    return {n: bounds[n] + extra[n] for n in bounds}


def _cl(t, heads, H, W):
    """logical [N*heads, L, D] -> channels_last-contiguous [N, heads*D, H, W]"""
    t = _to_nhwc(t.cuda(), heads, H, W)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _run(c, layout):
    """fwd + bwd through the entry points; results as logical [B, L, D]."""
    e = _ext()
    B, L, D, H, W = c.B, c.L, c.D, c.H, c.W
    rel_h, rel_w = c.rel_h.cuda(), c.rel_w.cuda()
    if layout == "dense":
        heads, qpix, vpix, kqoff = 1, D, D, B * L * D
        q, k, v, dO = (t.cuda() for t in (c.q, c.k, c.v, c.dO))
        dqk, dv = _nan(2, B, L, D), _nan(B, L, D)
        back = lambda t: t  # noqa: E731
    else:
        heads = 2
        n, qpix, vpix, kqoff = B // heads, 2 * heads * D, heads * D, heads * D
        q = torch.cat([_cl(c.q, heads, H, W), _cl(c.k, heads, H, W)], dim=1)
        q = q.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        k = q.permute(0, 2, 3, 1).reshape(n * L, qpix)[:, heads * D:]
        v, dO = _cl(c.v, heads, H, W), _cl(c.dO, heads, H, W)
        dqk = _nan(n, H, W, qpix).permute(0, 3, 1, 2)
        dv = _nan(n, H, W, vpix).permute(0, 3, 1, 2)
        back = lambda t: _from_nhwc(t, heads)  # noqa: E731
    o, lse = e.mhsa_stream_fwd(q, k, v, rel_w, rel_h, L, H, W, heads, qpix,
                               qpix, vpix, c.scale, True)
    o2, none = e.mhsa_stream_fwd(q, k, v, rel_w, rel_h, L, H, W, heads, qpix,
                                 qpix, vpix, c.scale, False)
    assert lse.shape == (B, L) and none.numel() == 0 and torch.equal(o, o2)
    dqk, dv, grw, grh = e.mhsa_stream_bwd(
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
def test_stream_vs_fp64(shape, layout):
    c, ref, bref, bounds = _case(shape, layout)
    got = _run(c, layout)
    ratios = {"O": R._ratio(got["O"], ref["O"], 3 * R.U * ref["O_abs"])}
    ratios.update({n: R._ratio(got[n], bref[n], bounds[n]) for n in bref})
    print(f"{_sid(shape)}/{layout} err/bound: {R.fmt(ratios)}")
    assert not R.failures(ratios), R.failures(ratios)


@pytest.mark.parametrize("fmap", [(17, 16), (24, 24)])
def test_module_streams_without_fallback(fmap):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _module_check(fmap, fmap, seed=21, stages=8)
    assert not [w for w in rec if "falling back" in str(w.message)]


def test_stream_bwd_bit_reproducible():
    from distribuuuu_amd import ops

    c = _case(SHAPES[0])[0]
    ops.set_deterministic(True)
    try:
        a, b = _run(c, "dense"), _run(c, "dense")
    finally:
        ops.set_deterministic(False)
    for n in ("dq", "dk", "dv", "grw", "grh"):
        assert torch.equal(a[n], b[n]), n


def _args(fn, H=17, W=16, D=32, L=None, MW=None, qdtype=torch.bfloat16):
    """Consistent zero arguments of mhsa_stream_fwd / _bwd, B = 1, dense."""
    L = H * W if L is None else L
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, device="cuda", dtype=dt)  # noqa: E731
    q, t = z(1, L, D, dt=qdtype), z(1, L, D)
    rel_w, rel_h = z(2 * W - 1 if MW is None else MW, D), z(2 * H - 1, D)
    if fn == "fwd":
        return (q, t, t, rel_w, rel_h, L, H, W, 1, D, D, D, 1.0, True)
    return (t, t, z(1, L, dt=torch.float32), q, t, t, rel_w, rel_h, H, W, 1, D,
            L * D, D, D, 1.0, z(2, 1, L, D), z(1, L, D))


REJECTS = {
    "l_le_256": (dict(H=16, W=16), r"L must be in \(256, 1024\]"),
    "h_33": (dict(H=33, W=8), r"H and W must be in \[1, 32\]"),
    "d_16": (dict(D=16), "D must be 32, 64, 96 or 128"),
    "d_160": (dict(D=160), "D must be 32, 64, 96 or 128"),
    "l_ne_hw": (dict(L=273), r"L = 273 != H\*W = 272"),
    "rel_rows": (dict(MW=32), r"rel_w must be \[2W-1, D\]"),
    "q_fp32": (dict(qdtype=torch.float32), "q must be a bf16"),
}


@pytest.mark.parametrize("fn", ["fwd", "bwd"])
@pytest.mark.parametrize("name", list(REJECTS))
def test_stream_rejects(name, fn):
    """Every TORCH_CHECK precedes the first allocation and launch."""
    f = getattr(_ext(), f"mhsa_stream_{fn}")
    kw, msg = REJECTS[name]
    with pytest.raises(RuntimeError, match=f"mhsa_stream_{fn}: {msg}"):
        f(*_args(fn, **kw))
    f(*_args(fn))  # the unmodified call is accepted
    torch.cuda.synchronize()
