"""The MHSA kernels (csrc/attention.hip) against the float64 reference and the
derived componentwise bounds of mhsa_ref.py, at every tile shape, in the dense
and the in-place NHWC layout. The extension entry points are called directly,
so each stage is compared with the reference evaluated at that stage's own
inputs (the backward at the kernel's own bf16 pout). test_mhsa_ref_cpu.py
shows on the CPU that these bounds hold for correct rounding and fail for a
clobbered LDS row or H and W confused."""

import copy
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhsa_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
_CASES = {}
_WORST = {}


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _case(shape, layout, large=False):
    """Inputs and fp64 forward reference, one per (shape, layout), computed
    once and shared (never modified) by the tests that need it."""
    key = (shape, layout, large)
    if key not in _CASES:
        B = LAYOUTS[layout][1]
        seed = (1000 * list(LAYOUTS).index(layout) + 100 * large
                + R.SHAPES.index(shape))
        c = R.make_case(*shape, B=B, seed=seed, large=large)
        _CASES[key] = (c, R.ref_forward(c))
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nworst err/bound per output over this module:")
    for name, (r, where) in sorted(_WORST.items()):
        print(f"  {name:10s} {r:.3f}  at {where}")


def _note(ratios, where):
    for n, r in ratios.items():
        if n not in _WORST or not r <= _WORST[n][0]:
            _WORST[n] = (r, where)


def _check(ratios, where):
    print(f"{where} err/bound: {R.fmt(ratios)}")
    _note(ratios, where)
    assert not R.failures(ratios), (where, R.failures(ratios))


def _nan(*shape, dtype=torch.bfloat16):
    """Outputs start as NaN: an element the kernel never writes fails."""
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------
# the two layouts: run(c) -> (fwd, bwd) with fwd() -> dict(rw, rh, P, O,
# O_nograd) and bwd(P) -> dict(dq, dk, dv, grw, grh), all as logical [B, L, D]
# ---------------------------------------------------------------------------
def _dense(c):
    e = _ext()
    B, L, D, H, W = c.B, c.L, c.D, c.H, c.W
    q, k, v, dO, rel_h, rel_w = (t.cuda() for t in (c.q, c.k, c.v, c.dO,
                                                    c.rel_h, c.rel_w))
    vt = v.transpose(1, 2).contiguous()
    kt = k.transpose(1, 2).contiguous()

    def fwd():
        rw = e.mhsa_rel_tables(q, rel_w, B * L, 1, L, D, c.scale).reshape(B, L, -1)
        rh = e.mhsa_rel_tables(q, rel_h, B * L, 1, L, D, c.scale).reshape(B, L, -1)
        P = _nan(B, L, L)
        O = e.mhsa_fwd(q, k, vt, rw, rh, H, W, P, 1, D, D, c.scale)
        O2 = e.mhsa_fwd(q, k, vt, rw, rh, H, W, None, 1, D, D, c.scale)
        assert O.shape == (B, L, D) and O.is_contiguous()
        return {"rw": rw, "rh": rh, "P": P, "O": O, "O_nograd": O2}

    def bwd(P):
        dqk, dvb = _nan(2, B, L, D), _nan(B, L, D)
        dqk, dvb, grw, grh = e.mhsa_bwd(dO, P, q, kt, v, rel_w, rel_h, H, W, 1,
                                        D, B * L * D, D, D, c.scale, dqk, dvb)
        return {"dq": dqk[0], "dk": dqk[1], "dv": dvb, "grw": grw, "grh": grh}

    return fwd, bwd


def _to_nhwc(t, heads, H, W):
    """logical [N*heads, L, D] -> channels_last [N, heads*D, H, W]"""
    B, L, D = t.shape
    n = B // heads
    phys = t.reshape(n, heads, L, D).permute(0, 2, 1, 3).reshape(n, H, W, heads * D)
    return phys.permute(0, 3, 1, 2)


def _from_nhwc(t, heads):
    """channels_last [N, heads*D, H, W] -> logical [N*heads, L, D]"""
    n, C, H, W = t.shape
    return (t.permute(0, 2, 3, 1).reshape(n, H * W, heads, C // heads)
            .permute(0, 2, 1, 3).reshape(n * heads, H * W, C // heads))


def _is_cl(t):
    n, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).is_contiguous()  # physical [N, H, W, C]


def _nhwc(heads):
    def make(c):
        e = _ext()
        B, L, D, H, W = c.B, c.L, c.D, c.H, c.W
        n = B // heads
        qpix = 2 * heads * D
        vpix = heads * D
        rel_h, rel_w = c.rel_h.cuda(), c.rel_w.cuda()
        # as _HIPMHSARelPosNHWC: q and k halves of one [N, 2*heads*D, H, W]
        qk = torch.cat([_to_nhwc(c.q.cuda(), heads, H, W),
                        _to_nhwc(c.k.cuda(), heads, H, W)], dim=1)
        qk = qk.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        v = _to_nhwc(c.v.cuda(), heads, H, W)
        v = v.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        gout = _to_nhwc(c.dO.cuda(), heads, H, W)
        gout = gout.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert _is_cl(qk) and _is_cl(v) and _is_cl(gout)
        vt = c.v.cuda().transpose(1, 2).contiguous()
        kt = c.k.cuda().transpose(1, 2).contiguous()
        kview = qk.permute(0, 2, 3, 1).reshape(n * L, qpix)[:, heads * D:]

        def fwd():
            rw = e.mhsa_rel_tables(qk, rel_w, B * L, heads, L, qpix,
                                   c.scale).reshape(B, L, -1)
            rh = e.mhsa_rel_tables(qk, rel_h, B * L, heads, L, qpix,
                                   c.scale).reshape(B, L, -1)
            P = _nan(B, L, L)
            O = e.mhsa_fwd(qk, kview, vt, rw, rh, H, W, P, heads, qpix, qpix,
                           c.scale)
            O2 = e.mhsa_fwd(qk, kview, vt, rw, rh, H, W, None, heads, qpix,
                            qpix, c.scale)
            assert O.shape == (n, heads * D, H, W) and _is_cl(O)
            return {"rw": rw, "rh": rh, "P": P, "O": _from_nhwc(O, heads),
                    "O_nograd": _from_nhwc(O2, heads)}

        def bwd(P):
            dqk_out = _nan(n, H, W, qpix).permute(0, 3, 1, 2)
            dv_out = _nan(n, H, W, vpix).permute(0, 3, 1, 2)
            dqk_out, dv_out, grw, grh = e.mhsa_bwd(
                gout, P, qk, kt, v, rel_w, rel_h, H, W, heads, qpix, heads * D,
                vpix, vpix, c.scale, dqk_out, dv_out)
            assert dqk_out.shape == (n, qpix, H, W) and _is_cl(dqk_out)
            assert dv_out.shape == (n, vpix, H, W) and _is_cl(dv_out)
            # dq in channels [0, heads*D), dk in [heads*D, 2*heads*D)
            return {"dq": _from_nhwc(dqk_out[:, :heads * D], heads),
                    "dk": _from_nhwc(dqk_out[:, heads * D:], heads),
                    "dv": _from_nhwc(dv_out, heads), "grw": grw, "grh": grh}

        return fwd, bwd

    return make


# layout id -> (maker, B)
LAYOUTS = {"dense": (_dense, 3), "nhwc-h2": (_nhwc(2), 4), "nhwc-h3": (_nhwc(3), 3)}


def _run_case(shape, layout, large=False):
    make = LAYOUTS[layout][0]
    c, ref = _case(shape, layout, large)
    where = f"{R.shape_id(shape)}{'-large' if large else ''}/{layout}"
    fwd, bwd = make(c)
    f = fwd()
    torch.cuda.synchronize()
    # need_grad=False (pout=None) runs the same arithmetic
    assert torch.equal(f["O"], f["O_nograd"]), where
    fc = {n: t.cpu() for n, t in f.items()}
    ratios = R.forward_ratios(c, ref, fc)
    got = {n: t.cpu() for n, t in bwd(f["P"]).items()}
    assert got["grw"].shape == (2 * c.W - 1, c.D)
    assert got["grh"].shape == (2 * c.H - 1, c.D)
    ratios.update(R.backward_ratios(c, fc["P"], got))
    _check(ratios, where)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_mhsa_vs_fp64(shape, layout):
    _run_case(shape, layout)


@pytest.mark.parametrize("layout", ["dense", "nhwc-h2"])
@pytest.mark.parametrize("shape", R.LARGE_LOGIT_SHAPES, ids=R.shape_id)
def test_mhsa_large_logits(shape, layout):
    """|S| up to 60: the max subtraction and the fp32 tables."""
    _run_case(shape, layout, large=True)


@pytest.mark.parametrize("heads,B,L", [(1, 65, 253), (2, 66, 249)])
def test_rel_tables_second_grid_stride_trip(heads, B, L):
    """rows = B*L > 2048 blocks * 8 rows with rows % 8 != 0: the grid-stride
    loop's second trip and its ragged last row group. Tables kernel only."""
    e = _ext()
    D, M = 32, 31
    rows = B * L
    assert rows > 2048 * 8 and rows % 8 != 0
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(B, L, D, generator=gen).bfloat16()
    rel = torch.randn(M, D, generator=gen).bfloat16()
    scale = float(torch.tensor(D ** -0.5, dtype=torch.float32))
    if heads == 1:
        qg, qpix = q.cuda(), D
    else:  # q half of a [N, L, 2*heads*D] pixel-major buffer
        n, qpix = B // heads, 2 * heads * D
        qg = torch.zeros(n, L, qpix, dtype=torch.bfloat16)
        qg[:, :, :heads * D] = (q.reshape(n, heads, L, D).permute(0, 2, 1, 3)
                                .reshape(n, L, heads * D))
        qg = qg.cuda()
    out = e.mhsa_rel_tables(qg, rel.cuda(), rows, heads, L, qpix, scale)
    assert out.shape == (rows, M) and out.dtype == torch.float32
    q64, rel64 = q.double().reshape(rows, D), rel.double()
    ratio = R._ratio(out.cpu(), scale * q64 @ rel64.t(),
                     R.g(D) * scale * q64.abs() @ rel64.abs().t())
    _check({"rw": ratio}, f"rel_tables rows={rows} heads={heads}")


@pytest.mark.parametrize("shape", [(1, 16, 32), (5, 13, 32), (16, 16, 32)],
                         ids=R.shape_id)
def test_mhsa_bwd_deterministic(shape):
    """Deterministic mode: grw / grh meet the same bounds and repeat bit for
    bit (the switch as test_deterministic_gpu.py uses it)."""
    from distribuuuu_amd import ops

    make = LAYOUTS["dense"][0]
    c, ref = _case(shape, "dense")
    fwd, bwd = make(c)
    P = fwd()["P"]
    ops.set_deterministic(True)
    try:
        outs = [bwd(P) for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    for o in outs[1:]:
        for n in ("dq", "dk", "dv", "grw", "grh"):
            assert torch.equal(outs[0][n], o[n]), n
    got = {n: t.cpu() for n, t in outs[0].items()}
    _check(R.backward_ratios(c, P.cpu(), got),
           f"{R.shape_id(shape)}/dense-deterministic")


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------
U8 = 2.0 ** -8  # largest relative error of one bf16 rounding


def _module_pair(fmap, seed):
    from distribuuuu_amd.models.botnet import MHSA

    torch.manual_seed(seed)
    m = MHSA(64, fmap, heads=2, dim_qk=32, dim_v=32).bfloat16()
    ref = copy.deepcopy(m).double()  # the same bf16 parameter values
    return m.cuda(), ref


def _module_fwd_bwd(m, x, gout):
    x = x.detach().clone().requires_grad_(True)
    out = m(x)
    out.backward(gout)
    grads = {"x": x.grad, "to_qk": m.to_qk.weight.grad,
             "to_v": m.to_v.weight.grad, "rel_h": m.rel_h.grad,
             "rel_w": m.rel_w.grad}
    return out, grads


def _module_check(fmap, act, seed, stages=8):
    """MHSA module on the GPU (bf16, channels_last) against the same module
    composed by torch in float64 on the CPU from the same bf16 parameters.

    Bound: between the input and any of these results lie at most eight bf16
    roundings in series on the HIP path (qk / v, P, O; dO, dS, dq / dk / dv,
    the convs' grads, the parameter-dtype cast), each at most 2^-8 of its
    stage's magnitude; to first order they add, so every element is held to
    stages * 2^-8 of the reference's largest magnitude. The torch composition
    of the fallback rounds every intermediate to bf16 as well (q scale, three
    einsums, two adds, the softmax and the P@v einsum, and their autograd
    mirrors: 16 more), so it gets stages = 24. This is a normwise check of the
    module's plumbing (dispatch, layouts, gates): the componentwise bounds
    live in the entry-point tests above. A zeroed or misplaced row is an error
    of order 1.
    """
    m, ref = _module_pair(fmap, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    n = 2
    x = torch.randn(n, 64, *act, generator=gen).bfloat16()
    gout = torch.randn(n, 64, *act, generator=gen).bfloat16()
    cl = torch.channels_last
    out, grads = _module_fwd_bwd(m, x.cuda().contiguous(memory_format=cl),
                                 gout.cuda().contiguous(memory_format=cl))
    rout, rgrads = _module_fwd_bwd(ref, x.double(), gout.double())
    worst = {}
    for name, got, want in [("out", out, rout)] + [
            (k, grads[k], rgrads[k]) for k in grads]:
        assert got.shape == want.shape, name
        err = (got.detach().double().cpu() - want.detach()).abs().max().item()
        worst[name] = err / (stages * U8 * want.abs().max().item())
    print(f"MHSA module {fmap} on {act}: err / ({stages} * 2^-8 * max|ref|): "
          f"{R.fmt(worst)}")
    assert all(r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("fmap", [(4, 4), (12, 12)])
def test_module_vs_fp64_composition(fmap):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _module_check(fmap, fmap, seed=11)
    # the HIP path, not the composition
    assert not [w for w in rec if "falling back" in str(w.message)]


def test_module_out_of_range_map_falls_back_with_one_warning():
    from distribuuuu_amd.ops import dispatch

    dispatch._WARNED.discard(
        ("mhsa_relpos", "dtype torch.bfloat16 head_dim 32 map 17x3"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _module_check((17, 3), (17, 3), seed=12, stages=24)
        _module_check((17, 3), (17, 3), seed=13, stages=24)
    hits = [w for w in rec if "mhsa_relpos" in str(w.message)]
    assert len(hits) == 1, [str(w.message) for w in rec]
    assert "17x3" in str(hits[0].message)


def test_module_rejects_activation_of_another_size():
    m, _ = _module_pair((4, 4), seed=14)
    x = torch.randn(1, 64, 5, 5, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"5x5.*4x4"):
        m(x.contiguous(memory_format=torch.channels_last))


# ---------------------------------------------------------------------------
# host checks: every rejection happens before any launch (all TORCH_CHECKs of
# mhsa_fwd / mhsa_bwd precede their first allocation and launch)
# ---------------------------------------------------------------------------
def _fwd_args():
    B, H, W, D = 2, 2, 3, 32
    L = H * W
    bf = dict(device="cuda", dtype=torch.bfloat16)
    return {"q": torch.zeros(B, L, D, **bf), "k": torch.zeros(B, L, D, **bf),
            "vt": torch.zeros(B, D, L, **bf),
            "rw": torch.zeros(B, L, 2 * W - 1, device="cuda"),
            "rh": torch.zeros(B, L, 2 * H - 1, device="cuda"),
            "H": H, "W": W, "pout": torch.zeros(B, L, L, **bf), "heads": 1,
            "qpix": D, "kpix": D, "scale": 1.0}


def _bad_fwd(name):
    a = _fwd_args()
    B, L, D = a["q"].shape
    H, W = a["H"], a["W"]
    if name in ("q", "k", "vt"):
        a[name] = a[name].float()
    elif name == "hw_range":  # L == H*W still holds
        a.update(H=17, W=1, q=a["q"].new_zeros(B, 17, D),
                 k=a["q"].new_zeros(B, 17, D), vt=a["q"].new_zeros(B, D, 17),
                 rw=a["rw"].new_zeros(B, 17, 1), rh=a["rw"].new_zeros(B, 17, 33),
                 pout=None)
    elif name == "w_zero":
        a.update(H=L, W=0)
    elif name == "rw_cols":  # the square-map size of the same L would pass L
        a["rw"] = a["rw"].new_zeros(B, L, 2 * W)
    elif name == "rh_cols":
        a["rh"] = a["rh"].new_zeros(B, L, 2 * W - 1)
    elif name == "rw_dtype":
        a["rw"] = a["rw"].bfloat16()
    elif name == "rh_strided":
        a["rh"] = a["rh"].new_zeros(B, L, 2 * (2 * H - 1))[:, :, ::2]
    elif name == "pout_shape":
        a["pout"] = a["pout"].new_zeros(B, L, L + 2)
    elif name == "pout_dtype":
        a["pout"] = a["pout"].float()
    elif name == "heads":
        a["heads"] = 3  # B = 2
    return a


@pytest.mark.parametrize("name", ["q", "k", "vt", "hw_range", "w_zero",
                                  "rw_cols", "rh_cols", "rw_dtype",
                                  "rh_strided", "pout_shape", "pout_dtype",
                                  "heads"])
def test_mhsa_fwd_rejects(name):
    a = _bad_fwd(name)
    with pytest.raises(RuntimeError, match="mhsa|H\\*W"):
        _ext().mhsa_fwd(a["q"], a["k"], a["vt"], a["rw"], a["rh"], a["H"],
                        a["W"], a["pout"], a["heads"], a["qpix"], a["kpix"],
                        a["scale"])
    _ext().mhsa_fwd(*_fwd_args().values())  # the unmodified call is accepted
    torch.cuda.synchronize()


def _bwd_args(D=32):
    B, H, W = 2, 2, 3
    L = H * W
    bf = dict(device="cuda", dtype=torch.bfloat16)
    z = torch.zeros
    return {"dO": z(B, L, D, **bf), "P": z(B, L, L, **bf), "q": z(B, L, D, **bf),
            "kt": z(B, D, L, **bf), "v": z(B, L, D, **bf),
            "rel_w": z(2 * W - 1, D, **bf), "rel_h": z(2 * H - 1, D, **bf),
            "H": H, "W": W, "heads": 1, "qpix": D, "kqoff": B * L * D,
            "vpix": D, "opix": D, "scale": 1.0,
            "dqk": z(2, B, L, D, **bf), "dv": z(B, L, D, **bf)}


def _bad_bwd(name):
    if name == "d16":
        return _bwd_args(D=16)
    if name == "d160":
        return _bwd_args(D=160)
    a = _bwd_args()
    if name == "l_hw":
        a.update(H=3, W=3, rel_w=a["rel_w"].new_zeros(5, 32),
                 rel_h=a["rel_h"].new_zeros(5, 32))
    elif name == "rel_w_rows":
        a["rel_w"] = a["rel_w"].new_zeros(3, 32)
    elif name == "rel_h_rows":
        a["rel_h"] = a["rel_h"].new_zeros(5, 32)
    elif name == "rel_h_cols":
        a["rel_h"] = a["rel_h"].new_zeros(3, 64)
    elif name in ("P", "dO", "v"):
        a[name] = a[name].float()
    return a


@pytest.mark.parametrize("name", ["d16", "d160", "l_hw", "rel_w_rows",
                                  "rel_h_rows", "rel_h_cols", "P", "dO", "v"])
def test_mhsa_bwd_rejects(name):
    with pytest.raises(RuntimeError, match="mhsa_bwd"):
        _ext().mhsa_bwd(*_bad_bwd(name).values())
    _ext().mhsa_bwd(*_bwd_args().values())  # the unmodified call is accepted
    torch.cuda.synchronize()
