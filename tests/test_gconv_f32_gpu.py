"""Exact-fp32 narrow-group conv kernels (csrc/gconv_tile_f32.hip) vs float64.

Every case is on the tiled route (asserted) and is compared elementwise with
F.conv2d(groups=g) and its autograd in float64 on the CPU, on the exact fp32
inputs. The bound is derived, not measured: any-order fp32 summation of n
products errs by less than 2 n 2^-24 A, with n the terms of the output's sum
(fwd and dgrad: 9 w, wgrad: N*Ho*Wo) and A the same sum over absolute values
(the reference run on |x|, |w|, |gy|). Zero-filled terms add exact zeros. One
bf16 rounding on the path (2^-9 relative) breaks it by orders of magnitude.
"""

import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# Per width: a group count that leaves the last 32-channel block part empty
# (C = 24, 40, 48, 96) and one that makes C = 160 (several chunks).
GROUPS = {4: (6, 40), 8: (5, 20), 16: (3, 10), 32: (3, 5)}
# (N, groups, w, H, W, stride, pad)
CASES = [c for w, (ga, gb) in GROUPS.items() for c in [
    (2, ga, w, 1, 1, 1, 1),  # a map smaller than the filter
    (3, gb, w, 37, 19, 1, 1),  # ragged tiles on both axes
    (2, ga, w, 37, 19, 2, 1), (2, gb, w, 38, 20, 2, 1),  # odd / even extents
    (2, ga, w, 20, 20, 1, 0), (2, ga, w, 21, 21, 2, (1, 0)),  # pads
]]
# the only stride-2 map whose w = 32 weight gradient stays on the tiled route
CASES.append((2, 3, 32, 9, 13, 2, 1))
PASSES = ("fwd", "dgrad", "wgrad")


def _wgrad_gated(w, s, out):
    """The weight gradients gconv_f32_route sends back to conv2d_wgrad (the
    measured losers, pinned in tests/test_gconv_f32_route.py)."""
    return ((w == 32 and s == 2 and out >= 49)
            or (w == 16 and s == 2 and out >= 784)
            or (w == 32 and s == 1 and out < 196))


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(case):
    n, g, w, h, wd, s, p = case
    p = p if isinstance(p, tuple) else (p, p)
    torch.manual_seed(sum(case[:6]) + sum(p))
    ho, wo = (h + 2 * p[0] - 3) // s + 1, (wd + 2 * p[1] - 3) // s + 1
    return (_cl(torch.randn(n, g * w, h, wd)), _cl(torch.randn(g * w, w, 3, 3)),
            _cl(torch.randn(n, g * w, ho, wo)), s, p, g)


def _ref64(x, wt, gy, s, p, g):
    """(y, gx, gw) in float64 on the CPU."""
    x, wt = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv2d(x, wt, None, s, p, 1, g)
    gx, gw = torch.autograd.grad(y, (x, wt), gy.double())
    return y.detach(), gx, gw


def _check(name, got, ref, mag, n):
    assert got.dtype == torch.float32 and got.shape == ref.shape, name
    err = (got.double().cpu() - ref).abs()
    bound = 2 * n * 2.0 ** -24 * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, err - bound {worst:.3e}")
    assert worst <= 0, name


def _check3(got, x, wt, gy, s, p, g):
    ref = _ref64(x, wt, gy, s, p, g)
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p, g)
    k = 9 * wt.shape[1]
    terms = (k, k, gy.numel() // gy.shape[1])
    for name, got_, rf, m, n in zip(PASSES, got, ref, mag, terms):
        if got_ is not None:
            _check(name, got_, rf, m, n)


def _run(e, x, wt, gy, s, p, g):
    """The three passes on the tiled route; None for a gated weight gradient,
    which is not this family's."""
    gated = _wgrad_gated(wt.shape[1], s, gy.shape[2] * gy.shape[3])
    for pass_ in PASSES:
        want = "generic" if gated and pass_ == "wgrad" else "tile"
        assert e.gconv_f32_route(x, x.shape[1], g, 3, 3, s, s, *p, 1, 1,
                                 pass_)[0] == want, pass_
    return (e.gconv_f32_fwd(x, wt, s, s, *p, g),
            e.gconv_f32_dgrad(gy, wt, x.shape[2], x.shape[3], s, s, *p, g),
            None if gated else e.gconv_f32_wgrad(gy, x, s, s, *p, g))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tiled_vs_fp64(case):
    x, wt, gy, s, p, g = _inputs(case)
    got = _run(_ext(), x.cuda(), wt.cuda(), gy.cuda(), s, p, g)
    assert got[2] is None or got[2].shape == wt.shape
    _check3(got, x, wt, gy, s, p, g)


def test_wgrad_many_items():
    """More (image, tile) items than slots: a block accumulates over a run of
    tiles across image seams, ordered_reduce sums many slots."""
    e = _ext()
    x, wt, gy, s, p, g = _inputs((60, 5, 32, 17, 33, 1, 1))
    route, th, _, _, per, slots, _ = e.gconv_f32_route(
        x, 160, g, 3, 3, s, s, *p, 1, 1, "wgrad")
    tiles = -(-17 // th) * 3
    assert route == "tile" and per > 1 and tiles % per != 0
    assert 1 < slots < 60 * tiles
    ref = _ref64(x, wt, gy, s, p, g)[2]
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p, g)[2]
    gw = e.gconv_f32_wgrad(gy.cuda(), x.cuda(), s, s, *p, g)
    _check("wgrad", gw, ref, mag, 60 * 17 * 33)


@pytest.mark.parametrize("case", [(3, 20, 8, 37, 19, 1, 1),
                                  (2, 3, 32, 37, 19, 2, 1)], ids=str)
def test_bn_partials(case):
    """Partial rows sum to the column sums of the kernel's own y and y^2:
    any-order fp32 sums of M terms, held to 2 M 2^-24 of the absolute sum."""
    e = _ext()
    x, wt, _, s, p, g = _inputs(case)
    y, part = e.gconv_f32_fwd_bn(x.cuda(), wt.cuda(), s, s, *p, g)
    c = x.shape[1]
    assert part.dtype == torch.float32 and part.shape[1] == 2 * c
    assert torch.equal(y, e.gconv_f32_fwd(x.cuda(), wt.cuda(), s, s, *p, g))
    yd = y.double().cpu()
    m = yd.numel() // c
    got = part.double().sum(0).cpu()
    for name, g_, ref, mag in (
            ("sum", got[:c], yd.sum((0, 2, 3)), yd.abs().sum((0, 2, 3))),
            ("sumsq", got[c:], (yd * yd).sum((0, 2, 3)),
             (yd * yd).sum((0, 2, 3)))):
        worst = ((g_ - ref).abs() - 2 * m * 2.0 ** -24 * mag).max().item()
        print(f"{name}: err - bound {worst:.3e}")
        assert worst <= 0, name


def test_functional_autograd():
    from distribuuuu_amd import ops
    from distribuuuu_amd.ops import functional as DF

    x, wt, gy, s, p, g = _inputs((3, 10, 16, 37, 19, 2, 1))
    assert DF._gconv_tiled(x.cuda(), wt.cuda(), (s, s), p, (1, 1),
                           g) == "gconv_f32"
    was = ops.get_fp32_precision()
    out = {}
    try:
        for mode in ("highest", "high"):
            ops.set_fp32_precision(mode)
            xg, wg = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                y = DF.conv2d(xg, wg, None, (s, s), p, (1, 1), g)
                y.backward(gy.cuda())
            assert not [w for w in caught if "fall" in str(w.message)]
            torch.cuda.synchronize()
            out[mode] = (y.detach(), xg.grad, wg.grad)
    finally:
        ops.set_fp32_precision(was)
    assert out["highest"][2].shape == wt.shape
    _check3(out["highest"], x, wt, gy, s, p, g)
    for name, a, b in zip(PASSES, out["highest"], out["high"]):
        assert torch.equal(a, b), f"{name} differs under fp32 precision high"


def _nan_backed(t):
    """The same NHWC tensor at the front of a larger NaN-filled storage."""
    n, c, h, w = t.shape
    buf = torch.full((t.numel() + 3 * c * (w + 2) * 8,), float("nan"),
                     dtype=t.dtype, device=t.device)
    v = buf[:t.numel()].view(n, h, w, c).permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.is_contiguous(memory_format=torch.channels_last)
    return v


def test_bits_repeat_and_halo_is_zero_fill():
    e = _ext()
    x, wt, gy, s, p, g = (t.cuda() if torch.is_tensor(t) else t
                          for t in _inputs((2, 5, 8, 38, 20, 2, 1)))
    a = _run(e, x, wt, gy, s, p, g)
    b = _run(e, x, wt, gy, s, p, g)
    c = _run(e, _nan_backed(x), wt, _nan_backed(gy), s, p, g)
    for name, u, v, z in zip(PASSES, a, b, c):
        assert torch.equal(u, v), f"{name} bits differ between two calls"
        assert torch.equal(u, z), f"{name} read past the image"
