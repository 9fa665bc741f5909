"""Exact-fp32 LDS-tiled depthwise kernels (csrc/depthwise_f32.hip) vs float64.

Every case is on the tiled route (asserted) and is compared elementwise with
F.conv2d(groups=C) and its autograd in float64 on the CPU, evaluated on the
exact fp32 inputs. The bound is derived, not measured: any-order fp32
summation of n products errs by at most gamma_n * A with gamma_n < 2 n 2^-24,
so every element is held to

    err <= 2 * n * 2^-24 * A

with n the number of terms of the output's sum (fwd and dgrad: R*S, wgrad:
N*Ho*Wo) and A the same sum over absolute values (the reference run on |x|,
|w|, |gy|). One bf16 rounding anywhere on the path (2^-9 relative) breaks it
by orders of magnitude.
"""

import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, C, H, W, R, stride, pad)
CASES = [
    # one pack, map smaller than the filter
    (2, 4, 1, 1, 3, 1, 1), (1, 4, 2, 3, 5, 2, 2),
    # ragged tiles on both axes, 5 packs, image seams in a wgrad run
    (3, 20, 37, 19, 3, 1, 1), (3, 20, 37, 19, 5, 1, 2),
    # stride 2, odd and even extents: all four dgrad parity classes
    (2, 12, 37, 19, 3, 2, 1), (2, 12, 38, 20, 5, 2, 2),
    # 17 packs: ragged last chunk, whole-image tiles, several images per block
    (2, 68, 14, 14, 5, 1, 2), (2, 68, 7, 7, 3, 2, 1),
    # pad 0 and unequal pads
    (2, 8, 20, 20, 3, 1, 0), (2, 8, 20, 20, 5, 1, (2, 0)),
]
PASSES = ("fwd", "dgrad", "wgrad")


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(case):
    n, c, h, w, r, s, p = case
    p = p if isinstance(p, tuple) else (p, p)
    torch.manual_seed(sum(case[:6]) + sum(p))
    ho, wo = (h + 2 * p[0] - r) // s + 1, (w + 2 * p[1] - r) // s + 1
    return (_cl(torch.randn(n, c, h, w)), _cl(torch.randn(c, 1, r, r)),
            _cl(torch.randn(n, c, ho, wo)), s, p)


def _ref64(x, wt, gy, s, p):
    """(y, gx, gw) in float64 on the CPU."""
    x, wt = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv2d(x, wt, None, s, p, 1, x.shape[1])
    gx, gw = torch.autograd.grad(y, (x, wt), gy.double())
    return y.detach(), gx, gw


def _check(name, got, ref, mag, n):
    assert got.dtype == torch.float32 and got.shape == ref.shape, name
    err = (got.double().cpu() - ref).abs()
    bound = 2 * n * 2.0 ** -24 * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, err - bound {worst:.3e}")
    assert worst <= 0, name


def _check3(got, x, wt, gy, s, p):
    ref = _ref64(x, wt, gy, s, p)
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p)
    rr = wt.shape[2] * wt.shape[3]
    terms = (rr, rr, gy.numel() // gy.shape[1])
    for name, g, rf, m, n in zip(PASSES, got, ref, mag, terms):
        _check(name, g, rf, m, n)


def _run(e, x, wt, gy, s, p):
    r = wt.shape[2]
    for pass_ in PASSES:
        assert e.dwconv_f32_route(x, r, r, s, s, *p, pass_)[0] == "tiled", pass_
    return (e.dwconv_f32_fwd(x, wt, s, s, *p),
            e.dwconv_f32_dgrad(gy, wt, x.shape[2], x.shape[3], s, s, *p),
            e.dwconv_f32_wgrad(gy, x, r, r, s, s, *p))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tiled_vs_fp64(case):
    x, wt, gy, s, p = _inputs(case)
    got = _run(_ext(), x.cuda(), wt.cuda(), gy.cuda(), s, p)
    assert got[2].shape == wt.shape
    _check3(got, x, wt, gy, s, p)


def test_wgrad_many_items():
    """More (image, tile) work items than slots: a block accumulates over a
    run of tiles across image seams, ordered_reduce sums many slots."""
    e = _ext()
    x, wt, gy, s, p = _inputs((6, 4, 130, 130, 3, 1, 1))
    route, th, tw, _, _, slots, _ = e.dwconv_f32_route(x, 3, 3, s, s, *p,
                                                        "wgrad")
    assert route == "tiled"
    assert 1 < slots < 6 * -(-130 // th) * -(-130 // tw)
    ref = _ref64(x, wt, gy, s, p)[2]
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p)[2]
    gw = e.dwconv_f32_wgrad(gy.cuda(), x.cuda(), 3, 3, s, s, *p)
    _check("wgrad", gw, ref, mag, 6 * 130 * 130)


def test_functional_autograd():
    from distribuuuu_amd import ops
    from distribuuuu_amd.ops import functional as DF

    x, wt, gy, s, p = _inputs((3, 20, 37, 19, 5, 2, 2))
    was = ops.get_fp32_precision()
    out = {}
    try:
        for mode in ("highest", "high"):
            ops.set_fp32_precision(mode)
            xg, wg = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                y = DF.conv2d(xg, wg, None, (s, s), p, (1, 1), x.shape[1])
                y.backward(gy.cuda())
            assert not [w for w in caught if "fall" in str(w.message)]
            torch.cuda.synchronize()
            out[mode] = (y.detach(), xg.grad, wg.grad)
    finally:
        ops.set_fp32_precision(was)
    assert out["highest"][2].shape == wt.shape
    _check3(out["highest"], x, wt, gy, s, p)
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
    x, wt, gy, s, p = (t.cuda() if torch.is_tensor(t) else t
                       for t in _inputs((2, 12, 38, 20, 5, 2, 2)))
    a = _run(e, x, wt, gy, s, p)
    b = _run(e, x, wt, gy, s, p)
    c = _run(e, _nan_backed(x), wt, _nan_backed(gy), s, p)
    for name, u, v, z in zip(PASSES, a, b, c):
        assert torch.equal(u, v), f"{name} bits differ between two calls"
        assert torch.equal(u, z), f"{name} read past the image"
