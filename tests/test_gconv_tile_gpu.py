"""LDS-tiled narrow-group conv kernels (csrc/gconv_tile.hip) vs float64.

Every case is on the tiled route (asserted) and is compared elementwise with
F.conv2d(groups=...) and its autograd in float64, evaluated on the exact bf16
inputs. The bound is derived, not measured:

    err <= 2^-8 * |ref| + 2 * n * 2^-24 * A

2^-8 is the worst relative half-ulp of the one bf16 rounding, n the number of
terms of the output's sum (fwd and dgrad: 9 * w, wgrad: N*Ho*Wo) and A the
same sum over absolute values (bf16 products are exact in fp32: only the adds
round; the factor 2 covers the MFMA's internal add order).
"""

import pytest
import torch
import torch.nn.functional as F

from test_gconv_route import GPU_CASES, RUN_CASES, route, tiles_per_image

pytestmark = pytest.mark.gpu
PASSES = ("fwd", "dgrad", "wgrad")


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
    x = _cl(torch.randn(n, g * w, h, wd).bfloat16())
    wt = _cl(torch.randn(g * w, w, 3, 3).bfloat16())
    gy = _cl(torch.randn(n, g * w, ho, wo).bfloat16())
    return x, wt, gy, s, p, g


def _ref64(x, wt, gy, s, p, g):
    """(y, gx, gw) in float64 on the CPU."""
    x, wt = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv2d(x, wt, None, s, p, 1, g)
    gx, gw = torch.autograd.grad(y, (x, wt), gy.double())
    return y.detach(), gx, gw


def _refs(x, wt, gy, s, p, g):
    return (_ref64(x, wt, gy, s, p, g),
            _ref64(x.abs(), wt.abs(), gy.abs(), s, p, g),
            (9 * wt.shape[1], 9 * wt.shape[1], gy.numel() // gy.shape[1]))


def _check(name, got, ref, mag, n):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2 * n * 2.0 ** -24 * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, err - bound {worst:.3e}")
    assert worst <= 0, name


def _run(e, x, wt, gy, s, p, g):
    y = e.gconv_fwd(x, wt, s, s, *p, g)
    gx = e.gconv_dgrad(gy, wt, x.shape[2], x.shape[3], s, s, *p, g)
    gw = e.gconv_wgrad(gy, x, s, s, *p, g)
    return y, gx, gw


@pytest.mark.parametrize("case", GPU_CASES + RUN_CASES, ids=str)
def test_tiled_vs_fp64(case):
    e = _ext()
    for pass_ in PASSES:
        rt = route(e, case, pass_)
        assert rt[0] == "tile", pass_
        if case in RUN_CASES:
            # a run length that does not divide the tiles of an image: runs
            # wrap tile rows and cross image seams
            assert rt[4] > 1 and tiles_per_image(case, pass_, rt[1]) % rt[4]
    x, wt, gy, s, p, g = _inputs(case)
    ref, mag, terms = _refs(x, wt, gy, s, p, g)
    got = _run(e, x.cuda(), wt.cuda(), gy.cuda(), s, p, g)
    # conv2d_wgrad's layout: at::empty(channels_last)
    assert got[2].shape == wt.shape and got[2].stride() == wt.stride()
    for name, gt, rf, m, n in zip(PASSES, got, ref, mag, terms):
        _check(name, gt, rf, m, n)


@pytest.mark.parametrize("case", [GPU_CASES[2], GPU_CASES[-4], RUN_CASES[0]],
                         ids=str)
def test_bn_partials(case):
    """The partial rows, summed, against float64 sums of the kernel's own y:
    each is a sum of M = N*Ho*Wo fp32 terms in some order."""
    e = _ext()
    x, wt, _, s, p, g = _inputs(case)
    y, part = e.gconv_fwd_bn(x.cuda(), wt.cuda(), s, s, *p, g)
    assert torch.equal(y, e.gconv_fwd(x.cuda(), wt.cuda(), s, s, *p, g))
    c = y.shape[1]
    assert part.shape == (route(e, case, "fwd")[5], 2 * c)
    yd = y.double()
    m = yd.numel() // c
    got = part.double().sum(0)
    for name, gt, v in (("sum", got[:c], yd), ("sumsq", got[c:], yd * yd)):
        ref, mag = v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))
        worst = ((gt - ref).abs() - 2 * m * 2.0 ** -24 * mag).max().item()
        print(f"{name}: err - bound {worst:.3e}")
        assert worst <= 0, name


def test_functional_autograd(monkeypatch):
    """DF.conv2d end to end, stride 2, the raw 4-D weight at w = 4: no
    block-diagonal packing on the way."""
    from distribuuuu_amd.ops import functional as DF

    monkeypatch.setattr(DF, "_pack_narrow_groups", None)
    case = GPU_CASES[3]
    assert case[2] == 4 and case[5] == 2
    x, wt, gy, s, p, g = _inputs(case)
    ref, mag, terms = _refs(x, wt, gy, s, p, g)
    xg, wg = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
    y = DF.conv2d(xg, wg, None, (s, s), p, (1, 1), g)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    assert wg.grad.shape == wt.shape
    for name, gt, rf, m, n in zip(PASSES, (y.detach(), xg.grad, wg.grad), ref,
                                  mag, terms):
        _check(name, gt, rf, m, n)


def _nan_backed(t):
    """The same NHWC tensor at the front of a larger NaN-filled storage."""
    n, c, h, w = t.shape
    buf = torch.full((t.numel() + 3 * c * (w + 2) * 8,), float("nan"),
                     dtype=t.dtype, device=t.device)
    v = buf[:t.numel()].view(n, h, w, c).permute(0, 3, 1, 2)
    v.copy_(t)
    assert v.is_contiguous(memory_format=torch.channels_last)
    return v


@pytest.mark.parametrize("case", [GPU_CASES[4], GPU_CASES[-5]], ids=str)
def test_bits_repeat_and_halo_is_zero_fill(case):
    e = _ext()
    x, wt, gy, s, p, g = (t.cuda() if torch.is_tensor(t) else t
                          for t in _inputs(case))
    a = _run(e, x, wt, gy, s, p, g)
    b = _run(e, x, wt, gy, s, p, g)
    c = _run(e, _nan_backed(x), wt, _nan_backed(gy), s, p, g)
    for name, u, v, z in zip(PASSES, a, b, c):
        assert torch.equal(u, v), f"{name} bits differ between two calls"
        assert torch.equal(u, z), f"{name} read past the image"
