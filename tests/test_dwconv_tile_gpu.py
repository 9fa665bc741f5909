"""LDS-tiled depthwise kernels (csrc/depthwise_tile.hip) vs float64.

Every case is on the tiled route (asserted) and is compared elementwise with
F.conv2d(groups=C) and its autograd in float64, evaluated on the exact bf16
inputs. The bound is derived, not measured:

    err <= 2^-8 * |ref| + 2 * n * 2^-24 * A

2^-8 is the worst relative half-ulp of the one bf16 rounding, n the number of
terms of the output's sum (fwd and dgrad: R*S, wgrad: N*Ho*Wo) and A the same
sum over absolute values (bf16 products are exact in fp32: only the adds
round).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, C, H, W, R, stride, pad)
CASES = [
    # map smaller than the filter: every tap but one is halo
    (2, 8, 1, 1, 3, 1, 1), (1, 8, 2, 3, 5, 2, 2),
    # several ragged tiles on both axes, C = 5 packs, image seams in a run
    (3, 40, 37, 19, 3, 1, 1), (3, 40, 37, 19, 5, 1, 2),
    # stride 2, odd and even extent: all four dgrad parity classes
    (2, 24, 37, 19, 3, 2, 1), (2, 24, 38, 20, 5, 2, 2),
    # two chunks (9 + 8 packs), whole-image tiles, several images per block
    (2, 136, 14, 14, 5, 1, 2), (2, 136, 7, 7, 3, 2, 1),
    # pad 0 and unequal pads
    (2, 16, 20, 20, 3, 1, 0), (2, 16, 21, 21, 5, 2, 0),
    (2, 16, 20, 20, 5, 1, (2, 0)),
    # 128 work items, one per slot (test_wgrad_many_items has runs of tiles)
    (4, 32, 64, 64, 3, 1, 1),
]


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
    x = _cl(torch.randn(n, c, h, w).bfloat16())
    wt = _cl(torch.randn(c, 1, r, r).bfloat16())
    gy = _cl(torch.randn(n, c, ho, wo).bfloat16())
    return x, wt, gy, s, p


def _ref64(x, wt, gy, s, p):
    """(y, gx, gw) in float64 on the CPU."""
    x, wt = x.double().requires_grad_(), wt.double().requires_grad_()
    y = F.conv2d(x, wt, None, s, p, 1, x.shape[1])
    gx, gw = torch.autograd.grad(y, (x, wt), gy.double())
    return y.detach(), gx, gw


def _check(name, got, ref, mag, n):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2 * n * 2.0 ** -24 * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, err - bound {worst:.3e}")
    assert worst <= 0, name


def _run(e, x, wt, gy, s, p):
    r = wt.shape[2]
    for pass_ in ("fwd", "dgrad", "wgrad"):
        assert e.dwconv_route(x, r, r, s, s, *p, pass_)[0] == "tiled", pass_
    y = e.dwconv_fwd(x, wt, s, s, *p)
    gx = e.dwconv_dgrad(gy, wt, x.shape[2], x.shape[3], s, s, *p)
    gw = e.dwconv_wgrad(gy, x, r, r, s, s, *p)
    return y, gx, gw


@pytest.mark.parametrize("case", CASES, ids=str)
def test_tiled_vs_fp64(case):
    e = _ext()
    x, wt, gy, s, p = _inputs(case)
    ref = _ref64(x, wt, gy, s, p)
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p)
    got = _run(e, x.cuda(), wt.cuda(), gy.cuda(), s, p)
    r = wt.shape[2]
    # the generic bf16 result's layout: at::empty(channels_last)
    assert got[2].shape == wt.shape and got[2].stride() == (r * r, 1, r, 1)
    terms = (r * r, r * r, gy.shape[0] * gy.shape[2] * gy.shape[3])
    for name, g, rf, m, n in zip(("fwd", "dgrad", "wgrad"), got, ref, mag,
                                 terms):
        _check(name, g, rf, m, n)


def test_wgrad_many_items():
    """More (image, tile) work items than slots: a block accumulates over a
    run of tiles across image seams, ordered_reduce sums many slots."""
    e = _ext()
    case = (6, 8, 130, 130, 3, 1, 1)  # 6 * 17 * 9 = 918 items, 512 slots
    x, wt, gy, s, p = _inputs(case)
    slots = e.dwconv_route(x, 3, 3, s, s, *p, "wgrad")[5]
    assert 1 < slots < 918
    ref = _ref64(x, wt, gy, s, p)[2]
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p)[2]
    gw = e.dwconv_wgrad(gy.cuda(), x.cuda(), 3, 3, s, s, *p)
    _check("wgrad", gw, ref, mag, 6 * 130 * 130)


def test_functional_autograd():
    from distribuuuu_amd.ops import functional as DF

    case = (3, 40, 37, 19, 5, 2, 2)
    x, wt, gy, s, p = _inputs(case)
    ref = _ref64(x, wt, gy, s, p)
    mag = _ref64(x.abs(), wt.abs(), gy.abs(), s, p)
    xg, wg = x.cuda().requires_grad_(), wt.cuda().requires_grad_()
    y = DF.conv2d(xg, wg, None, (s, s), p, (1, 1), x.shape[1])
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    _check("fwd", y.detach(), ref[0], mag[0], 25)
    _check("x.grad", xg.grad, ref[1], mag[1], 25)
    _check("w.grad", wg.grad, ref[2], mag[2], gy.numel() // gy.shape[1])


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
                       for t in _inputs((2, 24, 38, 20, 5, 2, 2)))
    assert not e.is_deterministic()
    a = _run(e, x, wt, gy, s, p)
    b = _run(e, x, wt, gy, s, p)
    assert torch.equal(a[2], b[2]), "wgrad bits differ between two calls"
    c = _run(e, _nan_backed(x), wt, _nan_backed(gy), s, p)
    for name, u, v in zip(("fwd", "dgrad", "wgrad"), a, c):
        assert torch.equal(u, v), f"{name} read past the image"
