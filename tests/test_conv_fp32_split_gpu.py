"""3xBF16 split fp32 conv kernels (csrc/conv_fp32_split.hip) vs float64.

Under ops.set_fp32_precision("high") every case is on the split route
(asserted) and is compared elementwise with F.conv2d and its autograd in
float64 on the CPU, evaluated on the exact fp32 inputs. The bound is derived
(docs/ARCHITECTURE.md "fp32 split-bf16 conv"), not measured:

    err <= 2^-15 * A + 2 * n * 2^-24 * A

2^-15 is the three kept bf16 products' worst relative error against the fp32
product, n the number of terms of the output's sum (fwd R*S*Cg, dgrad R*S*Kg,
wgrad N*Ho*Wo) and A the same sum over absolute values. One bf16 rounding is
128x looser; a kernel that loses a cross term misses by about 7x at n = 72.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
PASSES = ("fwd", "dgrad", "wgrad")

# (N, C, K, H, W, R, stride, pad, dil, groups): the smallest shapes that reach
# each thing that can go wrong; fwd / dgrad reductions stay under 600 terms
CASES = [
    (2, 8, 8, 5, 7, 3, 1, 1, 1, 1),       # partial tile everywhere, span 24 < 32
    (1, 40, 136, 9, 9, 1, 1, 0, 1, 1),    # Kg tail over two N tiles, span 40
    (3, 64, 64, 12, 12, 3, 1, 1, 1, 1),   # 432 rows: 4 m-tiles; dgrad Same
    (2, 16, 24, 11, 13, 3, 2, 1, 1, 1),   # dgrad Parity3x3 (offset scatter)
    (2, 32, 64, 10, 10, 1, 2, 0, 1, 1),   # dgrad Strided1x1 (zeroed gx)
    (1, 16, 16, 9, 9, 3, 1, 2, 2, 1),     # dilation 2
    (2, 48, 48, 8, 8, 3, 1, 1, 1, 3),     # groups, Cg = Kg = 16
    # wgrad M = 1125: two 1024-pixel split-m chunks, last k-step 5 pixels
    (5, 8, 16, 17, 17, 3, 1, 0, 1, 1),
]
DGRAD_KIND = {3: "Parity3x3", 4: "Strided1x1", 2: "Same"}
WGRAD_CASE = CASES[-1]
_REFS = {}


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ref64(x, w, gy, s, p, d, g):
    x, w = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv2d(x, w, None, s, p, d, g)
    gx, gw = torch.autograd.grad(y, (x, w), gy.double())
    return y.detach(), gx, gw


def _case(case):
    """(x, w, gy), float64 references, magnitudes A and term counts n;
    computed once per case and shared."""
    if case not in _REFS:
        n, c, k, h, wd, r, s, p, d, g = case
        torch.manual_seed(sum(case))
        ho = (h + 2 * p - d * (r - 1) - 1) // s + 1
        wo = (wd + 2 * p - d * (r - 1) - 1) // s + 1
        x, gy = torch.randn(n, c, h, wd), torch.randn(n, k, ho, wo)
        w = torch.randn(k, c // g, r, r)
        for t in (x, gy, w):  # mixed magnitudes meet in one sum
            t[:, ::7] *= 50
        x, w, gy = _cl(x), _cl(w), _cl(gy)
        _REFS[case] = ((x, w, gy), _ref64(x, w, gy, s, p, d, g),
                       _ref64(x.abs(), w.abs(), gy.abs(), s, p, d, g),
                       (r * r * c // g, r * r * k // g, n * ho * wo))
    return _REFS[case]


def _check(name, got, ref, A, n):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -15 * A + 2 * n * 2.0 ** -24 * A
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}")
    assert (err <= bound).all(), name


@pytest.fixture
def high():
    from distribuuuu_amd import ops

    ops.set_fp32_precision("high")
    try:
        yield _ext()
    finally:
        ops.set_fp32_precision("highest")
        ops.set_deterministic(False)


def _geom(case):
    _, _, _, _, _, _, s, p, d, g = case
    return (s, s, p, p, d, d, g)


def _assert_split(e, case):
    _, c, k, *_, g = case
    for ps in PASSES:
        assert e.fp32_conv_route(c // g, k // g, ps) == "split", ps


@pytest.mark.parametrize("case", CASES, ids=str)
def test_kernels_vs_fp64(high, case):
    e = high
    _assert_split(e, case)
    (x, w, gy), ref, mag, terms = _case(case)
    xg, wg, gyg = x.cuda(), w.cuda(), gy.cuda()
    geom = _geom(case)
    i = CASES.index(case)
    if i in DGRAD_KIND:
        assert e.conv2d_dgrad_route(gyg, wg, x.shape[2], x.shape[3],
                                    *geom)[0] == DGRAD_KIND[i]
    got = (e.conv2d_fwd(xg, wg, *geom),
           e.conv2d_dgrad(gyg, wg, x.shape[2], x.shape[3], *geom),
           e.conv2d_wgrad(gyg, xg, w.shape[2], w.shape[3], *geom))
    assert got[2].shape == w.shape
    assert got[2].is_contiguous(memory_format=torch.channels_last)
    for name, gt, rf, A, n in zip(PASSES, got, ref, mag, terms):
        _check(name, gt, rf, A, n)


def test_fwd_bn_partials(high):
    """y under the same bound; the partial rows, summed, against float64 sums
    of the kernel's own y: each is a sum of M fp32 terms in some order."""
    e, case = high, CASES[2]
    (x, w, _), ref, mag, terms = _case(case)
    y, part = e.conv2d_fwd_bn(x.cuda(), w.cuda(), *_geom(case))
    _check("fwd_bn", y, ref[0], mag[0], terms[0])
    k = y.shape[1]
    m = y.numel() // k
    assert part.shape == (2 * ((m + 127) // 128), 2 * k)
    yd, got = y.double(), part.double().sum(0)
    for name, gt, v in (("sum", got[:k], yd), ("sumsq", got[k:], yd * yd)):
        r, A = v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))
        assert ((gt - r).abs() <= 2 * m * 2.0 ** -24 * A).all(), name


def test_wgrad_deterministic(high):
    from distribuuuu_amd import ops

    e, case = high, WGRAD_CASE
    (x, w, gy), ref, mag, terms = _case(case)
    ops.set_deterministic(True)
    _assert_split(e, case)
    a, b = (e.conv2d_wgrad(gy.cuda(), x.cuda(), w.shape[2], w.shape[3],
                           *_geom(case)) for _ in range(2))
    assert torch.equal(a, b)
    _check("wgrad-det", a, ref[2], mag[2], terms[2])


def test_functional_autograd(high):
    from distribuuuu_amd import ops
    from distribuuuu_amd.ops import functional as DF

    e, case = high, CASES[2]
    (x, w, gy), ref, mag, terms = _case(case)
    s, _, p, _, d, _, g = _geom(case)
    _assert_split(e, case)
    xg, wg = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    y = DF.conv2d(xg, wg, None, (s, s), (p, p), (d, d), g)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    for name, gt, rf, A, n in zip(PASSES, (y.detach(), xg.grad, wg.grad), ref,
                                  mag, terms):
        _check(name, gt, rf, A, n)
    ops.set_fp32_precision("highest")
    for ps in PASSES:
        assert e.fp32_conv_route(case[1], case[2], ps) == "exact", ps
