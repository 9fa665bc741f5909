"""BN statistics, apply and backward kernels against fp64 references computed
from the values the kernels read, at the shapes where the reduction takes
another path:

  rows=1; rows below the 256 row-lanes; cpacks=10 (256/cpacks not a power of
  two: the host sizes blocks for 25 row-lanes, the kernel runs 16); cpacks=29
  (RegNetY width); cpacks=257 > blockDim (multi-column loop; 3 rows per block
  -> 451 partial rows, which reach bn_finalize's 64-way unrolled loop and its
  tail).

Inputs have a per-channel mean from {0, 4, -16} and std from {1, 0.05}: the
kernel forms the variance as E[x^2] - E[x]^2 in fp32, which zero-mean inputs
cannot stress.

Bounds (U = 2^-24, per channel with fp64 mean m, variance v, s = sqrt(v)):
  mean      16 U (|m| + s)
  variance  64 U (m^2 + v)   absolute; this is the conditioning of the
            one-pass formula with an effective accumulation depth of 64 (the
            deepest sequential chain at these shapes is 3 rows per block, then
            about 29 partials per finalize lane).
Everything else (rstd, scale, shift, running stats, raw sums) is bounded by
propagating those two through its formula, plus 4 U per fp32 operation.
The channels with m = -16, s = 0.05 (|m|/s = 320) document the limit of the
one-pass formula: only finiteness and var >= 0 are asserted there, and the
error is printed.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# measured worst |err| / bound over all cases below on MI355X: 0.26 (fp32,
# C=1028; bf16 worst 0.084)
MEAN_ULPS = 16
# measured worst |err| / bound: 0.13 (fp32, C=40; bf16 worst 0.082). The
# limit channels (|m|/s = 320) also stay at 0.12 of this absolute bound, which
# there is a relative variance error of up to 4.8%.
VAR_ULPS = 64
EPS = 1e-5
MOM = 0.1

MEANS = (0.0, 4.0, -16.0)
STDS = (1.0, 0.05)

SHAPES = {
    torch.bfloat16: [(1, 8, 1, 1), (2, 8, 3, 3), (8, 80, 13, 13),
                     (8, 232, 13, 13), (8, 2056, 13, 13)],
    torch.float32: [(1, 4, 1, 1), (2, 4, 3, 3), (8, 40, 13, 13),
                    (8, 116, 13, 13), (8, 1028, 13, 13)],
}
CASES = [(dt, s) for dt, shapes in SHAPES.items() for s in shapes]
IDS = [f"{'bf16' if dt == torch.bfloat16 else 'fp32'}-{'x'.join(map(str, s))}"
       for dt, s in CASES]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """Input, affine parameters and the fp64 statistics of the ROUNDED input.
    Computed once per case and shared; nothing here is modified by a test."""
    n, c, h, w = shape
    gen = torch.Generator(device="cuda").manual_seed(1234 + c)
    ch = torch.arange(c, device="cuda")
    m = torch.tensor(MEANS, device="cuda")[ch % 3]
    s = torch.tensor(STDS, device="cuda")[(ch // 3) % 2]
    x = torch.randn(shape, device="cuda", generator=gen) \
        * s.view(1, -1, 1, 1) + m.view(1, -1, 1, 1)
    x = _cl(x.to(dtype))
    gamma = torch.rand(c, device="cuda", generator=gen) + 0.5
    beta = torch.randn(c, device="cuda", generator=gen)
    xd = x.double()
    rows = n * h * w
    mean = xd.mean(dim=(0, 2, 3))
    var = xd.var(dim=(0, 2, 3), unbiased=False)
    # channels that only document the limit of the one-pass formula
    limit = (m == -16.0) & (s == 0.05)
    return dict(x=x, gamma=gamma, beta=beta, rows=rows, mean=mean, var=var,
                sum=xd.sum(dim=(0, 2, 3)), sumsq=(xd * xd).sum(dim=(0, 2, 3)),
                limit=limit)


def _bounds(k):
    mean, var = k["mean"], k["var"]
    tol_mean = MEAN_ULPS * U * (mean.abs() + var.sqrt())
    tol_var = VAR_ULPS * U * (mean * mean + var)
    return tol_mean, tol_var


def _assert_within(name, got, want, tol, keep):
    err = (got.double() - want).abs()
    ratio = (err / tol.clamp_min(1e-300))[keep]
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{name}: worst err/bound = {worst:.3g}")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_bn_stats_training_vs_fp64(dtype, shape):
    e = _ext()
    k = _case(dtype, shape)
    x, gamma, beta, rows = k["x"], k["gamma"], k["beta"], k["rows"]
    c = shape[1]
    rm = torch.zeros(c, device="cuda")
    rv = torch.ones(c, device="cuda")
    mean, rstd, scale, shift = e.bn_stats(x, gamma, beta, rm, rv, MOM, EPS,
                                          True, None)
    # second call: running stats accumulate, batch stats repeat bit for bit
    again = e.bn_stats(x, gamma, beta, rm, rv, MOM, EPS, True, None)
    for a, b in zip((mean, rstd, scale, shift), again):
        assert torch.equal(a, b)

    keep = ~k["limit"]
    tol_mean, tol_var = _bounds(k)
    rmean, rvar = k["mean"], k["var"]
    gvar = 1.0 / rstd.double() ** 2 - EPS

    for t in (mean, rstd, scale, shift, rm, rv):
        assert torch.isfinite(t).all()
    assert (gvar >= -4 * U * EPS - 4 * U * gvar.abs()).all()
    lim = k["limit"]
    if lim.any():
        rel = ((gvar - rvar).abs() / rvar.clamp_min(1e-300))[lim].max().item()
        print(f"limit channels (m=-16, s=0.05): worst relative variance "
              f"error {rel:.3g}, worst / variance bound "
              f"{((gvar - rvar).abs() / tol_var)[lim].max().item():.3g}")

    _assert_within("mean", mean, rmean, tol_mean, keep)
    # 1/rstd^2 - eps adds the rsqrt's own rounding: 4 U (v + eps)
    _assert_within("var", gvar, rvar, tol_var + 4 * U * (rvar + EPS), keep)

    # propagate: rstd = (v+eps)^-1/2 -> relative error tol_var / (2 (v+eps))
    r_rstd = (rvar + EPS).rsqrt()
    rel_rstd = 0.5 * tol_var / (rvar + EPS) + 4 * U
    _assert_within("rstd", rstd, r_rstd, rel_rstd * r_rstd, keep)
    gd, bd = gamma.double(), beta.double()
    r_scale = gd * r_rstd
    tol_scale = (rel_rstd + 2 * U) * r_scale.abs()
    _assert_within("scale", scale, r_scale, tol_scale, keep)
    r_shift = bd - rmean * r_scale
    tol_shift = tol_mean * r_scale.abs() + rmean.abs() * tol_scale \
        + 4 * U * (bd.abs() + (rmean * r_scale).abs())
    _assert_within("shift", shift, r_shift, tol_shift, keep)

    # running stats after two updates from (0, 1); n/(n-1) correction (the
    # kernel applies none for a single row, where it is undefined)
    unb = rows / (rows - 1.0) if rows > 1 else 1.0
    a2 = 1.0 - (1.0 - MOM) ** 2
    r_rm = a2 * rmean
    r_rv = (1.0 - MOM) ** 2 + a2 * rvar * unb
    _assert_within("running_mean", rm, r_rm,
                   a2 * tol_mean + 4 * U * r_rm.abs(), keep)
    _assert_within("running_var", rv, r_rv,
                   a2 * unb * tol_var + 4 * U * r_rv.abs(), keep)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_bn_sums_vs_fp64(dtype, shape):
    """Raw per-channel sums (the SyncBN path): same bounds, times the count."""
    e = _ext()
    k = _case(dtype, shape)
    s, ss = e.bn_sums(k["x"])
    tol_mean, tol_var = _bounds(k)
    keep = torch.ones_like(k["limit"])  # sums are well conditioned everywhere
    _assert_within("sum", s, k["sum"], k["rows"] * tol_mean, keep)
    _assert_within("sumsq", ss, k["sumsq"], k["rows"] * tol_var, keep)


@pytest.mark.parametrize("dtype,shape", CASES, ids=IDS)
def test_bn_stats_eval_vs_fp64(dtype, shape):
    e = _ext()
    k = _case(dtype, shape)
    c = shape[1]
    gen = torch.Generator(device="cuda").manual_seed(7)
    rm = torch.randn(c, device="cuda", generator=gen) * 4
    rv = torch.rand(c, device="cuda", generator=gen) * 2 + 1e-3
    rm0, rv0 = rm.clone(), rv.clone()
    mean, rstd, scale, shift = e.bn_stats(k["x"], k["gamma"], k["beta"], rm,
                                          rv, MOM, EPS, False, None)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    assert torch.equal(mean, rm)
    keep = torch.ones_like(k["limit"])
    r_rstd = (rv.double() + EPS).rsqrt()
    _assert_within("rstd", rstd, r_rstd, 4 * U * r_rstd, keep)
    r_scale = k["gamma"].double() * r_rstd
    _assert_within("scale", scale, r_scale, 6 * U * r_scale.abs(), keep)
    r_shift = k["beta"].double() - rm.double() * r_scale
    _assert_within("shift", shift, r_shift,
                   6 * U * (rm.double() * r_scale).abs()
                   + 4 * U * (k["beta"].double().abs()
                              + (rm.double() * r_scale).abs()), keep)


# ---------------------------------------------------------------------------
# apply / backward at the same awkward channel counts
# ---------------------------------------------------------------------------
APPLY_SHAPES = [(8, 80, 13, 13), (8, 2056, 7, 7)]


def _tol(dtype):
    return dict(atol=3e-2, rtol=3e-2) if dtype == torch.bfloat16 else dict(
        atol=1e-4, rtol=1e-4)


def _act(z, act):
    return (z, F.relu(z), F.silu(z), torch.sigmoid(z))[act]


@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=["c80", "c2056"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", [0, 1])
def test_bn_apply_vs_fp64(dtype, act, shape):
    e = _ext()
    torch.manual_seed(0)
    c = shape[1]
    x = _cl(torch.randn(shape, device="cuda", dtype=dtype))
    r = _cl(torch.randn(shape, device="cuda", dtype=dtype))
    scale = torch.randn(c, device="cuda")
    shift = torch.randn(c, device="cuda")
    z = x.double() * scale.double().view(1, -1, 1, 1) \
        + shift.double().view(1, -1, 1, 1)
    y = e.bn_apply_act(x, scale, shift, act, None)
    assert torch.allclose(y.double(), _act(z, act), **_tol(dtype))
    y2 = e.bn_apply_act(x, scale, shift, act, r)
    assert torch.allclose(y2.double(), _act(z + r.double(), act),
                          **_tol(dtype))


@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=["c80", "c2056"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_bn_bwd_vs_fp64(act, res, shape):
    e = _ext()
    torch.manual_seed(0)
    c = shape[1]
    x = _cl(torch.randn(shape, device="cuda", dtype=torch.bfloat16))
    rt = _cl(torch.randn_like(x)) if res else None
    gamma = torch.randn(c, device="cuda") * 0.5 + 1
    beta = torch.randn(c, device="cuda") * 0.1
    mean, rstd, scale, shift = e.bn_stats(x, gamma, beta, None, None,
                                          0.1, 1e-5, True, None)
    gy = _cl(torch.randn_like(x))
    gx, gw, gb, gres = e.bn_bwd(gy, x, rt, mean, rstd, gamma, scale, shift,
                                act, True, res)
    xf = x.double().detach().requires_grad_(True)
    gamf = gamma.double().detach().requires_grad_(True)
    betf = beta.double().detach().requires_grad_(True)
    mu = xf.mean(dim=(0, 2, 3), keepdim=True)
    var = xf.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    z = (xf - mu) / (var + 1e-5).sqrt() * gamf.reshape(1, -1, 1, 1) \
        + betf.reshape(1, -1, 1, 1)
    if res:
        rf = rt.double().detach().requires_grad_(True)
        z = z + rf
    _act(z, act).backward(gy.double())
    if act == 1:
        # relu' jumps at 0: where |z| is within the fp32 rounding of the
        # kernel's own z the reference mask is not defined; such elements
        # (expected count here << 1) are left out of the elementwise checks
        sure = (z.detach().abs() > 1e-5).double()
        gx, xf.grad = gx.double() * sure, xf.grad * sure
        if res:
            gres, rf.grad = gres.double() * sure, rf.grad * sure
    assert torch.allclose(gx.double(), xf.grad, atol=5e-2, rtol=5e-2)
    for got, want in ((gw, gamf.grad), (gb, betf.grad)):
        assert torch.allclose(got.double(), want, rtol=2e-2,
                              atol=2e-2 * want.abs().max().item())
    if res:
        assert torch.allclose(gres.double(), rf.grad, atol=5e-2, rtol=5e-2)
