"""Fused BN kernels against the compositions they replace, bit for bit.

Part A: bn_act_maxpool_fwd / bn_pool_bwd(_stats/_apply) versus
bn_apply_act -> maxpool_fwd and maxpool_bwd -> bn_bwd. Every step of either
chain is elementwise, a max under one tie rule, or a sum in one fixed order,
so the comparison is torch.equal, not a tolerance. One anchor case is also
held against an fp64 autograd reference that shares no kernel with either.

Part B: the residual-join BN apply that normalises the raw shortcut-conv
output itself versus bn_apply_act -> bn_apply_act_mask, and the module-level
wiring (Bottleneck, resnet18) with the fused paths on and forced off.
"""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


# ---------------------------------------------------------------------------
# Part A
# ---------------------------------------------------------------------------
A_SHAPES = [
    (1, 8, 7, 7),     # odd size, single pack, every window clipped somewhere
    (2, 64, 8, 8),    # the stem's channel count, even size
    (3, 24, 6, 10),   # cpacks = 3: ncp not a power of two, idle row lanes
    (2, 64, 9, 11),   # rows = 198: unrolled loop and tail, 7 blocks
    (2, 16, 1, 5),    # degenerate rows
    (2, 16, 5, 1),    # degenerate columns
]
A_CASES = [(dt, s) for s in A_SHAPES for dt in (BF16, FP32)] + [
    (BF16, (1, 2056, 4, 4)),  # C/pack = 257: multi-column loop with barrier
]
A_IDS = [f"{_name(dt)}-{'x'.join(map(str, s))}" for dt, s in A_CASES]


@functools.lru_cache(maxsize=None)
def _a_inputs(dtype, shape):
    """x ~ N(0,1), gamma of both signs, beta near 0 (about half of the
    pre-activations negative), the bn_stats coefficients, and a pooled
    gradient ~ N(0,1) rounded to the dtype. Shared and never modified."""
    e = _ext()
    n, c, h, w = shape
    gen = torch.Generator(device="cuda").manual_seed(4321 + c + 7 * h + w)
    x = _cl(torch.randn(shape, device="cuda", generator=gen).to(dtype))
    sign = torch.where(torch.arange(c, device="cuda") % 2 == 0, 1.0, -1.0)
    gamma = sign * (torch.rand(c, device="cuda", generator=gen) + 0.5)
    beta = 0.1 * torch.randn(c, device="cuda", generator=gen)
    mean, rstd, scale, shift = e.bn_stats(x, gamma, beta, None, None, 0.1,
                                          1e-5, True, None)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gp = _cl(torch.randn((n, c, ho, wo), device="cuda",
                         generator=gen).to(dtype))
    return dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd,
                scale=scale, shift=shift, gp=gp)


@functools.lru_cache(maxsize=None)
def _a_chain(dtype, shape, act):
    """Today's composition on the shared inputs."""
    e = _ext()
    k = _a_inputs(dtype, shape)
    h, w = shape[2], shape[3]
    y = e.bn_apply_act(k["x"], k["scale"], k["shift"], act, None)
    yp, idx = e.maxpool_fwd(y, 3, 2, 1)
    g = e.maxpool_bwd(k["gp"], idx, h, w, 3, 2, 1)
    gx, gw, gb, _ = e.bn_bwd(g, k["x"], None, k["mean"], k["rstd"],
                             k["gamma"], k["scale"], k["shift"], act, True,
                             False)
    sums = e.bn_bwd_stats(g, k["x"], None, k["scale"], k["shift"], act)
    return dict(y=y, yp=yp, idx=idx, g=g, gx=gx, gw=gw, gb=gb, sums=sums)


def _tie_fraction(y):
    """Share of (window, channel) pairs whose in-bounds taps hold two equal
    values."""
    p = F.pad(y.float().contiguous(), (1, 1, 1, 1), value=float("-inf"))
    n, c = p.shape[:2]
    u = F.unfold(p, 3, stride=2).reshape(n, c, 9, -1)
    v, _ = u.sort(dim=2)
    tie = ((v[:, :, 1:] == v[:, :, :-1]) & torch.isfinite(v[:, :, 1:])).any(2)
    top_tie = (v[:, :, 8] == v[:, :, 7])
    return tie.float().mean().item(), top_tie.float().mean().item()


@pytest.mark.parametrize("act", [1, 0], ids=["relu", "none"])
@pytest.mark.parametrize("dtype,shape", A_CASES, ids=A_IDS)
def test_bn_act_maxpool_fwd_equals_chain(dtype, shape, act):
    e = _ext()
    k = _a_inputs(dtype, shape)
    ref = _a_chain(dtype, shape, act)
    if act == 1:
        # the tie rule is only under test if ties are there
        frac, top = _tie_fraction(ref["y"])
        print(f"windows with a tie {frac:.3f}, with a tie at the max {top:.3f}")
        assert frac >= 0.10
    yp, idx = e.bn_act_maxpool_fwd(k["x"], k["scale"], k["shift"], act)
    assert yp.shape == ref["yp"].shape and idx.dtype == torch.uint8
    assert yp.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(yp, ref["yp"])
    assert torch.equal(idx, ref["idx"])


@pytest.mark.parametrize("act", [1, 0], ids=["relu", "none"])
@pytest.mark.parametrize("dtype,shape", A_CASES, ids=A_IDS)
def test_bn_pool_bwd_equals_chain(dtype, shape, act):
    e = _ext()
    k = _a_inputs(dtype, shape)
    ref = _a_chain(dtype, shape, act)
    gx, gw, gb = e.bn_pool_bwd(k["gp"], ref["idx"], k["x"], k["mean"],
                               k["rstd"], k["gamma"], k["scale"], k["shift"],
                               act, True)
    assert torch.equal(gx, ref["gx"])
    assert torch.equal(gw, ref["gw"])
    assert torch.equal(gb, ref["gb"])
    # the stats/apply split (the SyncBN entry points)
    sums = e.bn_pool_bwd_stats(k["gp"], ref["idx"], k["x"], k["scale"],
                               k["shift"], act)
    assert torch.equal(sums, ref["sums"])
    rows = float(k["x"].numel() // shape[1])
    want = e.bn_bwd_apply(ref["g"], k["x"], None, k["mean"], k["rstd"],
                          k["gamma"], k["scale"], k["shift"], sums, rows, act,
                          True, False)
    got = e.bn_pool_bwd_apply(k["gp"], ref["idx"], k["x"], k["mean"],
                              k["rstd"], k["gamma"], k["scale"], k["shift"],
                              sums, rows, act, True)
    for a, b in zip(got, want[:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [BF16, FP32], ids=_name)
def test_stem_fused_equals_chain_when_the_max_itself_ties(dtype):
    """The strict-'>' argmax rule only shows where the MAXIMUM is tied. With
    shift = -|scale| a pre-activation is negative with probability 0.84, so
    about a fifth of the interior windows (0.84^9) and more of the clipped
    ones are all zero under relu: the argmax must then be the first
    in-bounds tap, and the backward must route every gradient there."""
    e = _ext()
    shape = (2, 64, 9, 11)
    k = _a_inputs(dtype, shape)
    scale = k["scale"]
    shift = -scale.abs()
    y = e.bn_apply_act(k["x"], scale, shift, 1, None)
    frac, top = _tie_fraction(y)
    print(f"windows with a tie {frac:.3f}, with a tie at the max {top:.3f}")
    assert top >= 0.10
    yp_ref, idx_ref = e.maxpool_fwd(y, 3, 2, 1)
    yp, idx = e.bn_act_maxpool_fwd(k["x"], scale, shift, 1)
    assert torch.equal(yp, yp_ref)
    assert torch.equal(idx, idx_ref)
    g = e.maxpool_bwd(k["gp"], idx_ref, shape[2], shape[3], 3, 2, 1)
    want = e.bn_bwd(g, k["x"], None, k["mean"], k["rstd"], k["gamma"], scale,
                    shift, 1, True, False)
    got = e.bn_pool_bwd(k["gp"], idx, k["x"], k["mean"], k["rstd"],
                        k["gamma"], scale, shift, 1, True)
    for a, b in zip(got, want[:3]):
        assert torch.equal(a, b)


def test_bn_act_maxpool_vs_fp64_autograd():
    """Anchor outside the project's kernels: max_pool2d(relu(x*scale+shift))
    in fp64 autograd on the CPU, shape (2, 64, 9, 11) bf16.

    The reference's argmax has to be unambiguous, so the input is built
    without ties: the centre tap of a window belongs to no other window, and
    wherever a window's best pre-activation is not positive or leads the
    runner-up by less than 1/16 of its value (bf16 rounds at 2^-9) the
    centre tap is raised above the rest. About two windows in three keep a
    natural winner. Nothing is masked out. Tolerances are those of
    test_pool_loss_gpu.py (pooled values) and test_bn_stats_gpu.py (gx, gw,
    gb) for the unfused kernels."""
    e = _ext()
    n, c, h, w = 2, 64, 9, 11
    ho, wo = 5, 6
    gen = torch.Generator().manual_seed(99)
    sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0)
    scale = (sign * (torch.rand(c, generator=gen) + 0.5)).double()
    shift = (0.1 * torch.randn(c, generator=gen)).double()
    x = torch.randn(n, c, h, w, generator=gen).bfloat16().double()
    sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)

    def windows(z):
        p = F.pad(z, (1, 1, 1, 1), value=float("-inf"))
        return F.unfold(p, 3, stride=2).reshape(n, c, 9, ho, wo)

    u = windows(x * sc + sh)
    others = torch.cat([u[:, :, :4], u[:, :, 5:]], 2).amax(2).clamp_min(0.0)
    top2 = u.topk(2, dim=2).values
    weak = (top2[:, :, 0] <= 0) | (top2[:, :, 0] - top2[:, :, 1]
                                   < top2[:, :, 0].abs() / 16)
    target = others * 1.25 + 0.5 + torch.rand(n, c, ho, wo, generator=gen)
    centre = x[:, :, ::2, ::2]
    x[:, :, ::2, ::2] = torch.where(weak, (target - sh) / sc, centre)
    x = x.bfloat16().double()
    # the construction holds after rounding x: clear, positive winners
    top2 = windows(x * sc + sh).topk(2, dim=2).values
    assert (top2[:, :, 0] > 0).all()
    assert (top2[:, :, 0] - top2[:, :, 1] >= top2[:, :, 0] / 32).all()
    print(f"windows steered to the centre tap: {weak.double().mean():.3f}")

    gp = torch.randn(n, c, ho, wo, generator=gen).bfloat16().double()
    xr = x.clone().requires_grad_(True)
    scr = scale.clone().requires_grad_(True)
    shr = shift.clone().requires_grad_(True)
    z = torch.relu(xr * scr.view(1, -1, 1, 1) + shr.view(1, -1, 1, 1))
    ref_y, ref_i = F.max_pool2d(z, 3, 2, 1, return_indices=True)
    ref_y.backward(gp)
    # flat h*W+w index -> window-local kh*3+kw
    hh, ww = ref_i // w, ref_i % w
    oh = torch.arange(ho).view(1, 1, -1, 1)
    ow = torch.arange(wo).view(1, 1, 1, -1)
    ref_local = (hh - (2 * oh - 1)) * 3 + (ww - (2 * ow - 1))

    dev = dict(device="cuda")
    xg = _cl(x.to(dtype=BF16, **dev))
    scg, shg = scale.to(dtype=FP32, **dev), shift.to(dtype=FP32, **dev)
    yp, idx = e.bn_act_maxpool_fwd(xg, scg, shg, 1)
    tol = dict(atol=3e-2, rtol=3e-2)
    assert torch.allclose(yp.double().cpu(), ref_y.detach(), **tol)
    assert torch.equal(idx.cpu().long(), ref_local)
    # eval-mode backward with mean 0, rstd 1, gamma = scale: gx = scale * g,
    # gw = sum(g * x), gb = sum(g) — the derivatives of the reference
    zero = torch.zeros(c, **dev)
    one = torch.ones(c, **dev)
    gx, gw, gb = e.bn_pool_bwd(_cl(gp.to(dtype=BF16, **dev)), idx, xg, zero,
                               one, scg, scg, shg, 1, False)
    assert torch.allclose(gx.double().cpu(), xr.grad, atol=5e-2, rtol=5e-2)
    for got, want in ((gw, scr.grad), (gb, shr.grad)):
        assert torch.allclose(got.double().cpu(), want, rtol=2e-2,
                              atol=2e-2 * want.abs().max().item())


# ---------------------------------------------------------------------------
# Part B
# ---------------------------------------------------------------------------
B_CASES = [(dt, s) for s in [(2, 8, 3, 3), (2, 64, 5, 7), (1, 2056, 2, 2)]
           for dt in (BF16, FP32)]
B_IDS = [f"{_name(dt)}-{'x'.join(map(str, s))}" for dt, s in B_CASES]


@pytest.mark.parametrize("dtype,shape", B_CASES, ids=B_IDS)
def test_dual_apply_equals_two_applies(dtype, shape):
    e = _ext()
    c = shape[1]
    gen = torch.Generator(device="cuda").manual_seed(77 + c)
    x = _cl(torch.randn(shape, device="cuda", generator=gen).to(dtype))
    xr = _cl(torch.randn(shape, device="cuda", generator=gen).to(dtype))
    sc, sh, rsc, rsh = (torch.randn(c, device="cuda", generator=gen)
                        for _ in range(4))
    ident = e.bn_apply_act(xr, rsc, rsh, 0, None)
    y_ref, m_ref = e.bn_apply_act_mask(x, sc, sh, 1, ident)
    y, m = e.bn_apply_act_mask(x, sc, sh, 1, xr, rsc, rsh)
    assert torch.equal(y, y_ref)
    assert torch.equal(m, m_ref)
    assert 0.2 < (y > 0).float().mean().item() < 0.8  # both relu branches


def _run_model(model, x, gy, fuse, monkeypatch, steps=2):
    """``steps`` forward/backward passes (the second takes BN statistics from
    the conv epilogues) with the fused paths on or forced off."""
    monkeypatch.setenv("DISTRIBUUUU_BN_FUSE", "1" if fuse else "0")
    m = copy.deepcopy(model)
    xin = x.clone().requires_grad_(True)
    for _ in range(steps):
        m.zero_grad(set_to_none=True)
        xin.grad = None
        out = m(xin)
        out.backward(gy)
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters()}
    return out.detach(), xin.grad, grads, m.state_dict()


def _assert_same_run(a, b):
    out_a, gx_a, grads_a, sd_a = a
    out_b, gx_b, grads_b, sd_b = b
    assert torch.equal(out_a, out_b)
    assert torch.equal(gx_a, gx_b)
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        ga, gb = grads_a[k], grads_b[k]
        if ga.dim() == 4:
            # conv weight gradients are sums of fp32 atomics: the tolerance
            # of test_conv_gpu.py::test_conv2d_wgrad
            err = (ga.float() - gb.float()).abs().max().item()
            assert err < 3e-2 * max(gb.float().abs().max().item(), 1.0), k
        else:
            assert torch.equal(ga, gb), k
    for k in sd_a:
        if "running_" in k or "num_batches_tracked" in k:
            assert torch.equal(sd_a[k], sd_b[k]), k


def _count_calls(monkeypatch, name):
    from distribuuuu_amd.ops import functional as DF

    calls = []
    real = getattr(DF, name)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(DF, name, spy)
    return calls


def _count_stem_ops(monkeypatch):
    """Counts applications of the fused stem autograd Function."""
    from distribuuuu_amd.ops import functional as DF

    calls = []
    real = DF._HIPBatchNormActMaxPool

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(1)
            return real.apply(*a)

    monkeypatch.setattr(DF, "_HIPBatchNormActMaxPool", Spy)
    return calls


def test_bottleneck_fused_shortcut_on_off(monkeypatch):
    from distribuuuu_amd.models.resnet import Bottleneck, conv1x1
    from distribuuuu_amd.ops import BatchNorm2d

    torch.manual_seed(11)
    ds = nn.Sequential(conv1x1(64, 64, 2), BatchNorm2d(64))
    blk = Bottleneck(64, 16, stride=2, downsample=ds)
    for m in blk.modules():
        if isinstance(m, BatchNorm2d):
            nn.init.normal_(m.weight, 1.0, 0.3)
            nn.init.normal_(m.bias, 0.0, 0.2)
    blk = blk.cuda().to(BF16).to(memory_format=torch.channels_last).train()
    x = _cl(torch.randn(2, 64, 8, 8, device="cuda").to(BF16))
    gy = _cl(torch.randn(2, 64, 4, 4, device="cuda").to(BF16))
    dual = _count_calls(monkeypatch, "batch_norm_act_dual")
    on = _run_model(blk, x, gy, True, monkeypatch)
    assert len(dual) == 2  # the fused path really ran, once per step
    off = _run_model(blk, x, gy, False, monkeypatch)
    assert len(dual) == 2
    _assert_same_run(on, off)
    sd = on[3]
    assert sd["downsample.1.num_batches_tracked"].item() == 2
    assert sd["bn3.num_batches_tracked"].item() == 2
    assert not torch.equal(sd["downsample.1.running_mean"],
                           torch.zeros_like(sd["downsample.1.running_mean"]))


def test_resnet18_fused_stem_and_shortcuts_on_off(monkeypatch):
    from distribuuuu_amd.models.resnet import resnet18

    torch.manual_seed(12)
    net = resnet18(num_classes=8)
    net = net.cuda().to(BF16).to(memory_format=torch.channels_last).train()
    x = _cl(torch.randn(2, 3, 32, 32, device="cuda").to(BF16))
    gy = torch.randn(2, 8, device="cuda").to(BF16)
    dual = _count_calls(monkeypatch, "batch_norm_act_dual")
    stem = _count_stem_ops(monkeypatch)
    on = _run_model(net, x, gy, True, monkeypatch)
    assert len(dual) == 2 * 3  # layer2-4 downsample blocks, two steps
    assert len(stem) == 2      # the fused stem ran, once per step
    off = _run_model(net, x, gy, False, monkeypatch)
    assert len(dual) == 2 * 3 and len(stem) == 2
    _assert_same_run(on, off)
    assert on[3]["bn1.num_batches_tracked"].item() == 2
