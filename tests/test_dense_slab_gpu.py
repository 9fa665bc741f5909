"""Dense-block slab kernels (csrc/dense_bn.hip) and route against fp64.

U = 2^-24 (one fp32 operation), u = 2^-8 for one bf16 rounding (0 in fp32).
Every stage is evaluated from the kernel's own tensors of the stage before
and held to 2x its bound:
  append sums  mean 16 U (|m| + s), variance 64 U (m^2 + v)  (test_bn_stats_gpu)
  finalize     the fp64 formulas on the kernel's sums, 4 U per fp32 operation
               propagated (variance through its one-pass conditioning)
  y            u |ref| + 4 U (|x scale| + |shift|)
  gb, gw       u |ref| + 2 n U A, A the sum of the terms' magnitudes
  coef         8 U times the terms' magnitudes, from the kernel's gw and gb
  gslab        u |ref| + 8 U (|before| + |P1 g'| + |P3 x| + |P2|)
Copies (append, take, channels outside a range) are bit-exact.
Measured worst err / (2 * bound) on MI355X is in docs/ARCHITECTURE.md.
"""

import copy

import pytest
import torch

from distribuuuu_amd.ops import dispatch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS, MOM = 1e-5, 0.1
# (N, H, W, C0, g, layers) in bf16; fp32 halves the widths (same pack counts)
SHAPES = [(2, 5, 5, 16, 8, 3), (3, 17, 13, 24, 16, 2), (2, 2, 2, 2064, 8, 2),
          (1, 1, 1, 8, 8, 1)]
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(autouse=True)
def deterministic_reductions():
    """Conv wgrad atomics are not this file's subject: runs must repeat."""
    was = dispatch.is_deterministic()
    dispatch.set_deterministic(True)
    yield
    dispatch.set_deterministic(was)


def slab_ref(x, sums, gamma, beta, rm0, rv0, k, training, u):
    """fp64 reference of one norm1 on the slab prefix x [rows, cin] ->
    {name: (value, bound)}; k holds the kernel's own tensors, each stage is
    evaluated from k's tensors of the stage before."""
    n = x.shape[0]
    if training:
        m = sums[0] / n
        q = sums[1] / n
        v = (q - m * m).clamp_min(0)
        e_m = 4 * U * m.abs()
        e_v = 4 * U * (q + m * m) + 2 * m.abs() * e_m
        unb = n / max(n - 1, 1)
        rm, rv = rm0 * (1 - MOM) + m * MOM, rv0 * (1 - MOM) + v * unb * MOM
        out = {"running_mean": (rm, MOM * e_m + 4 * U * rm.abs()),
               "running_var": (rv, MOM * unb * e_v + 4 * U * rv.abs())}
    else:
        m, v, e_m, e_v, out = rm0, rv0, 0 * rm0, 0 * rv0, {}
    r = (v + EPS) ** -0.5
    e_r = r * (0.5 * e_v / (v + EPS) + 4 * U)
    sc = gamma * r
    e_sc = gamma.abs() * e_r + 2 * U * sc.abs()
    sh = beta - m * sc
    e_sh = 2 * U * (beta.abs() + (m * sc).abs()) + m.abs() * e_sc + sc.abs() * e_m
    out.update(mean=(m, e_m), rstd=(r, e_r), scale=(sc, e_sc), shift=(sh, e_sh))
    ks, kh = k["scale"], k["shift"]
    y = (x * ks + kh).clamp_min(0)
    out["y"] = (y, u * y + 4 * U * ((x * ks).abs() + kh.abs()))
    if "gy" not in k:
        return out
    gp = k["gy"] * (k["y"] > 0)
    km, kr = k["mean"], k["rstd"]
    gb, agb = gp.sum(0), gp.abs().sum(0)
    gw = kr * ((gp * x).sum(0) - km * gb)
    agw = kr * ((gp * x).abs().sum(0) + km.abs() * agb)
    out["gb"] = (gb, u * gb.abs() + 2 * n * U * agb)
    out["gw"] = (gw, u * gw.abs() + 2 * n * U * agw)
    p1 = gamma * kr
    p3 = -gamma * kr * kr * k["gw"] / n
    p2a, p2b = -p1 * k["gb"] / n, -p3 * km
    out["coef"] = (torch.stack([p1, p2a + p2b, p3]), 8 * U * torch.stack(
        [p1.abs(), p2a.abs() + p2b.abs(), p3.abs()]))
    c1, c2, c3 = k["coef"]
    terms = [k["gslab_before"], c1 * gp, c3 * x, c2.expand_as(x)]
    gs = sum(terms)
    out["gslab"] = (gs, u * gs.abs() + 8 * U * sum(t.abs() for t in terms))
    return out


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_fp64(shape, dtype, training):
    n, h, w, c0, g, layers = shape
    if dtype == torch.float32:
        c0, g = c0 // 2, g // 2
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    ctot, rows = c0 + g * layers, n * h * w
    e, dev = dispatch.ext(), "cuda"
    torch.manual_seed(c0 + rows)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    mat = lambda t: d(t).permute(0, 2, 3, 1).reshape(rows, -1)  # noqa: E731

    def feature(c):  # per-channel mean in {0, 4}, std in {1, 0.05}
        ch = torch.arange(c, device=dev)
        mean = 4.0 * (ch % 2).view(1, -1, 1, 1)
        std = (1.0 - 0.95 * ((ch // 2) % 2)).view(1, -1, 1, 1)
        return cl((torch.randn(n, c, h, w, device=dev) * std + mean).to(dtype))

    slab = cl(torch.full((n, ctot, h, w), 7.0, device=dev, dtype=dtype))
    sums = torch.full((2, ctot), float("nan"), device=dev)
    want_slab, c = slab.clone(), 0
    for i in range(layers + 1):
        y = feature(c0 if i == 0 else g)
        cg = y.shape[1]
        e.dense_append(slab, y, c, sums if training else None)
        want_slab[:, c:c + cg] = y
        assert torch.equal(slab, want_slab), "append: slice or its surroundings"
        assert torch.equal(e.dense_take(slab, c, cg), y), "take"
        if training:
            yd, s = mat(y), d(sums[:, c:c + cg])
            m, v = yd.mean(0), yd.var(0, unbiased=False)
            km = s[0] / rows
            for name, got, want, bound in (
                    ("sum mean", km, m, 16 * U * (m.abs() + v.sqrt())),
                    ("sum var", s[1] / rows - km * km, v, 64 * U * (m * m + v))):
                over = ((got - want).abs() / (2 * bound).clamp_min(1e-300)).max()
                print(f"append {i} {name}: max err/(2*bound) = {over:.3f}")
                assert over <= 1.0, name
        c += cg
        if i == layers:
            break
        # norm1 of layer i + 1 on the prefix [0, c)
        gamma = torch.rand(c, device=dev) + 0.5
        beta = torch.randn(c, device=dev)
        rm0, rv0 = torch.randn(c, device=dev), torch.rand(c, device=dev) + 0.5
        rm, rv = rm0.clone(), rv0.clone()
        names = ("y", "mean", "rstd", "scale", "shift")
        k = dict(zip(names, e.dense_bn_fwd(slab, c, sums if training else None,
                                           gamma, beta, rm, rv, MOM, EPS,
                                           training)))
        assert k["y"].shape == (n, c, h, w) and k["y"].dtype == dtype
        assert k["y"].is_contiguous(memory_format=torch.channels_last)
        k.update(running_mean=rm, running_var=rv)
        if training:
            k["gy"] = cl(torch.randn(n, c, h, w, device=dev).to(dtype))
            gslab = cl(torch.randn(n, ctot, h, w, device=dev).to(dtype))
            before = gslab.clone()
            k["gw"], k["gb"], k["coef"] = e.dense_bn_bwd(
                k["gy"], slab, c, gslab, k["mean"], k["rstd"], gamma,
                k["scale"], k["shift"])
            assert torch.equal(gslab[:, c:], before[:, c:]), "gslab beyond cin"
            k.update(gslab=gslab[:, :c], gslab_before=before[:, :c])
        else:
            assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
        kd = {a: mat(t) if t.dim() == 4 else d(t) for a, t in k.items()}
        ref = slab_ref(mat(slab)[:, :c], d(sums[:, :c]), d(gamma), d(beta),
                       d(rm0), d(rv0), kd, training, u)
        for name, (want, bound) in ref.items():
            err = (kd[name] - want).abs()
            over = (err / (2 * bound).clamp_min(1e-300)).max().item()
            print(f"layer {i + 1} {name}: max err/(2*bound) = {over:.3f}")
            assert over <= 1.0, name


def test_block_vs_fp64_and_concat(monkeypatch):
    from distribuuuu_amd.models.densenet import _DenseBlock

    torch.manual_seed(21)
    bf, dev = torch.bfloat16, "cuda"
    ref_block = _DenseBlock(3, 16, 4, 8, 0.0)
    with torch.no_grad():
        for name, p in ref_block.named_parameters():
            if "norm" in name:
                p.copy_(torch.rand_like(p) + 0.5 if name.endswith("weight")
                        else 0.2 * torch.randn_like(p))
            p.copy_(p.to(bf))
    x0 = torch.randn(2, 16, 9, 7).to(bf).contiguous(
        memory_format=torch.channels_last)
    gout = torch.randn(2, 40, 9, 7).to(bf).contiguous(
        memory_format=torch.channels_last)

    def run(block, x, g):
        x = x.clone().requires_grad_()
        out = block(x)
        out.backward(g.clone())  # the slab path accumulates into it in place
        return out, [out.detach(), x.grad] + [p.grad for p in block.parameters()]

    _, want = run(copy.deepcopy(ref_block).double(), x0.double(), gout.double())
    rel, got = {}, {}
    for knob in ("1", "1", "0"):
        monkeypatch.setenv("DISTRIBUUUU_DENSE_SLAB", knob)
        block = copy.deepcopy(ref_block).to(dev).to(bf).to(
            memory_format=torch.channels_last)
        for mod in block.modules():
            if hasattr(mod, "running_mean"):
                mod.float()
        warned = set(dispatch._WARNED)
        out, res = run(block, x0.to(dev), gout.to(dev))
        assert dispatch._WARNED == warned, "an ATen fallback warning fired"
        part = getattr(out, "_bn_partials", None)
        if knob == "1":
            assert part is not None and part.shape == (1, 2 * 40)
            if "1" in got:
                assert all(torch.equal(a, b) for a, b in zip(got["1"], res)), \
                    "two slab runs differ"
        got[knob] = res
        rel[knob] = [((a.double().cpu() - b).abs().max() / b.abs().max()).item()
                     for a, b in zip(res, want)]
    names = ["out", "gx"] + [k for k, _ in ref_block.named_parameters()]
    for name, s, c in zip(names, rel["1"], rel["0"]):
        print(f"{name}: slab {s:.3e} concat {c:.3e}")
    for name, s, c in zip(names, rel["1"], rel["0"]):
        assert s <= 2 * c, (name, s, c)


def test_captured_step_matches_eager():
    from distribuuuu_amd.graph_step import GraphedTrainStep
    from distribuuuu_amd.models.densenet import DenseNet
    from distribuuuu_amd.ops import functional as DF
    from distribuuuu_amd.ops.optim import HIPSGD

    bf, dev = torch.bfloat16, "cuda"
    torch.manual_seed(4)
    x = torch.randn(4, 3, 32, 32, device=dev).to(bf).contiguous(
        memory_format=torch.channels_last)
    t = torch.randint(0, 10, (4,), device=dev)
    losses = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(9)
        net = DenseNet(8, (2, 2), 16, num_classes=10).to(dev).to(bf)
        for mod in net.modules():
            if hasattr(mod, "running_mean"):
                mod.float()
        net = net.to(memory_format=torch.channels_last).train()
        opt = HIPSGD(net.parameters(), lr=0.05, momentum=0.9, nesterov=True)
        step = GraphedTrainStep(net, DF.cross_entropy, opt, 5,
                                warmup=2 if mode == "graph" else 10 ** 9,
                                dtype=bf)
        losses[mode] = [step(x, t)[0].item() for _ in range(4)]
        if mode == "graph":
            assert step.stats["replays"] == 2, step.stats
    print(losses)
    assert losses["graph"] == losses["eager"]
    assert losses["eager"][0] != losses["eager"][-1]
