"""Deterministic mode on the GPU (docs/DETERMINISM.md).

Per kernel: with the mode on, the raw extension op called five times on the
same inputs returns bit-equal results, stays within the fp32-ATen bound of
that op's existing test, and has the dtype, shape and strides of the default
(atomic) call. Every shape is the smallest at which at least three partials
meet in one output element — two partials commute and would prove nothing.
The chunk counts in the case table follow from the split-m constants (bf16
chunk 4096 px, runtime-csteps floor 8 = 512 px, fp32 chunk 1024 px).

End to end: a seeded run with CUDNN.DETERMINISTIC repeats bit for bit, eagerly
and as a replayed hipGraph.

NOTE: on a build without the mode the end-to-end runs differ only by block
scheduling luck, so they CAN pass there. The tests that are guaranteed to fail
without the feature are the CPU ones in tests/test_deterministic.py (and the
per-kernel ones here, which need ops.set_deterministic). Do not "fix" a lucky
pass by loosening anything here.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPEATS = 5


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


@pytest.fixture(autouse=True)
def _mode_off_after():
    """The flag is process-global: leave it off for the rest of the suite."""
    from distribuuuu_amd import ops

    ops.set_deterministic(False)
    yield
    ops.set_deterministic(False)


def _det_and_default(fn):
    """fn() REPEATS times in deterministic mode + once in the default mode."""
    from distribuuuu_amd import ops

    ops.set_deterministic(False)
    default = fn()
    ops.set_deterministic(True)
    try:
        outs = [fn() for _ in range(REPEATS)]
    finally:
        ops.set_deterministic(False)
    torch.cuda.synchronize()
    return outs, default


def _assert_repeats(outs):
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(outs[0], o), (
            f"call {i} differs from call 0 in "
            f"{(outs[0] != o).sum().item()} elements")


def _assert_same_layout(got, default):
    assert got.dtype == default.dtype
    assert got.shape == default.shape
    assert got.stride() == default.stride()
    for fmt in (torch.contiguous_format, torch.channels_last):
        if got.dim() == 4:
            assert (got.is_contiguous(memory_format=fmt)
                    == default.is_contiguous(memory_format=fmt))


# (N, C, H, W, K, R, stride, pad, groups), env to force the route
WGRAD_CASES = [
    pytest.param((4, 64, 64, 64, 64, 3, 1, 1, 1), {}, id="64x64-xcd-grid"),
    pytest.param((4, 128, 64, 64, 64, 3, 1, 1, 1), {}, id="64x64-2d-grid"),
    pytest.param((5, 64, 45, 37, 72, 3, 1, 1, 1), {}, id="64x64-ragged"),
    pytest.param((4, 64, 64, 64, 64, 3, 1, 1, 4), {}, id="64x64-grouped"),
    pytest.param((4, 128, 32, 32, 128, 3, 1, 1, 1), {}, id="tr128"),
    pytest.param((8, 464, 16, 16, 464, 3, 1, 1, 2),
                 {"DISTRIBUUUU_WGRAD_128": "1"}, id="ring128-kg-tail"),
    pytest.param((4, 64, 64, 64, 64, 3, 1, 1, 1),
                 {"DISTRIBUUUU_WGRAD_RING": "1"}, id="ring"),
]


@pytest.mark.parametrize("case,env", WGRAD_CASES)
def test_wgrad_bf16(case, env, monkeypatch):
    e = _ext()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, c, h, w_, k, r, s, p, g = case
    torch.manual_seed(5)
    x = _cl(torch.randn(n, c, h, w_, device="cuda", dtype=torch.bfloat16))
    ho = (h + 2 * p - r) // s + 1
    wo = (w_ + 2 * p - r) // s + 1
    gy = _cl(torch.randn(n, k, ho, wo, device="cuda", dtype=torch.bfloat16))
    outs, default = _det_and_default(
        lambda: e.conv2d_wgrad(gy, x, r, r, s, s, p, p, 1, 1, g))
    _assert_repeats(outs)
    _assert_same_layout(outs[0], default)
    wf = torch.zeros(k, c // g, r, r, device="cuda", requires_grad=True)
    F.conv2d(x.float(), wf, None, s, p, 1, g).backward(gy.float())
    err = (outs[0].float() - wf.grad).abs().max().item()
    scale = wf.grad.abs().max().item()
    print(f"wgrad {case}: err {err} scale {scale}")
    assert err < 3e-2 * max(scale, 1.0), f"{case}: err {err} scale {scale}"


# The runtime-csteps kernels (tr128, ring128) cap their workspace at 64 MiB by
# doubling csteps (DET_WS_CAP, docs/DETERMINISM.md). A 512-deep 3x3 has
# 512 * 4608 * 4 B = 9.4 MB slots and 4 * 36 = 144 tiles, so 4 chunks already
# fill the machine and csteps is not shrunk below 64; at M = 32 * 32 * 32 =
# 32768 pixels that is 8 chunks = 75.5 MB > 64 MiB, so csteps must grow to 128,
# leaving 4 chunks (still >= 3 partials per element) and 37.7 MB.
GROW_CASE = (32, 512, 32, 32, 512, 3, 1, 1, 1)
DET_WS_CAP = 64 << 20
_grow_cache = {}


def _grow_inputs():
    """Inputs and the fp32 ATen reference, computed once for both routes."""
    if not _grow_cache:
        n, c, h, w_, k, r, s, p, g = GROW_CASE
        torch.manual_seed(11)
        x = _cl(torch.randn(n, c, h, w_, device="cuda", dtype=torch.bfloat16))
        gy = _cl(torch.randn(n, k, h, w_, device="cuda",
                             dtype=torch.bfloat16))
        wf = torch.zeros(k, c // g, r, r, device="cuda", requires_grad=True)
        F.conv2d(x.float(), wf, None, s, p, 1, g).backward(gy.float())
        _grow_cache.update(x=x, gy=gy, ref=wf.grad.detach())
    return _grow_cache["x"], _grow_cache["gy"], _grow_cache["ref"]


@pytest.mark.parametrize("env,padded", [
    pytest.param({}, False, id="tr128"),
    pytest.param({"DISTRIBUUUU_WGRAD_128": "1"}, True, id="ring128"),
])
def test_wgrad_workspace_cap_grows_csteps(env, padded, monkeypatch):
    """Without the growth the 8-chunk workspace (75.5 MB) would show in the
    allocator's peak; with it the call stays within cap + its other buffers,
    and the csteps = 128 launch still matches ATen and repeats."""
    e = _ext()
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    n, c, h, w_, k, r, s, p, g = GROW_CASE
    x, gy, ref = _grow_inputs()
    call = lambda: e.conv2d_wgrad(gy, x, r, r, s, s, p, p, 1, 1, g)
    outs, default = _det_and_default(call)
    _assert_repeats(outs)
    _assert_same_layout(outs[0], default)
    err = (outs[0].float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"wgrad grow {env}: err {err} scale {scale}")
    assert err < 3e-2 * max(scale, 1.0), f"err {err} scale {scale}"

    from distribuuuu_amd import ops

    del outs, default
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ops.set_deterministic(True)
    out = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    # everything else the call allocates: bf16 gw, and ring128's padded x
    other = out.numel() * 2
    if padded:
        other += n * (h + 2 * p) * (w_ + 2 * p) * c * 2
    slot = k * (c // g) * r * r * 4
    print(f"wgrad grow {env}: peak {peak} other {other} slot {slot}")
    assert 8 * slot > DET_WS_CAP  # the ungrown workspace would not fit
    assert peak <= DET_WS_CAP + other + (1 << 20), (peak, other)
    assert peak >= 3 * slot  # and at least 3 partials still meet


def test_wgrad_fp32():
    e = _ext()
    n, c, h, w_, k, r, s, p, g = (4, 32, 32, 32, 32, 3, 1, 1, 1)  # 4 chunks
    torch.manual_seed(2)
    x = _cl(torch.randn(n, c, h, w_, device="cuda"))
    gy = _cl(torch.randn(n, k, h, w_, device="cuda"))
    outs, default = _det_and_default(
        lambda: e.conv2d_wgrad(gy, x, r, r, s, s, p, p, 1, 1, g))
    _assert_repeats(outs)
    _assert_same_layout(outs[0], default)
    wf = torch.zeros(k, c // g, r, r, device="cuda", requires_grad=True)
    F.conv2d(x, wf, None, s, p, 1, g).backward(gy)
    print("wgrad fp32: err", (outs[0] - wf.grad).abs().max().item())
    assert torch.allclose(outs[0], wf.grad, atol=3e-2, rtol=1e-4), \
        (outs[0] - wf.grad).abs().max().item()


def test_dwconv_wgrad():
    e = _ext()
    # 4096 pixels, 4 channel packs -> 64 pixels per block -> 64 pixel blocks
    n, c, h, k, s = 4, 32, 32, 3, 1
    p = k // 2
    torch.manual_seed(6)
    x = _cl(torch.randn(n, c, h, h, device="cuda", dtype=torch.bfloat16))
    gy = _cl(torch.randn(n, c, h, h, device="cuda", dtype=torch.bfloat16))
    outs, default = _det_and_default(
        lambda: e.dwconv_wgrad(gy, x, k, k, s, s, p, p))
    _assert_repeats(outs)
    _assert_same_layout(outs[0], default)
    wr = torch.zeros(c, 1, k, k, device="cuda", requires_grad=True)
    F.conv2d(x.float(), wr, None, s, p, 1, c).backward(gy.float())
    err = (outs[0].float() - wr.grad).abs().max().item()
    print("dwconv_wgrad: err", err, "scale", wr.grad.abs().max().item())
    assert err < 3e-2 * max(wr.grad.abs().max().item(), 1)


def test_se_scale_bwd():
    e = _ext()
    n, c, h = 2, 32, 32  # HW = 1024 in ceil(768/2) = 384 chunks of 3 rows
    torch.manual_seed(0)
    x = _cl(torch.randn(n, c, h, h, device="cuda", dtype=torch.bfloat16))
    s = torch.rand(n, c, 1, 1, device="cuda", dtype=torch.bfloat16)
    gy = _cl(torch.randn_like(x))
    outs, default = _det_and_default(lambda: e.se_scale_bwd(gy, x, s))
    _assert_repeats([o[0] for o in outs])
    _assert_repeats([o[1] for o in outs])
    for got, dflt in zip(outs[0], default):
        _assert_same_layout(got, dflt)
    assert torch.equal(outs[0][0], default[0])  # gx never used atomics
    xr = x.float().requires_grad_(True)
    sr = s.float().requires_grad_(True)
    (xr * sr).backward(gy.float())
    assert torch.allclose(outs[0][0].float(), xr.grad, atol=2e-2, rtol=2e-2)
    scale = sr.grad.abs().max().item()
    err = (outs[0][1].float() - sr.grad).abs().max().item()
    print("se_scale_bwd: err", err, "scale", scale)
    assert err < 3e-2 * max(scale, 1)


# Both existing MHSA backward tests, each with its own config and bounds:
# test_conv_gpu.test_mhsa_fused_backward (n=1, heads=2, 7x7, d=32; max error
# < 6e-2 * max(scale, 1)) with the batch raised to 4 so that rows /
# rows_per_block = 4*2*49 / 128 >= 3 (4 row blocks), and
# test_kernels_gpu.test_mhsa_fwd_bwd_vs_torch (n=2, heads=4, 14x14, d=32: 13
# row blocks, M = 27 so the kernel's two m-halves are unequal, 14 and 13; mean
# and max error relative to the gradient's own scale). Every case asserts all
# three bounds.
@pytest.mark.parametrize("seed,n,heads,h,w,d", [
    pytest.param(10, 4, 2, 7, 7, 32, id="7x7-b4"),
    pytest.param(0, 2, 4, 14, 14, 32, id="14x14-b2"),
])
def test_mhsa_bwd(seed, n, heads, h, w, d):
    """mhsa_bwd's relative-position weight grads (grw, grh)."""
    from distribuuuu_amd.ops import attention as A

    e = _ext()
    torch.manual_seed(seed)
    l, bh = h * w, n * heads
    assert (bh * l + 127) // 128 >= 3  # row blocks that meet in one element
    q = torch.randn(n, heads, l, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    rel_h = torch.randn(2 * h - 1, d, device="cuda", dtype=torch.bfloat16)
    rel_w = torch.randn(2 * w - 1, d, device="cuda", dtype=torch.bfloat16)
    gout = torch.randn_like(q)
    # forward exactly as ops.attention._HIPMHSARelPos does, keeping the probs
    qf = q.reshape(bh, l, d).contiguous()
    kf = k.reshape(bh, l, d).contiguous()
    vf = v.reshape(bh, l, d).contiguous()
    rw = e.mhsa_rel_tables(qf, rel_w, bh * l, 1, 1, d, 1.0).reshape(bh, l, -1)
    rh = e.mhsa_rel_tables(qf, rel_h, bh * l, 1, 1, d, 1.0).reshape(bh, l, -1)
    P = torch.empty(bh, l, l, dtype=q.dtype, device="cuda")
    e.mhsa_fwd(qf, kf, vf.transpose(1, 2).contiguous(), rw, rh, h, w, P, 1, d,
               d, 1.0)
    kt = kf.transpose(1, 2).contiguous()
    dO = gout.reshape(bh, l, d).contiguous()

    def bwd():
        dqk = torch.empty(2, bh, l, d, dtype=q.dtype, device="cuda")
        dvb = torch.empty(bh, l, d, dtype=q.dtype, device="cuda")
        return e.mhsa_bwd(dO, P, qf, kt, vf, rel_w, rel_h, h, w, 1, d,
                          bh * l * d, d, d, 1.0, dqk, dvb)

    outs, default = _det_and_default(bwd)
    for j in range(4):  # dqk, dv, grw, grh
        _assert_repeats([o[j] for o in outs])
        _assert_same_layout(outs[0][j], default[j])
    qr, kr, vr, rhr, rwr = (t.float().requires_grad_(True)
                            for t in (q, k, v, rel_h, rel_w))
    A._torch_mhsa(qr, kr, vr, rhr, rwr, h, w).backward(gout.float())
    for name, got, ref in (("grw", outs[0][2], rwr.grad),
                           ("grh", outs[0][3], rhr.grad)):
        assert got.shape == ref.shape
        err = (got.float() - ref).abs()
        scale_max = ref.abs().max().item()
        scale_mean = ref.abs().mean().item()
        print(f"mhsa_bwd {name}: err max {err.max().item()} mean "
              f"{err.mean().item()} scale max {scale_max} mean {scale_mean}")
        assert err.max().item() < 6e-2 * max(scale_max, 1.0), (name, err.max())
        assert err.mean().item() < 0.02 * (scale_mean + 0.1), \
            (name, err.mean().item(), scale_mean)
        assert err.max().item() < 0.05 * scale_max + 0.3, (name, err.max())


def test_ce_fwd():
    e = _ext()
    torch.manual_seed(0)
    logits = torch.randn(64, 1000, device="cuda")
    target = torch.randint(0, 1000, (64,), device="cuda")
    outs, default = _det_and_default(lambda: e.ce_fwd(logits, target))
    _assert_repeats([o[0] for o in outs])
    _assert_repeats([o[1] for o in outs])
    for got, dflt in zip(outs[0], default):
        _assert_same_layout(got, dflt)
    ref = F.cross_entropy(logits, target)
    print("ce_fwd: diff", (outs[0][0] - ref).abs().item())
    assert torch.allclose(outs[0][0], ref, atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
@pytest.fixture
def det_cfg(tmp_path):
    """cfg with RNG_SEED 3 + CUDNN.DETERMINISTIC, restored afterwards."""
    from distribuuuu_amd.config import cfg

    saved = cfg.clone()
    cudnn = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    cfg.defrost()
    cfg.RNG_SEED = 3
    cfg.CUDNN.DETERMINISTIC = True
    cfg.OUT_DIR = str(tmp_path)
    yield cfg
    cfg.defrost()
    cfg.merge_from_other_cfg(saved)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = cudnn


def _build(arch, im, batch):
    """setup_seed() + model + fused SGD + one fixed synthetic batch."""
    from distribuuuu_amd import models, ops, utils
    from distribuuuu_amd.ops.optim import HIPSGD

    utils.setup_seed()
    assert ops.is_deterministic()
    m = models.build_model(arch, num_classes=16).to("cuda").to(torch.bfloat16)
    for mod in m.modules():
        if hasattr(mod, "running_mean"):
            mod.float()
    m = m.to(memory_format=torch.channels_last)
    m.train()
    opt = HIPSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-5,
                 nesterov=True)
    x = _cl(torch.randn(batch, 3, im, im, device="cuda",
                        dtype=torch.bfloat16))
    t = torch.randint(0, 16, (batch,), device="cuda")
    return m, opt, x, t


def _snapshot(m, opt):
    snap = {f"model.{k}": v.detach().clone()
            for k, v in m.state_dict().items()}
    for i, p in enumerate(m.parameters()):
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                snap[f"opt.{i}.{k}"] = v.detach().clone()
    return snap


def _assert_snapshots_equal(a, b):
    assert a.keys() == b.keys()
    assert any(k.endswith("momentum_buffer") for k in a)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{len(bad)} of {len(a)} tensors differ, e.g. {bad[:5]}"


def _seeded_run(arch, im, batch, steps):
    from distribuuuu_amd.ops import functional as DF

    m, opt, x, t = _build(arch, im, batch)
    losses = []
    for _ in range(steps):
        loss = DF.cross_entropy(m(x).float(), t)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    snap = _snapshot(m, opt)
    snap["losses"] = torch.stack(losses)
    assert torch.isfinite(snap["losses"]).all()
    return snap


@pytest.mark.parametrize("arch,im,batch,steps", [
    ("resnet18", 64, 8, 3),
    ("efficientnet_b0", 64, 8, 1),   # depthwise + SE
    # MHSA is built for a 14x14 map, i.e. a 224 input; batch 8 because the
    # fc's MFMA GEMM backward reduces over the batch and needs it 8-aligned
    ("botnet50", 224, 8, 1),
])
def test_seeded_training_repeats(det_cfg, arch, im, batch, steps):
    a = _seeded_run(arch, im, batch, steps)
    b = _seeded_run(arch, im, batch, steps)
    _assert_snapshots_equal(a, b)


def test_graph_replay_repeats(det_cfg):
    """One deterministic resnet18 step captured after an eager warm-up (the
    bench.py pattern), replayed twice from identical restored weights."""
    from distribuuuu_amd.ops import functional as DF

    m, opt, x, t = _build("resnet18", 64, 8)

    def step():
        loss = DF.cross_entropy(m(x).float(), t)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()

    def eager_step():  # drained: see bench.py on the SGD chunk table
        step()
        torch.cuda.synchronize()

    eager_step()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(2):
            eager_step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    torch.cuda.synchronize()

    # live tensors the graph reads and writes: restore them in place
    live = dict(m.state_dict())
    for i, p in enumerate(m.parameters()):
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                live[f"opt.{i}.{k}"] = v
    start = {k: v.detach().clone() for k, v in live.items()}

    results = []
    for _ in range(2):
        with torch.no_grad():
            for k, v in live.items():
                v.copy_(start[k])
        graph.replay()
        torch.cuda.synchronize()
        snap = _snapshot(m, opt)
        snap["loss"] = loss.clone()
        results.append(snap)
    _assert_snapshots_equal(*results)
    # the replay did train: weights moved away from the restored state
    assert any(not torch.equal(results[0][f"model.{k}"], start[k])
               for k in m.state_dict())
