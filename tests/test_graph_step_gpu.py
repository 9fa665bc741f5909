"""TRAIN.COMPILE_GRAPH on the GPU: the device-rate SGD kernel, the
counter-keyed dropout kernel, HIPSGD's capture-private chunk table, and
graph_step.GraphedTrainStep driven through trainer.train_epoch.

Every comparison is torch.equal. The model runs use RNG_SEED 3 +
CUDNN.DETERMINISTIC: every kernel of the step is then ordered and kernel
routes depend on shapes and launch-time environment only, so a captured run
and an eager run of the same batches must agree to the bit.
"""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

GOLDEN = 0x9E3779B97F4A7C15
NUMELS = (1, 255, 16384, 16385, 40000)  # 1 elt, partial block, 1 chunk, +1, many


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


@pytest.fixture(autouse=True)
def _mode_off_after():
    """Process-global switches: leave them off for the rest of the suite."""
    from distribuuuu_amd import ops
    from distribuuuu_amd.ops import functional as DF

    ops.set_deterministic(False)
    yield
    ops.set_deterministic(False)
    DF.remove_step_counter()


# ---------------------------------------------------------------------------
# 1. sgd_step_dev == sgd_step
# ---------------------------------------------------------------------------
def _param_sets(dtype, numels, seed=0):
    torch.manual_seed(seed)
    base = [torch.randn(n, device="cuda").to(dtype) for n in numels]
    return ([b.clone().requires_grad_(True) for b in base],
            [b.clone().requires_grad_(True) for b in base])


def _assert_opt_equal(opt_a, pa, opt_b, pb, what):
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), f"{what}: param {i}"
        sa, sb = opt_a.state[a], opt_b.state[b]
        assert sa.keys() == sb.keys()
        assert "momentum_buffer" in sa
        for k in sa:
            if torch.is_tensor(sa[k]):
                assert torch.equal(sa[k], sb[k]), f"{what}: {k} {i}"


def _fill_grads(pa, pb, seed):
    """The same fresh gradient values into the existing grad tensors."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for a, b in zip(pa, pb):
        v = torch.randn(a.shape, device="cuda", generator=g).to(a.dtype)
        for p in (a, b):
            if p.grad is None:
                p.grad = v.clone()
            else:
                p.grad.copy_(v)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("nesterov,dampening", [
    (True, 0.0), (False, 0.0), (False, 0.1)])
def test_sgd_step_dev_matches_sgd_step(dtype, nesterov, dampening):
    from distribuuuu_amd.ops.optim import HIPSGD

    _ext()
    pa, pb = _param_sets(dtype, NUMELS)
    kw = dict(lr=0.05, momentum=0.9, dampening=dampening, weight_decay=5e-5,
              nesterov=nesterov)
    ref, dev = HIPSGD(pa, **kw), HIPSGD(pb, **kw)
    dev.enable_device_lr()
    assert dev.device_lr_blocker() is None
    lr_ptr = dev._lr_dev[0].data_ptr()
    for step, lr in enumerate((0.05, 0.2, 0.0)):
        _fill_grads(pa, pb, seed=step)
        for opt in (ref, dev):
            opt.param_groups[0]["lr"] = lr
        dev.sync_device_lr()
        ref.step()
        dev.step()
        _assert_opt_equal(ref, pa, dev, pb, f"step {step} lr {lr}")
    # the rate never went through a launch argument or a new tensor
    assert dev._lr_dev[0].data_ptr() == lr_ptr
    assert dev._lr_dev[0].item() == 0.0
    if dtype == torch.bfloat16:
        assert all("master" in dev.state[p] for p in pb)


# ---------------------------------------------------------------------------
# 2. a captured step follows the rate and owns its chunk table
# ---------------------------------------------------------------------------
def test_captured_sgd_follows_rate_and_keeps_its_table():
    from distribuuuu_amd.ops.optim import HIPSGD

    _ext()
    pa, pb = _param_sets(torch.bfloat16, (1000, 20000), seed=1)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=5e-5, nesterov=True)
    ref, dev = HIPSGD(pa, **kw), HIPSGD(pb, **kw)
    dev.enable_device_lr()

    def both(lr, seed, dev_step):
        _fill_grads(pa, pb, seed)
        for opt in (ref, dev):
            opt.param_groups[0]["lr"] = lr
        dev.sync_device_lr()
        ref.step()
        dev_step()
        _assert_opt_equal(ref, pa, dev, pb, f"seed {seed} lr {lr}")

    both(0.05, 0, dev.step)          # eager: creates momentum and masters
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.step()                   # capturing executes nothing
    private = dev._private[0]
    eager_dev = dev.param_groups[0]["_hip_table_dev"]
    assert private[1].data_ptr() != eager_dev.data_ptr()
    assert private[0].data_ptr() != \
        dev.param_groups[0]["_hip_table_pin"].data_ptr()
    assert private[0].is_pinned()
    table = private[0].clone()

    both(0.3, 1, graph.replay)       # rate A
    # what used to break a captured step: state_dict() drops the eager
    # table, the allocator hands its memory out again, an eager step of the
    # same optimizer builds a table of its own
    dev.state_dict()
    assert "_hip_table_dev" not in dev.param_groups[0]
    junk = [torch.full(table.shape, -1, dtype=torch.int64, device="cuda")
            for _ in range(4)]
    junk += [torch.full(table.shape, -1, dtype=torch.int64).pin_memory()
             for _ in range(4)]
    del junk
    both(0.3, 2, dev.step)           # eager step in between
    assert dev._private[0][0] is private[0]
    assert torch.equal(private[0], table)  # eager never wrote it
    both(0.01, 3, graph.replay)      # rate B
    both(0.0, 4, graph.replay)
    del graph
    dev.release_capture_tables()
    assert dev._private is None


# ---------------------------------------------------------------------------
# 3. dropout keyed by a device step counter
# ---------------------------------------------------------------------------
def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("numel", [5, 70001])
def test_dropout_fwd_dev_matches_host_seed(dtype, numel):
    e = _ext()
    torch.manual_seed(numel)
    x = torch.randn(numel, device="cuda").to(dtype)
    salt = 0x2545F4914F6CDD1D & ((1 << 62) - 1)
    outs = []
    for step in (0, 1, 1 << 40):
        counter = torch.tensor([step], dtype=torch.int64, device="cuda")
        got = e.dropout_fwd_dev(x, 0.3, salt, counter)
        want = e.dropout_fwd(x, 0.3, _i64(salt + step * GOLDEN))
        assert torch.equal(got, want), f"step {step}"
        assert counter.item() == step  # read only
        outs.append(got)
    if numel > 5:
        assert not torch.equal(outs[0], outs[1])
        kept = (outs[0] != 0).float().mean().item()
        assert 0.65 < kept < 0.75, kept  # 70001 draws at keep 0.7: sd 0.0017


class _Toy(nn.Module):
    """scale -> Dropout(0.5) -> linear(32 -> 16), keeping the dropout's
    input and output so their zero patterns can be compared."""

    def __init__(self):
        super().__init__()
        from distribuuuu_amd import ops

        self.scale = nn.Parameter(torch.ones(32))
        self.drop = ops.Dropout(0.5)
        self.fc = ops.Linear(32, 16)

    def forward(self, x):
        self.h = x * self.scale
        self.h.retain_grad()
        self.y = self.drop(self.h)
        return self.fc(self.y)


def test_graphed_dropout_mask_moves_and_backward_reuses_it():
    from distribuuuu_amd.graph_step import GraphedTrainStep
    from distribuuuu_amd.ops import functional as DF
    from distribuuuu_amd.ops.optim import HIPSGD

    _ext()
    torch.manual_seed(0)
    net = _Toy().cuda().train()
    opt = HIPSGD(net.parameters(), lr=0.01, momentum=0.9)
    runner = GraphedTrainStep(net, DF.cross_entropy, opt, 5, warmup=1,
                              dtype=torch.float32)
    x = torch.randn(8, 32, device="cuda")
    t = torch.randint(0, 16, (8,), device="cuda")
    masks = []
    for i in range(4):
        loss, _, _ = runner(x, t)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        if i == 0:
            continue  # eager warm-up step
        mask = net.y != 0
        assert torch.equal(net.h.grad != 0, mask), f"replay {i}"
        assert 0 < mask.sum().item() < mask.numel()
        masks.append(mask.clone())
    assert runner.stats["captured"], runner.stats
    assert runner.stats["replays"] == 3 and runner.stats["eager_steps"] == 1
    assert not torch.equal(masks[0], masks[1])
    assert not torch.equal(masks[1], masks[2])
    assert DF._STEP_COUNTER is None  # installed around the capture only


# ---------------------------------------------------------------------------
# 4-6. captured train_epoch
# ---------------------------------------------------------------------------
@pytest.fixture
def det_cfg(tmp_path):
    """cfg with RNG_SEED 3 + CUDNN.DETERMINISTIC and the small bf16
    channels_last set-up, restored afterwards."""
    from distribuuuu_amd.config import cfg

    saved = cfg.clone()
    cudnn = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    cfg.defrost()
    cfg.RNG_SEED = 3
    cfg.CUDNN.DETERMINISTIC = True
    cfg.OUT_DIR = str(tmp_path)
    cfg.MODEL.NUM_CLASSES = 16
    cfg.TRAIN.BATCH_SIZE = 8
    cfg.TRAIN.PRINT_FREQ = 1
    cfg.TRAIN.DTYPE = "bfloat16"
    cfg.TRAIN.CHANNELS_LAST = True
    cfg.TRAIN.COMPILE_GRAPH = False  # runners are passed in explicitly
    cfg.OPTIM.WARMUP_EPOCHS = 2
    cfg.OPTIM.MAX_EPOCH = 3
    yield cfg
    cfg.defrost()
    cfg.merge_from_other_cfg(saved)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = cudnn


def _build(arch):
    """setup_seed() + model + fused SGD."""
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
    return m, opt


def _batches(sizes, seed=21):
    """Distinct fp32 NCHW device batches: the eager loop casts and converts
    in two passes, the runner in one copy."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, 64, 64, generator=g).cuda(),
             torch.randint(0, 16, (n,), generator=g).cuda()) for n in sizes]


def _snapshot(m, opt):
    snap = {f"model.{k}": v.detach().clone()
            for k, v in m.state_dict().items()}
    for i, p in enumerate(m.parameters()):
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                snap[f"opt.{i}.{k}"] = v.detach().clone()
    return snap


def _assert_snapshots_equal(a, b, what):
    assert a.keys() == b.keys()
    assert any(k.endswith("momentum_buffer") for k in a)
    assert any(k.endswith("master") for k in a)
    assert any(k.endswith("num_batches_tracked") for k in a)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (f"{what}: {len(bad)} of {len(a)} tensors differ, "
                     f"e.g. {bad[:5]}")


def _run(arch, loader, epochs, graphed, monkeypatch, reload_after=None):
    """`epochs` calls of trainer.train_epoch, each followed by a checkpoint.
    Returns per-epoch snapshots, the meter-logged losses, the last step's
    grads and the runner."""
    from distribuuuu_amd import trainer, utils
    from distribuuuu_amd.graph_step import GraphedTrainStep
    from distribuuuu_amd.ops import functional as DF

    logged = []
    orig_update = utils.AverageMeter.update

    def update(self, val, n=1):
        if self.name == "Loss":
            logged.append(val)
        orig_update(self, val, n)

    monkeypatch.setattr(utils.AverageMeter, "update", update)
    m, opt = _build(arch)
    runner = None
    if graphed:
        runner = GraphedTrainStep(m, DF.cross_entropy, opt, 5, warmup=2,
                                  dtype=torch.bfloat16)
    dev = torch.device("cuda")
    snaps, lrs = [], []
    for epoch in range(epochs):
        trainer.train_epoch(loader, m, DF.cross_entropy, opt, epoch, dev,
                            torch.bfloat16, graph_step=runner)
        torch.cuda.synchronize()
        lrs.append(opt.param_groups[0]["lr"])
        utils.save_checkpoint(m, opt, epoch, 0.0)
        if epoch == reload_after:
            opt.load_state_dict(opt.state_dict())
        snaps.append(_snapshot(m, opt))
    grads = [p.grad.detach().clone() for p in m.parameters()]
    monkeypatch.setattr(utils.AverageMeter, "update", orig_update)
    assert len(set(lrs)) == epochs  # every epoch at another rate
    return snaps, logged, grads, runner


def _assert_runs_equal(eager, graphed):
    for i, (a, b) in enumerate(zip(eager[0], graphed[0])):
        _assert_snapshots_equal(a, b, f"epoch {i}")
    assert len(eager[1]) == len(graphed[1])
    assert all(x == x and abs(x) != float("inf") for x in eager[1])
    assert eager[1] == graphed[1], (eager[1], graphed[1])
    bad = [i for i, (a, b) in enumerate(zip(eager[2], graphed[2]))
           if not torch.equal(a, b)]
    assert not bad, f"last-step grads differ for params {bad[:5]}"


def test_captured_train_epoch_matches_eager(det_cfg, monkeypatch):
    """Three epochs at three rates, a checkpoint after each, the optimizer
    state reloaded after the second (forces one re-capture)."""
    loader = _batches([8] * 5)
    eager = _run("resnet18", loader, 3, False, monkeypatch, reload_after=1)
    graphed = _run("resnet18", loader, 3, True, monkeypatch, reload_after=1)
    stats = graphed[3].stats
    print(stats)
    assert len(eager[1]) == 15
    _assert_runs_equal(eager, graphed)
    nbt = eager[0][-1]["model.bn1.num_batches_tracked"]
    assert nbt.item() == 15
    assert stats["captured"] is True, stats
    assert stats["fallback_reason"] is None
    assert stats["captures"] == 2, stats
    assert stats["replays"] + stats["eager_steps"] == 15, stats
    assert stats["eager_steps"] == 2, stats


def test_off_shape_batch_runs_eagerly_and_keeps_the_graph(det_cfg,
                                                          monkeypatch):
    loader = _batches([8, 8, 8, 4, 8, 8], seed=22)
    eager = _run("resnet18", loader, 1, False, monkeypatch)
    graphed = _run("resnet18", loader, 1, True, monkeypatch)
    stats = graphed[3].stats
    print(stats)
    _assert_runs_equal(eager, graphed)
    assert stats["captured"] is True, stats
    assert stats["captures"] == 1, stats
    assert stats["eager_steps"] == 3, stats  # two warm-up steps + the 4
    assert stats["replays"] == 3, stats


def test_knob_without_runner_keeps_one_runner_across_calls(det_cfg,
                                                           monkeypatch):
    """train_epoch with the knob set and no runner: the first call builds
    the optimizer's runner and captures, the second call replays that graph
    (no second warm-up, no second capture, no fall-back to eager), and the
    weights equal the eager run's."""
    from distribuuuu_amd import trainer
    from distribuuuu_amd.ops import functional as DF

    loader = _batches([8] * 4, seed=24)
    eager = _run("resnet18", loader, 2, False, monkeypatch)

    det_cfg.TRAIN.COMPILE_GRAPH = True
    m, opt = _build("resnet18")
    dev = torch.device("cuda")
    snaps, stats = [], []
    for epoch in range(2):
        trainer.train_epoch(loader, m, DF.cross_entropy, opt, epoch, dev,
                            torch.bfloat16)
        torch.cuda.synchronize()
        snaps.append(_snapshot(m, opt))
        stats.append(dict(opt._graph_step.stats))
    grads = [p.grad.detach().clone() for p in m.parameters()]
    print(stats)
    assert stats[0] == {"captured": True, "captures": 1, "replays": 2,
                        "eager_steps": 2, "fallback_reason": None}
    assert stats[1] == {"captured": True, "captures": 1, "replays": 6,
                        "eager_steps": 2, "fallback_reason": None}
    for i, (a, b) in enumerate(zip(eager[0], snaps)):
        _assert_snapshots_equal(a, b, f"epoch {i}")
    bad = [i for i, (a, b) in enumerate(zip(eager[2], grads))
           if not torch.equal(a, b)]
    assert not bad, f"last-step grads differ for params {bad[:5]}"


def test_efficientnet_dropout_head_captures(det_cfg, monkeypatch):
    """Integration check of the dropout path (head dropout 0.2); the mask
    itself is checked on the toy net above."""
    loader = _batches([8] * 4, seed=23)
    _, logged, _, runner = _run("efficientnet_b0", loader, 1, True,
                                monkeypatch)
    print(runner.stats, logged)
    assert len(logged) == 4
    assert all(x == x and abs(x) != float("inf") for x in logged), logged
    assert runner.stats["captured"] is True, runner.stats
    assert runner.stats["replays"] == 2
    assert runner._advance_counter  # the head's dropout took the counter
    assert runner._counter.item() == 2


# ---------------------------------------------------------------------------
# linear backward at a batch that is not a multiple of 8
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,u_out", [
    pytest.param(torch.float32, 2.0 ** -24, id="fp32"),
    pytest.param(torch.bfloat16, 2.0 ** -8, id="bf16")])
@pytest.mark.parametrize("batch", [4, 12, 16])
def test_linear_backward_unaligned_batch(batch, dtype, u_out):
    """The weight-gradient GEMM reduces over the batch and zero-pads it to a
    multiple of 8 (16 is the unpadded control). Reference: fp64 on the same
    (already rounded) inputs. Bound per element, from the formats alone:
    products of two bf16/fp32 inputs summed in fp32 over K terms are off by
    at most (K + 1) * 2^-24 * sum|a||b| (K - 1 additions and one rounding of
    each product), and the result is rounded once to the output format
    (half an ulp, i.e. the unit roundoff u_out = 2^-24 or 2^-8, times |ref|); zero padding adds exact zeros."""
    from distribuuuu_amd.ops import functional as DF

    _ext()
    torch.manual_seed(batch)
    x = torch.randn(batch, 32, device="cuda").to(dtype).requires_grad_(True)
    w = torch.randn(16, 32, device="cuda").to(dtype).requires_grad_(True)
    b = torch.randn(16, device="cuda").to(dtype).requires_grad_(True)
    gy = torch.randn(batch, 16, device="cuda").to(dtype)
    DF.linear(x, w, b).backward(gy)
    x64, w64, gy64 = (t.detach().double() for t in (x, w, gy))
    cases = {
        "gw": (w.grad, gy64.t() @ x64, gy64.abs().t() @ x64.abs(), batch),
        "gx": (x.grad, gy64 @ w64, gy64.abs() @ w64.abs(), 16),
    }
    for name, (got, ref, mag, k) in cases.items():
        assert got.shape == ref.shape and got.dtype == dtype
        err = (got.double() - ref).abs()
        bound = (k + 1) * 2.0 ** -24 * mag + u_out * ref.abs()
        print(f"linear bwd batch {batch} {dtype} {name}: max err "
              f"{err.max().item():.3e}, max err/bound "
              f"{(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (name, (err / bound).max().item())
    assert torch.equal(b.grad, gy.sum(0))
