"""TRAIN.COMPILE_GRAPH without a GPU: the runner falls back to the eager loop
body and trains exactly as with the knob off; the host-side parts of HIPSGD's
device-rate mode and its generation counter."""

import pytest
import torch

from distribuuuu_amd import models, trainer, utils
from distribuuuu_amd.config import cfg
from distribuuuu_amd.graph_step import GraphedTrainStep
from distribuuuu_amd.ops import functional as DF
from distribuuuu_amd.ops.optim import HIPSGD


@pytest.fixture
def small_cfg(tmp_path):
    saved = cfg.clone()
    cfg.defrost()
    cfg.OUT_DIR = str(tmp_path)
    cfg.MODEL.NUM_CLASSES = 10
    cfg.TRAIN.BATCH_SIZE = 4
    cfg.TRAIN.PRINT_FREQ = 1
    cfg.TRAIN.DTYPE = "float32"
    cfg.TRAIN.CHANNELS_LAST = False
    cfg.OPTIM.MAX_EPOCH = 2
    cfg.OPTIM.WARMUP_EPOCHS = 1
    yield cfg
    cfg.defrost()
    cfg.merge_from_other_cfg(saved)


def _batches():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(4, 3, 32, 32, generator=g),
             torch.randint(0, 10, (4,), generator=g)) for _ in range(3)]


def _train(knob, runner_factory=None):
    """Two CPU epochs of resnet18 from a fixed seed; returns (state, runner)."""
    cfg.TRAIN.COMPILE_GRAPH = knob
    torch.manual_seed(11)
    net = models.build_model("resnet18", num_classes=10)
    opt = HIPSGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5,
                 nesterov=True)
    runner = runner_factory(net, opt) if runner_factory else None
    dev = torch.device("cpu")
    for epoch in range(2):
        trainer.train_epoch(_batches(), net, DF.cross_entropy, opt, epoch,
                            dev, torch.float32, graph_step=runner)
    return {k: v.clone() for k, v in net.state_dict().items()}, runner


def _assert_same(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad[:5]


def test_knob_on_cpu_trains_like_knob_off(small_cfg):
    off, _ = _train(False)
    on, _ = _train(True)
    _assert_same(off, on)
    assert int(on["bn1.num_batches_tracked"]) == 6


def test_runner_on_cpu_reports_fallback(small_cfg):
    off, _ = _train(False)
    on, runner = _train(False, lambda net, opt: GraphedTrainStep(
        net, DF.cross_entropy, opt, cfg.TRAIN.TOPK, warmup=2))
    _assert_same(off, on)
    s = runner.stats
    assert s["captured"] is False
    assert isinstance(s["fallback_reason"], str) and s["fallback_reason"]
    assert s["captures"] == 0 and s["replays"] == 0
    assert s["eager_steps"] == 6


def test_runner_rejects_unfused_optimizer(small_cfg):
    net = models.build_model("resnet18", num_classes=10)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    runner = GraphedTrainStep(net, DF.cross_entropy, opt, 5)
    assert runner.stats["fallback_reason"]


def test_sync_device_lr_uploads_only_on_change():
    p = torch.nn.Parameter(torch.zeros(4))
    q = torch.nn.Parameter(torch.zeros(4))
    opt = HIPSGD([{"params": [p]}, {"params": [q], "lr": 0.5}], lr=0.1)
    assert opt.sync_device_lr() == 0          # mode off: nothing to do
    opt.enable_device_lr()
    assert [t.dtype for t in opt._lr_dev] == [torch.float32] * 2
    assert [t.item() for t in opt._lr_dev] == [
        torch.tensor(0.1).item(), 0.5]
    assert opt.sync_device_lr() == 0          # unchanged
    before = [t.data_ptr() for t in opt._lr_dev]
    utils.set_lr(opt, 0.2)
    assert opt.sync_device_lr() == 2
    assert opt.sync_device_lr() == 0
    opt.param_groups[1]["lr"] = 0.0
    assert opt.sync_device_lr() == 1
    assert [t.item() for t in opt._lr_dev] == [torch.tensor(0.2).item(), 0.0]
    assert before == [t.data_ptr() for t in opt._lr_dev]  # in place
    # the mode is not part of the serialized state
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == set(
        torch.optim.SGD([p], lr=0.1).state_dict()["param_groups"][0])
    # on the CPU the mode cannot drive the fused kernel, and says so
    assert opt.device_lr_blocker()
    opt.disable_device_lr()
    assert opt.sync_device_lr() == 0


def test_generation_counts_state_replacement():
    p = torch.nn.Parameter(torch.ones(4))
    opt = HIPSGD([p], lr=0.1, momentum=0.9)
    p.grad = torch.ones(4)
    opt.step()
    g0 = opt.generation
    sd = opt.state_dict()
    assert opt.generation == g0               # reading replaces nothing
    buf = opt.state[p]["momentum_buffer"]
    opt.load_state_dict(sd)
    assert opt.generation == g0 + 1
    assert opt.state[p]["momentum_buffer"] is not buf
    opt.load_state_dict(sd)
    assert opt.generation == g0 + 2


def test_step_counter_install_remove():
    with pytest.raises(ValueError):
        DF.install_step_counter(torch.zeros(1))
    DF.install_step_counter(torch.zeros(1, dtype=torch.int64))
    try:
        # CPU tensors never take the HIP path: the counter changes nothing
        x = torch.ones(64)
        y = DF.dropout(x, 0.5, True)
        assert y.shape == x.shape
    finally:
        assert DF.remove_step_counter() == 0
    assert DF._STEP_COUNTER is None
