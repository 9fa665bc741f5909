"""Soft-target training through trainer.train_epoch on the GPU: label
smoothing + mixup + CutMix, eager against hipGraph-captured, bit for bit.

Set-up as tests/test_graph_step_gpu.py (resnet18, 16 classes, batch 8, 64x64,
bf16 channels_last, RNG_SEED 3 + CUDNN.DETERMINISTIC), two epochs of five
batches. The host draws are deterministic; for seed 3 they are (checked on
the CPU by SoftTargetCriterion.draw):

    epoch 0: cutmix .2354, mixup .1758, cutmix .9961, cutmix .1826, mixup .7181
    epoch 1: cutmix .6938, mixup .6739, mixup .7166, cutmix .2920, mixup .1422

The first two steps are the runner's eager warm-up, so the eight replays see
both modes and eight different lambdas through one captured graph.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_graph_step_gpu import (  # noqa: E402,F401
    _assert_snapshots_equal, _batches, _build, _mode_off_after, _snapshot,
    det_cfg)

pytestmark = pytest.mark.gpu

SOFT_KEYS = dict(LABEL_SMOOTH=0.1, MIXUP_ALPHA=0.8, CUTMIX_ALPHA=1.0)


def _run(loader, epochs, graphed, monkeypatch, cfg, keys):
    """`epochs` calls of trainer.train_epoch with the criterion that
    train_model would build for `keys`. Returns per-epoch snapshots, the
    logged losses, the last grads, the runner, the criterion and its draws."""
    from distribuuuu_amd import trainer, utils
    from distribuuuu_amd.graph_step import GraphedTrainStep

    for k, v in keys.items():
        cfg.TRAIN[k] = v
    logged = []
    orig_update = utils.AverageMeter.update

    def update(self, val, n=1):
        if self.name == "Loss":
            logged.append(val)
        orig_update(self, val, n)

    monkeypatch.setattr(utils.AverageMeter, "update", update)
    m, opt = _build("resnet18")
    crit = trainer.build_criterion()
    draws = []
    if hasattr(crit, "mix"):
        orig_mix = crit.mix

        def mix(inputs):
            out = orig_mix(inputs)
            draws.append(crit.last)
            return out

        crit.mix = mix
    runner = None
    if graphed:
        runner = GraphedTrainStep(m, crit, opt, 5, warmup=2,
                                  dtype=torch.bfloat16)
    dev = torch.device("cuda")
    snaps = []
    for epoch in range(epochs):
        trainer.train_epoch(loader, m, crit, opt, epoch, dev, torch.bfloat16,
                            graph_step=runner)
        torch.cuda.synchronize()
        snaps.append(_snapshot(m, opt))
    grads = [p.grad.detach().clone() for p in m.parameters()]
    monkeypatch.setattr(utils.AverageMeter, "update", orig_update)
    return snaps, logged, grads, runner, crit, draws


def test_captured_soft_training_matches_eager(det_cfg, monkeypatch):
    from distribuuuu_amd.mixing import SoftTargetCriterion
    from distribuuuu_amd.ops import functional as DF

    loader = _batches([8] * 5)
    eager = _run(loader, 2, False, monkeypatch, det_cfg, SOFT_KEYS)
    graphed = _run(loader, 2, True, monkeypatch, det_cfg, SOFT_KEYS)
    assert isinstance(eager[4], SoftTargetCriterion)
    assert eager[4].seed == 3
    stats = graphed[3].stats
    print(stats, graphed[5])

    for i, (a, b) in enumerate(zip(eager[0], graphed[0])):
        _assert_snapshots_equal(a, b, f"epoch {i}")
    assert len(eager[1]) == len(graphed[1]) == 10
    assert all(x == x and abs(x) != float("inf") for x in eager[1])
    assert eager[1] == graphed[1], (eager[1], graphed[1])
    bad = [i for i, (a, b) in enumerate(zip(eager[2], graphed[2]))
           if not torch.equal(a, b)]
    assert not bad, f"last-step grads differ for params {bad[:5]}"
    assert stats["captured"] is True, stats
    assert stats["fallback_reason"] is None
    assert stats["captures"] == 1, stats
    assert stats["eager_steps"] == 2 and stats["replays"] == 8, stats

    # same draws in both runs; the replays saw both modes and moving lambdas
    assert eager[5] == graphed[5] and len(graphed[5]) == 10
    replayed = graphed[5][2:]
    assert {d[0] for d in replayed} == {"mixup", "cutmix"}
    assert len({d[1] for d in replayed}) >= 2
    lam = graphed[4].lam
    assert lam.dtype == torch.float32 and lam.numel() == 1
    assert lam.item() == torch.tensor(replayed[-1][1],
                                      dtype=torch.float32).item()

    # the keys change the run
    plain = _run(loader, 2, False, monkeypatch, det_cfg,
                 dict.fromkeys(SOFT_KEYS, 0.0))
    assert plain[4] is DF.cross_entropy and plain[5] == []
    assert plain[1] != eager[1]
    w = "model.conv1.weight"
    assert not torch.equal(plain[0][-1][w], eager[0][-1][w])


def test_smoothing_only_allocates_no_lambda_and_never_mixes(det_cfg,
                                                            monkeypatch):
    from distribuuuu_amd.ops import functional as DF

    calls = []
    orig = DF.batch_mix
    monkeypatch.setattr(DF, "batch_mix",
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    loader = _batches([8] * 4, seed=25)
    keys = dict(LABEL_SMOOTH=0.1, MIXUP_ALPHA=0.0, CUTMIX_ALPHA=0.0)
    eager = _run(loader, 1, False, monkeypatch, det_cfg, keys)
    graphed = _run(loader, 1, True, monkeypatch, det_cfg, keys)
    for run in (eager, graphed):
        assert run[4].lam is None and not run[4].mixing
        assert all(d == ("none", 1.0, None) for d in run[5])
    assert calls == []
    assert graphed[3].stats["captured"] is True, graphed[3].stats
    assert graphed[3].stats["replays"] == 2
    assert eager[1] == graphed[1] and len(eager[1]) == 4
    _assert_snapshots_equal(eager[0][0], graphed[0][0], "smoothing only")
    plain = _run(loader, 1, False, monkeypatch, det_cfg,
                 dict(LABEL_SMOOTH=0.0))
    assert plain[1] != eager[1]
