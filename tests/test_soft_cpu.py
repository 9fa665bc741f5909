"""Soft-target training off the GPU: config keys, the trainer's criterion
choice, the CPU compositions of functional.cross_entropy / batch_mix, and the
host-side draws of mixing.SoftTargetCriterion."""

import glob
import math
import os

import pytest
import torch
import torch.nn.functional as F

from distribuuuu_amd import models, trainer, utils
from distribuuuu_amd.config import cfg, merge_from_file, reset_cfg
from distribuuuu_amd.mixing import SoftTargetCriterion
from distribuuuu_amd.ops import functional as DF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# config + criterion choice
# ---------------------------------------------------------------------------
def test_new_keys_default_off_and_presets_load():
    assert cfg.TRAIN.LABEL_SMOOTH == 0.0
    assert cfg.TRAIN.MIXUP_ALPHA == 0.0
    assert cfg.TRAIN.CUTMIX_ALPHA == 0.0
    assert cfg.TRAIN.MIX_PROB == 1.0
    assert cfg.TRAIN.MIX_SWITCH_PROB == 0.5
    presets = sorted(glob.glob(os.path.join(REPO, "config", "*.yaml")))
    assert len(presets) == 7
    for preset in presets:
        reset_cfg()
        merge_from_file(preset)
        assert cfg.TRAIN.LABEL_SMOOTH == 0.0 and cfg.TRAIN.MIXUP_ALPHA == 0.0
    cfg.merge_from_list(["TRAIN.LABEL_SMOOTH", "0.1", "TRAIN.MIXUP_ALPHA",
                         "1", "TRAIN.CUTMIX_ALPHA", "1.0"])
    assert cfg.TRAIN.LABEL_SMOOTH == 0.1
    assert cfg.TRAIN.MIXUP_ALPHA == 1.0 and cfg.TRAIN.CUTMIX_ALPHA == 1.0


def test_criterion_is_plain_cross_entropy_at_defaults():
    assert trainer.build_criterion() is DF.cross_entropy
    assert not hasattr(DF.cross_entropy, "mix")


@pytest.mark.parametrize("key,val", [("LABEL_SMOOTH", 0.1),
                                     ("MIXUP_ALPHA", 0.8),
                                     ("CUTMIX_ALPHA", 1.0)])
def test_any_key_selects_soft_criterion(key, val):
    cfg.RNG_SEED = 5
    cfg.TRAIN[key] = val
    cfg.TRAIN.MIX_PROB = 0.75
    cfg.TRAIN.MIX_SWITCH_PROB = 0.25
    crit = trainer.build_criterion(rank=2)
    assert isinstance(crit, SoftTargetCriterion)
    assert crit.seed == 7
    assert (crit.prob, crit.switch_prob) == (0.75, 0.25)
    assert crit.mixing == (key != "LABEL_SMOOTH")
    assert getattr(crit, {"LABEL_SMOOTH": "label_smoothing",
                          "MIXUP_ALPHA": "mixup_alpha",
                          "CUTMIX_ALPHA": "cutmix_alpha"}[key]) == val


# ---------------------------------------------------------------------------
# functional.cross_entropy on CPU
# ---------------------------------------------------------------------------
def _q(target, k, eps, lam):
    """fp64 soft targets straight from the definition."""
    a = F.one_hot(target, k).double()
    b = F.one_hot(target.flip(0), k).double()
    return (1 - eps) * (lam * a + (1 - lam) * b) + eps / k


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("eps,lam", [(0.1, None), (0.0, 0.3), (0.1, 0.3),
                                     (0.1, 0.0), (0.5, 0.5)])
def test_cross_entropy_soft_matches_prob_targets(n, eps, lam):
    g = torch.Generator().manual_seed(n)
    k = 10
    logits = torch.randn(n, k, generator=g).requires_grad_(True)
    target = torch.randint(0, k, (n,), generator=g)
    lam_t = None if lam is None else torch.tensor([lam], dtype=torch.float32)
    loss = DF.cross_entropy(logits, target, label_smoothing=eps, lam=lam_t)
    loss.backward()
    ref_in = logits.detach().double().requires_grad_(True)
    lam64 = 1.0 if lam is None else float(lam_t.item())
    ref = F.cross_entropy(ref_in, _q(target, k, eps, lam64))
    ref.backward()
    assert torch.allclose(loss.double(), ref, rtol=1e-5, atol=1e-6)
    assert torch.allclose(logits.grad.double(), ref_in.grad, rtol=1e-5,
                          atol=1e-7)
    if lam is None:
        # the definition at lam = 1 is torch's own label smoothing
        own = F.cross_entropy(logits.detach(), target, label_smoothing=eps)
        assert torch.allclose(loss, own, rtol=1e-5, atol=1e-6)


def test_cross_entropy_positional_use_unchanged():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(5, 7, generator=g)
    target = torch.randint(0, 7, (5,), generator=g)
    assert torch.equal(DF.cross_entropy(logits, target),
                       F.cross_entropy(logits, target))
    with pytest.raises(ValueError):
        DF.cross_entropy(logits, target, label_smoothing=1.0)


# ---------------------------------------------------------------------------
# functional.batch_mix on CPU: the same equalities the kernel is held to
# ---------------------------------------------------------------------------
def _x(n, c, h, w, dtype, cl, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g).to(dtype)
    return x.contiguous(memory_format=torch.channels_last) if cl else x


def _boxes(h, w):
    return [(0, 0, 0, 0), (0, h, 0, w), (h - 1, h, w - 1, w),
            (1, h - 1, 1, w - 2), (1, 3, 0, w)]


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_batch_mix_cpu_composition(n, dtype, cl):
    c, h, w = 3, 7, 5
    x = _x(n, c, h, w, dtype, cl)
    keep = x.clone()
    fmt = torch.channels_last if cl else torch.contiguous_format
    for box in _boxes(h, w):
        out = DF.batch_mix(x, 1.0, box)
        inside = torch.zeros(1, 1, h, w, dtype=torch.bool)
        inside[:, :, box[0]:box[1], box[2]:box[3]] = True
        assert torch.equal(out, torch.where(inside, x.flip(0), x))
        assert out.dtype == dtype and out.is_contiguous(memory_format=fmt)
    assert torch.equal(DF.batch_mix(x, 1.0), x)
    assert DF.batch_mix(x, 1.0).data_ptr() != x.data_ptr()
    assert torch.equal(DF.batch_mix(x, 0.0), x.flip(0))
    for lam in (0.3, 0.9371):
        out = DF.batch_mix(x, lam)
        assert out.dtype == dtype and out.is_contiguous(memory_format=fmt)
        l32 = float(torch.tensor(lam, dtype=torch.float32))
        a, b = x.double(), x.flip(0).double()
        ref = l32 * a + (1 - l32) * b
        b32 = 4 * 2.0 ** -24 * ((l32 * a).abs() + ((1 - l32) * b).abs())
        bound = b32 if dtype == torch.float32 else \
            b32 + 2.0 ** -8 * (ref.abs() + b32)
        assert ((out.double() - ref).abs() <= bound).all()
    assert torch.equal(x, keep)
    with pytest.raises(ValueError):
        DF.batch_mix(x, 0.5, (0, h + 1, 0, w))
    with pytest.raises(ValueError):
        DF.batch_mix(x, 1.5)


# ---------------------------------------------------------------------------
# SoftTargetCriterion: host draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(224, 224), (64, 64), (7, 5), (1, 9),
                                (32, 200)])
def test_cutmix_lambda_is_box_area_and_box_stays_inside(hw):
    h, w = hw
    crit = SoftTargetCriterion(0.0, 0.0, 1.0, seed=hw[0] * 1000 + hw[1])
    areas = set()
    for _ in range(1000):
        mode, lam, (y0, y1, x0, x1) = crit.draw(h, w)
        assert mode == "cutmix"
        assert 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
        assert lam == 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)
        assert 0.0 <= lam <= 1.0
        areas.add((y1 - y0) * (x1 - x0))
    if h > 1:  # a 1-pixel-high image only has the empty box (ch = 0)
        assert len(areas) > 3


def test_draw_modes_follow_the_knobs():
    both = SoftTargetCriterion(0.1, 0.8, 1.0, prob=0.5, switch_prob=0.5,
                               seed=1)
    modes = [both.draw(32, 32)[0] for _ in range(400)]
    counts = {m: modes.count(m) for m in ("none", "mixup", "cutmix")}
    # binomial(400, .5) and (400, .25): 6 sigma is 60 and 52
    assert abs(counts["none"] - 200) < 60, counts
    assert abs(counts["mixup"] - 100) < 52 and abs(counts["cutmix"] - 100) < 52
    only_mix = SoftTargetCriterion(0.0, 0.4, 0.0, seed=2)
    draws = [only_mix.draw(8, 8) for _ in range(50)]
    assert all(m == "mixup" and box is None and 0.0 <= lam <= 1.0
               for m, lam, box in draws)
    assert len({lam for _, lam, _ in draws}) > 10
    off = SoftTargetCriterion(0.1, 0.0, 0.0, seed=3)
    assert off.draw(8, 8) == ("none", 1.0, None) and not off.mixing


def test_set_epoch_reproduces_the_draw_sequence():
    a = SoftTargetCriterion(0.1, 0.8, 1.0, seed=11)
    b = SoftTargetCriterion(0.1, 0.8, 1.0, seed=11)
    a.set_epoch(0)
    first = [a.draw(64, 64) for _ in range(7)]
    a.set_epoch(1)
    second = [a.draw(64, 64) for _ in range(7)]
    assert first != second
    b.set_epoch(1)  # a run resumed at epoch 1
    assert [b.draw(64, 64) for _ in range(7)] == second
    b.set_epoch(0)
    assert [b.draw(64, 64) for _ in range(3)] == first[:3]
    c = SoftTargetCriterion(0.1, 0.8, 1.0, seed=12)
    c.set_epoch(1)
    assert [c.draw(64, 64) for _ in range(7)] != second


def test_mix_publishes_lambda_and_loss_reads_it():
    crit = SoftTargetCriterion(0.1, 0.8, 1.0, seed=4)
    crit.set_epoch(0)
    x = _x(4, 3, 8, 8, torch.float32, False, seed=9)
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(4, 6, generator=g)
    target = torch.randint(0, 6, (4,), generator=g)
    assert crit.lam is None
    seen = set()
    ptr = None
    for _ in range(12):
        out = crit.mix(x)
        mode, lam, box = crit.last
        seen.add(mode)
        ptr = ptr or crit.lam.data_ptr()
        assert crit.lam.data_ptr() == ptr  # one tensor, refilled
        assert crit.lam.dtype == torch.float32 and crit.lam.numel() == 1
        assert crit.lam.item() == torch.tensor(lam, dtype=torch.float32).item()
        assert torch.equal(out, DF.batch_mix(x, lam, box))
        want = F.cross_entropy(
            logits.double(), _q(target, 6, 0.1, float(crit.lam.item())))
        assert math.isclose(crit(logits, target).item(), want.item(),
                            rel_tol=1e-5)
    assert seen == {"mixup", "cutmix"}
    skip = SoftTargetCriterion(0.0, 0.8, 0.0, prob=0.0, seed=4)
    assert skip.mix(x) is x and skip.last == ("none", 1.0, None)
    assert skip.lam.item() == 1.0
    smooth = SoftTargetCriterion(0.1, seed=4)
    assert smooth.mix(x) is x and smooth.lam is None


# ---------------------------------------------------------------------------
# train_epoch with the keys on
# ---------------------------------------------------------------------------
def test_train_epoch_cpu_with_soft_targets(tmp_path, monkeypatch):
    cfg.OUT_DIR = str(tmp_path)
    cfg.RNG_SEED = 3
    cfg.MODEL.NUM_CLASSES = 10
    cfg.TRAIN.BATCH_SIZE = 4
    cfg.TRAIN.PRINT_FREQ = 1
    cfg.TRAIN.LABEL_SMOOTH = 0.1
    cfg.TRAIN.MIXUP_ALPHA = 0.8
    cfg.TRAIN.CUTMIX_ALPHA = 1.0
    utils.setup_seed(0)
    logged = []
    orig_update = utils.AverageMeter.update

    def update(self, val, n=1):
        if self.name == "Loss":
            logged.append(val)
        orig_update(self, val, n)

    monkeypatch.setattr(utils.AverageMeter, "update", update)
    g = torch.Generator().manual_seed(0)
    loader = [(torch.randn(4, 3, 32, 32, generator=g),
               torch.randint(0, 10, (4,), generator=g)) for _ in range(4)]
    net = models.build_model("resnet18", num_classes=10)
    opt = utils.construct_optimizer(net)
    crit = trainer.build_criterion()
    modes = []
    for epoch in range(2):
        trainer.train_epoch(loader, net, crit, opt, epoch,
                            torch.device("cpu"), torch.float32)
        modes.append(crit.last[0])
    assert len(logged) == 8
    assert all(math.isfinite(v) for v in logged), logged
    assert crit.lam is not None and modes[-1] in ("mixup", "cutmix")
