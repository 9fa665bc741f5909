"""Soft-target training: label smoothing, mixup and CutMix
(cfg.TRAIN.LABEL_SMOOTH / MIXUP_ALPHA / CUTMIX_ALPHA / MIX_PROB /
MIX_SWITCH_PROB).

``SoftTargetCriterion`` is the trainer's loss object when any of those keys is
set. It does two things per batch:

* ``mix(inputs)`` draws this batch's mode, lambda and box ON THE HOST, writes
  lambda into a one-element float32 device tensor (``fill_``: no ``.item()``,
  no sync) and mixes the batch with its own reversal in one ``batch_mix``
  kernel. It runs before the step, eager or captured.
* ``criterion(logits, targets)`` is ``cross_entropy`` on the soft targets; the
  loss kernels READ lambda from that tensor, so a hipGraph replay of the step
  follows the value of the batch it runs on.

Sample n is always paired with sample N-1-n and the whole batch shares one
lambda (and one box), so neither a permutation nor a per-sample weight tensor
exists.
"""

import math

import numpy as np
import torch

from . import utils
from .ops import functional as DF


class SoftTargetCriterion:
    def __init__(self, label_smoothing=0.0, mixup_alpha=0.0, cutmix_alpha=0.0,
                 prob=1.0, switch_prob=0.5, seed=None):
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError("label_smoothing must be in [0, 1)")
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("mixup_alpha / cutmix_alpha must be >= 0")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("prob / switch_prob must be in [0, 1]")
        self.label_smoothing = float(label_smoothing)
        self.mixup_alpha = float(mixup_alpha)
        self.cutmix_alpha = float(cutmix_alpha)
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.mixing = self.mixup_alpha > 0 or self.cutmix_alpha > 0
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (1 << 63))
        self.seed = int(seed)
        self._rng = np.random.default_rng([self.seed, utils.get_rank()])
        # float32[1] on the inputs' device, allocated at the first mix()
        # (always an eager call: nothing is allocated while a stream captures)
        self.lam = None
        # host record of the latest draw: (mode, lam, box)
        self.last = ("none", 1.0, None)

    def set_epoch(self, epoch):
        """Reseed the draws from (seed, rank, epoch): a run resumed at an
        epoch boundary draws what the uninterrupted run drew."""
        self._rng = np.random.default_rng(
            [self.seed, utils.get_rank(), int(epoch)])

    def draw(self, h, w):
        """This batch's (mode, lam, box) for h x w images; host only."""
        rng = self._rng
        if not self.mixing or rng.random() >= self.prob:
            return "none", 1.0, None
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            a = self.mixup_alpha
            return "mixup", float(rng.beta(a, a)), None
        a = self.cutmix_alpha
        r = math.sqrt(1.0 - float(rng.beta(a, a)))
        ch, cw = int(h * r), int(w * r)
        cy, cx = int(rng.integers(h)), int(rng.integers(w))
        y0, y1 = _clip(cy - ch // 2, h), _clip(cy + ch // 2, h)
        x0, x1 = _clip(cx - cw // 2, w), _clip(cx + cw // 2, w)
        lam = 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)
        return "cutmix", lam, (y0, y1, x0, x1)

    def mix(self, inputs):
        """Draw, publish lambda on the device, mix. Returns the inputs as they
        came when this batch is not mixed (no launch)."""
        if not self.mixing:
            return inputs
        if self.lam is None:
            self.lam = torch.ones(1, dtype=torch.float32,
                                  device=inputs.device)
        mode, lam, box = self.last = self.draw(inputs.shape[2],
                                               inputs.shape[3])
        self.lam.fill_(lam)
        if mode == "none":
            return inputs
        return DF.batch_mix(inputs, lam, box)

    def __call__(self, logits, targets):
        return DF.cross_entropy(logits, targets,
                                label_smoothing=self.label_smoothing,
                                lam=self.lam if self.mixing else None)


def _clip(v, hi):
    return min(max(v, 0), hi)
