"""hipGraph-captured train step for the trainer (cfg.TRAIN.COMPILE_GRAPH).

``GraphedTrainStep`` runs the body of ``trainer.train_epoch`` (forward, loss,
zero_grad, backward, fused SGD step, top-k accuracy) for one batch. Its first
``warmup`` batches are ordinary eager steps; the next batch is copied into
static buffers and the step is captured, and from then on every batch of that
shape is one copy plus one graph replay instead of ~900 launches with Python
in between.

A replayed graph repeats its launch arguments, so the four pieces of per-step
state that the eager loop keeps on the host live elsewhere:

* learning rate    a float32 device tensor per param group that the SGD
                   kernel reads (HIPSGD device-rate mode), refreshed by
                   ``sync_device_lr()`` when ``group["lr"]`` changes;
* dropout seed     host-drawn salt per call site (fixed at capture) plus an
                   int64 device step counter, advanced before each replay;
* BN batch count   ``_nbt_pending`` is bumped here per replay, since
                   ``forward()`` does not run;
* SGD chunk table  the captured step owns a pinned/device pair of its own
                   that eager steps and ``state_dict()`` never touch.

Anything that prevents capture (no GPU, more than one rank, an optimizer
without the fused device-rate step, an exception while capturing) is logged
once and the runner trains eagerly for the rest of the run, exactly as
``train_epoch`` does without it.
"""

import torch

from . import utils
from .config import cfg
from .logger import logger
from .ops import functional as DF
from .ops.optim import HIPSGD


class GraphedTrainStep:
    """``runner(inputs, targets) -> (loss, acc1, acck)``: one training step,
    replayed from a hipGraph where possible. ``acc1``/``acck`` are what
    ``utils.accuracy`` returns (shape-[1] percentages); after a replay all
    three are static tensors that the next replay overwrites."""

    def __init__(self, net, criterion, optimizer, topk, warmup=2,
                 device=None, dtype=None):
        self.net = net
        self.criterion = criterion
        self.optimizer = optimizer
        self.topk = topk
        # a parameter's first step cannot be captured (HIPSGD first-step flag)
        self.warmup = max(int(warmup), 1)
        self.params = [p for p in net.parameters() if p.requires_grad]
        self.device = device if device is not None else self.params[0].device
        if dtype is None:
            dtype = (torch.bfloat16 if cfg.TRAIN.DTYPE == "bfloat16"
                     else torch.float32)
        self.dtype = dtype
        self.stats = {"captured": False, "captures": 0, "replays": 0,
                      "eager_steps": 0, "fallback_reason": None}
        self._fallback = False
        self._graph = None
        self._key = None
        self._static = None     # (x, targets)
        self._out = None        # (loss, acc1, acck)
        self._grads = None      # the captured step's grad tensors
        self._state_refs = None
        self._nbt = []          # (module, bumps per step)
        self._counter = None
        self._advance_counter = False
        self._gen = None
        self._side = None
        reason = self._cannot_capture()
        if reason is not None:
            self._fall_back(reason)
        else:
            optimizer.enable_device_lr()

    # -- policy ------------------------------------------------------------
    def _cannot_capture(self):
        if not torch.cuda.is_available() or self.device.type != "cuda":
            return "no GPU"
        if utils.get_world_size() > 1:
            return ("world_size > 1: captured collectives are not supported "
                    "yet")
        if not isinstance(self.optimizer, HIPSGD):
            return "optimizer is not the fused HIPSGD"
        return self.optimizer.device_lr_blocker()

    def _fall_back(self, reason):
        self._release()
        if isinstance(self.optimizer, HIPSGD):
            self.optimizer.disable_device_lr()
        self._fallback = True
        self.stats["captured"] = False
        self.stats["fallback_reason"] = str(reason)
        if utils.get_rank() == 0:
            logger.info(f"TRAIN.COMPILE_GRAPH: training eagerly ({reason})")

    def _release(self):
        """Drop the graph, then the chunk table it replays."""
        had = self._graph is not None
        self._graph = None
        self._out = None
        self._grads = None
        self._state_refs = None
        self._nbt = []
        if had:
            # the old graph's pool owns these
            for p in self.params:
                p.grad = None
        if isinstance(self.optimizer, HIPSGD):
            self.optimizer.release_capture_tables()

    # -- steps -------------------------------------------------------------
    def _step_body(self, inputs, targets, zero_none):
        outputs = self.net(inputs)
        loss = self.criterion(outputs.float(), targets)
        self.optimizer.zero_grad(set_to_none=zero_none)
        loss.backward()
        self.optimizer.step()
        acc1, acck = utils.accuracy(outputs, targets, topk=(1, self.topk))
        return loss, acc1, acck

    def _eager(self, inputs, targets):
        """The loop body of trainer.train_epoch."""
        from .trainer import _prepare_batch

        inputs, targets = _prepare_batch(inputs, targets, self.device,
                                         self.dtype)
        self.stats["eager_steps"] += 1
        return self._step_body(inputs, targets,
                               utils.get_world_size() == 1)

    def _drained_eager(self, inputs, targets):
        # HIPSGD rewrites its pinned chunk table on the host every eager
        # set_to_none step: the host must not run a step ahead of the device
        # (docs/BENCHMARKING.md, "The warm-up sync")
        out = self._eager(inputs, targets)
        torch.cuda.synchronize()
        return out

    def _capture(self, inputs, targets):
        opt = self.optimizer
        reason = opt.device_lr_blocker()  # strided params show after a step
        if reason is not None:
            raise RuntimeError(reason)
        if self._static is None or self._key != self._batch_key(inputs,
                                                                targets):
            x = torch.empty(inputs.shape, dtype=self.dtype,
                            device=self.device)
            if cfg.TRAIN.CHANNELS_LAST and x.dim() == 4:
                x = x.contiguous(memory_format=torch.channels_last)
            t = torch.empty(targets.shape, dtype=targets.dtype,
                            device=self.device)
            self._static = (x, t)
            self._key = self._batch_key(inputs, targets)
        if self._counter is None:
            self._counter = torch.zeros(1, dtype=torch.int64,
                                        device=self.device)
        x, t = self._static
        opt.sync_device_lr()
        opt.reserve_capture_tables()
        bns = [m for m in self.net.modules()
               if hasattr(m, "_nbt_pending") and m.training]
        pending = [m._nbt_pending for m in bns]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        DF.install_step_counter(self._counter)
        try:
            with torch.cuda.graph(graph):
                loss, acc1, acck = self._step_body(x, t, True)
        finally:
            uses = DF.remove_step_counter()
            # capturing ran forward() but trained nothing
            self._nbt = [(m, m._nbt_pending - n)
                         for m, n in zip(bns, pending)]
            for m, n in zip(bns, pending):
                m._nbt_pending = n
        self._graph = graph
        self._out = (loss.detach(), acc1, acck)
        self._grads = [p.grad for p in self.params]
        # the graph holds raw pointers to momentum and master tensors too:
        # keep them allocated until it is dropped, whatever replaces them
        self._state_refs = [v for p in self.params
                            for v in opt.state[p].values()
                            if torch.is_tensor(v)]
        self._advance_counter = uses > 0
        self._gen = opt.generation
        self.stats["captures"] += 1
        self.stats["captured"] = True

    @staticmethod
    def _batch_key(inputs, targets):
        return (tuple(inputs.shape), inputs.dtype,
                tuple(targets.shape), targets.dtype)

    def _replay(self, inputs, targets):
        x, t = self._static
        # one pass: H2D (if any), dtype cast and channels_last conversion
        x.copy_(inputs, non_blocking=True)
        t.copy_(targets, non_blocking=True)
        for p, g in zip(self.params, self._grads):
            if p.grad is not g:
                # an eager step left its own grad (or none) on the parameter
                p.grad = g
        if self._advance_counter:
            self._counter.add_(1)
        self.optimizer.sync_device_lr()
        for m, n in self._nbt:
            m._nbt_pending += n
        self._graph.replay()
        self.stats["replays"] += 1
        return self._out

    def __call__(self, inputs, targets):
        if self._fallback:
            return self._eager(inputs, targets)
        if self.stats["eager_steps"] < self.warmup:
            if self._side is None:
                self._side = torch.cuda.Stream()
            cur = torch.cuda.current_stream()
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                out = self._drained_eager(inputs, targets)
            cur.wait_stream(self._side)
            return out
        if (self._graph is not None
                and self._gen != self.optimizer.generation):
            # load_state_dict replaced the momentum/master tensors
            self._release()
        if self._graph is None and self._key in (
                None, self._batch_key(inputs, targets)):
            try:
                self._capture(inputs, targets)
            except Exception as exc:  # never fail the run
                for p in self.params:
                    p.grad = None  # whatever the broken capture left behind
                self._fall_back(f"capture failed: {exc!r}")
                return self._eager(inputs, targets)
        if self._graph is None or self._key != self._batch_key(inputs,
                                                               targets):
            return self._drained_eager(inputs, targets)
        return self._replay(inputs, targets)
