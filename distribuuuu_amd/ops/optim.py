"""Fused SGD-momentum optimizer.

One multi-tensor HIP kernel per step consumes a device-resident chunk table
covering every parameter (the reference launches one ATen kernel per tensor —
161 launches for ResNet-50). The table is built once and cached across steps
(no per-step host work; the step is hipGraph-capturable). bf16 parameters
carry fp32 master weights and fp32 momentum so the update math never loses
precision (SURVEY.md §7 hard-part 4).

The kernel addresses grad, param, momentum and master by ONE linear storage
offset, so a parameter only enters the table when all four are dense and laid
out with the parameter's strides. Optimizer state that is not (e.g. loaded
from a checkpoint saved in another memory format) is re-strided once at table
build; a parameter whose GRAD is laid out differently is updated with the
stride-aware tensor math of the fallback instead (with a one-time warning).

Both paths follow torch.optim.SGD semantics (reference utils.py:187-196:
momentum + nesterov + weight decay + dampening), including the first step of
a parameter, which seeds the momentum buffer with the un-dampened gradient.

For a hipGraph-captured step (graph_step.GraphedTrainStep) two things are
opt-in or automatic: device-rate mode reads the learning rate from a float32
device tensor per group (``enable_device_lr`` / ``sync_device_lr``), so a
replayed graph follows the schedule; and a ``step()`` issued while the stream
is capturing builds its chunk table into a pinned/device pair of its own,
which eager steps and ``state_dict()`` never touch.

``HIPLARS`` (at the end of this file) is HIPSGD with a layer-wise trust ratio
on the same table, cache and capture machinery (csrc/lars.hip).
"""

import warnings

import torch
from torch.optim import SGD

from .dispatch import hip_op_available, ext

_CHUNK = 16384
_FLAG_FRESH = 4  # sgd.hip: momentum uninitialised (first step)


def _capturing():
    return (torch.cuda.is_available()
            and torch.cuda.is_current_stream_capturing())


def _layout(t):
    """Strides of the dims that matter (size-1 dims carry arbitrary strides)."""
    return tuple(st for s, st in zip(t.shape, t.stride()) if s != 1)


def _dense(t):
    """Non-overlapping and dense: some dim permutation is contiguous."""
    expect = 1
    for st, s in sorted((st, s) for s, st in zip(t.shape, t.stride())
                        if s != 1):
        if st != expect:
            return False
        expect *= s
    return True


class HIPSGD(SGD):
    """torch.optim.SGD drop-in whose GPU step is one fused multi-tensor kernel."""

    _warned_layout = False

    # class-level defaults: instances unpickled from older checkpoints (and
    # __init__ itself, which torch defines) need no extra set-up
    generation = 0       # bumped whenever state tensors are replaced
    _lr_dev = None       # device-rate mode: one float32[1] tensor per group
    _lr_last = None      # ... and the host value last uploaded into each
    _private = None      # capture-private (pinned, device) table per group

    # the extension ops behind step(); a subclass names its own pair
    _step_op = "sgd_step"
    _dev_op = "sgd_step_dev"
    _fused = True        # False (HIPLARS(fused=False)): tensor ops throughout

    # -- device-rate mode --------------------------------------------------
    def enable_device_lr(self):
        """The fused kernel reads each group's rate from a float32[1] tensor
        on the group's device instead of a launch argument. Call
        sync_device_lr() after changing group["lr"]."""
        self._lr_dev, self._lr_last = [], []
        for group in self.param_groups:
            lr = float(group["lr"])
            self._lr_dev.append(torch.full(
                (1,), lr, dtype=torch.float32,
                device=group["params"][0].device))
            self._lr_last.append(lr)

    def disable_device_lr(self):
        self._lr_dev = self._lr_last = None

    def device_lr_blocker(self):
        """Why the fused step cannot run in device-rate mode (a string), or
        None. Parameters on the stride-aware path are known once a step has
        built the chunk table, so ask again after the first step."""
        if not self._fused or not hip_op_available(self._dev_op):
            return f"fused {self._dev_op} kernel unavailable"
        for group in self.param_groups:
            if not group["params"][0].is_cuda:
                return "parameters are not on the GPU"
            cache = group.get("_hip_table")
            if cache is not None and cache[2]:
                return (f"{len(cache[2])} parameter(s) take the stride-aware "
                        "update outside the fused kernel")
        return None

    def sync_device_lr(self):
        """Upload every group["lr"] that differs from the value last
        uploaded; returns how many were. A host float compare per group
        otherwise."""
        if self._lr_dev is None:
            return 0
        n = 0
        for i, group in enumerate(self.param_groups):
            lr = float(group["lr"])
            if lr != self._lr_last[i]:
                self._lr_dev[i].fill_(lr)
                self._lr_last[i] = lr
                n += 1
        return n

    # -- capture-private chunk table ---------------------------------------
    def reserve_capture_tables(self):
        """Allocate the capture-private table pair of every GPU group ahead
        of the capture (pinned host memory is best not allocated while a
        stream is capturing). Sized like the eager table when a step has
        built one, else for every trainable parameter."""
        if self._private is None:
            self._private = {}
        for gi, group in enumerate(self.param_groups):
            if not group["params"][0].is_cuda:
                continue
            pin = group.get("_hip_table_pin")
            if pin is not None:
                nrec = pin.numel() // 6
            else:
                nrec = sum(-(-p.numel() // _CHUNK) + self._rows_per_tensor
                           for p in group["params"] if p.requires_grad)
            self._private_pair(gi, group, nrec)

    def _private_pair(self, gi, group, nrec):
        pair = self._private.get(gi)
        if pair is None or pair[0].shape[0] != nrec:
            if pair is not None and pair[2]:
                raise RuntimeError(
                    "HIPSGD: a captured graph owns this group's private "
                    "chunk table and the new step needs another size; "
                    "call release_capture_tables() after dropping the graph")
            pin = torch.empty((nrec, 6), dtype=torch.int64, pin_memory=True)
            dev = torch.empty((nrec, 6), dtype=torch.int64,
                              device=group["params"][0].device)
            pair = self._private[gi] = [pin, dev, False]
        return pair

    def release_capture_tables(self):
        """Drop the capture-private tables. Only after the graph that was
        captured with them is gone: it replays the pinned-to-device copy and
        holds raw pointers to both."""
        self._private = None

    def _init_state(self, p):
        """Create momentum (+ master) state; True when it was just created,
        i.e. this is the parameter's first step."""
        state = self.state[p]
        if p.dtype in (torch.bfloat16, torch.float16) \
                and state.get("master") is None:
            state["master"] = p.detach().float().clone()
        if state.get("momentum_buffer") is not None:
            return False
        state["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
        return True

    def _build_table(self, group):
        """Returns (device table, params to update with stride-aware math,
        whether any record carries the first-step flag). While the stream is
        capturing the table goes into the group's capture-private pair and
        the eager pair is left alone."""
        capturing = _capturing()
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        recs = []
        strided = []
        any_fresh = False
        # momentum == 0 never reads the buffer's history: no first-step case
        seed_first = group["dampening"] != 0 and group["momentum"] != 0
        tensors = []  # (first record, records, index in the group, param)
        for pi, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            fresh = self._init_state(p)
            state = self.state[p]
            lay = _layout(p)
            if not _dense(p) or _layout(p.grad) != lay:
                # never hand a permuted grad to the linear-index kernel
                if not HIPSGD._warned_layout:
                    HIPSGD._warned_layout = True
                    warnings.warn(
                        "HIPSGD: a gradient is not laid out like its "
                        f"parameter (param strides {p.stride()}, grad strides "
                        f"{p.grad.stride()}); such parameters are updated "
                        "outside the fused kernel.")
                strided.append((p, fresh))
                continue
            for k in ("momentum_buffer", "master"):
                t = state.get(k)
                if t is not None and _layout(t) != lay:
                    state[k] = torch.empty_like(
                        p, dtype=torch.float32).copy_(t)
            master = state.get("master", p)
            flags = (1 if p.dtype == torch.bfloat16 else 0) | (
                2 if p.grad.dtype == torch.bfloat16 else 0) | (
                self._extra_flags(pi))
            if fresh and seed_first:
                flags |= _FLAG_FRESH
                any_fresh = True
            n = p.numel()
            off = 0
            first = len(recs)
            while off < n:
                cnt = min(_CHUNK, n - off)
                recs.append([p.grad.data_ptr(), p.data_ptr(),
                             state["momentum_buffer"].data_ptr(),
                             master.data_ptr(), off,
                             cnt | (flags << 32)])
                off += _CHUNK
            tensors.append((first, len(recs) - first, pi, p))
        nchunks = len(recs)
        recs += self._tensor_records(tensors)
        device = group["params"][0].device
        # pinned staging + async copy. The pinned buffer and device table are
        # allocated on the FIRST build (outside any hipGraph capture, during
        # warmup); capture-time rebuilds (grad pointers change under
        # zero_grad(set_to_none=True)) only do host writes + one capturable
        # async H2D copy into the existing device tensor.
        cpu = torch.tensor(recs, dtype=torch.int64).reshape(-1, 6)
        if capturing:
            if any_fresh:
                raise RuntimeError(
                    "HIPSGD: a parameter's first step cannot be captured "
                    "(its first-step flag would replay); run one eager step "
                    "before capturing")
            if self._private is None:
                self._private = {}
            pair = self._private_pair(gi, group, cpu.shape[0])
            if pair[2]:
                raise RuntimeError(
                    "HIPSGD: one captured step() per graph; call "
                    "release_capture_tables() after dropping the graph")
            pair[2] = True  # a graph now replays the copy below
            pair[0].copy_(cpu)
            pair[1].copy_(pair[0], non_blocking=True)
            self._table_built(group, pair, nchunks)
            return pair[1], strided, any_fresh
        pin = group.get("_hip_table_pin")
        table = group.get("_hip_table_dev")
        if pin is None or pin.numel() != cpu.numel():
            pin = cpu.pin_memory()
            table = pin.to(device, non_blocking=True)
            group["_hip_table_pin"] = pin
            group["_hip_table_dev"] = table
            ws = self._workspace(group, cpu.shape[0])
            if ws is not None:
                group["_hip_table_ws"] = ws
            # a later captured step needs a pair of this size and must not
            # allocate pinned memory while capturing: set it aside now
            # (allocated, never written here)
            if not (self._private or {}).get(gi, (None, None, False))[2]:
                if self._private is None:
                    self._private = {}
                self._private_pair(gi, group, cpu.shape[0])
        else:
            pin.copy_(cpu)
            table.copy_(pin, non_blocking=True)
        self._table_built(group, None, nchunks)
        return table, strided, any_fresh

    # -- hooks for an optimizer that rides on this table (HIPLARS) ----------
    _rows_per_tensor = 0  # table rows a tensor adds beyond its chunks

    def _extra_flags(self, pi):
        """More bits for a chunk record's flags word; `pi` is the
        parameter's index in its group."""
        return 0

    def _tensor_records(self, tensors):
        """Rows appended after all chunk records."""
        return []

    def _workspace(self, group, nrec):
        """Device scratch that lives and dies with a table pair of `nrec`
        rows, or None."""
        return None

    def _table_built(self, group, pair, nchunks):
        """A table was just written: `pair` is the capture-private pair, or
        None for the group's eager one."""

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        if not self._fused or not hip_op_available(self._step_op):
            return self._fallback_step(loss)

        capturing = _capturing()
        if not capturing:
            self.sync_device_lr()
        for gi, group in enumerate(self.param_groups):
            if not group["params"][0].is_cuda:
                # host-resident model on a GPU machine: tensor ops
                self._fallback_group(group)
                continue
            if capturing:
                # never read or written by eager steps, and the other way round
                table, strided, _ = self._build_table(group)
                if strided:
                    raise RuntimeError(
                        "HIPSGD: parameters on the stride-aware path cannot "
                        "be captured")
                self._launch(gi, group, table)
                continue
            cache = group.get("_hip_table")
            # the grad's strides are part of the key: the kernel's linear
            # indexing is only valid for the layout the table was validated
            # against (a parameter cannot change strides and keep its pointer)
            key = []
            for p in group["params"]:
                g = p.grad  # one attribute read: this loop runs every step
                if g is None:
                    key.append(None)
                else:
                    key += (p.data_ptr(), g.data_ptr(), g.stride())
            if cache is None or cache[1] != key:
                table, strided, any_fresh = self._build_table(group)
                # a table with first-step records is good for one step only
                group["_hip_table"] = (table, None if any_fresh else key,
                                       strided)
            else:
                table, strided = cache[0], cache[2]
            self._launch(gi, group, table)
            if strided:
                self._update_strided(group, strided)
                # first-step status is spent
                group["_hip_table"] = (table, group["_hip_table"][1],
                                       [(p, False) for p, _ in strided])
        return loss

    def _launch(self, gi, group, table):
        if not table.numel():
            return
        # torch ignores dampening when there is no momentum
        damp = group["dampening"] if group["momentum"] != 0 else 0.0
        if self._lr_dev is not None:
            ext().sgd_step_dev(table, self._lr_dev[gi], group["momentum"],
                               damp, group["weight_decay"], group["nesterov"])
        else:
            ext().sgd_step(table, group["lr"], group["momentum"], damp,
                           group["weight_decay"], group["nesterov"])

    def _drop_table_cache(self):
        # the capture-private pair stays: a graph may still replay it, and
        # whoever holds that graph calls release_capture_tables()
        for group in self.param_groups:
            group.pop("_hip_table", None)
            group.pop("_hip_table_pin", None)
            group.pop("_hip_table_dev", None)
            group.pop("_hip_table_ws", None)

    def state_dict(self):
        # drop the pointer cache from serialized state
        self._drop_table_cache()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        # loading replaces momentum/master tensors; the cached device table
        # embeds their raw pointers, so it must be rebuilt on the next step
        super().load_state_dict(state_dict)
        self._drop_table_cache()
        # a captured graph still points at the replaced tensors: its owner
        # compares this counter and captures again
        self.generation += 1
        # the table kernel requires fp32 momentum/master on the param's device
        # (their strides are checked, and fixed, when the table is built).
        # torch casts loaded state to the PARAMETER's dtype, which would round
        # a bf16 parameter's fp32 momentum and master to bf16: take those two
        # from the source dict instead.
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            state = self.state.get(p)
            if not state:
                continue
            src = state_dict["state"].get(i, {})
            for k in ("momentum_buffer", "master"):
                if state.get(k) is None:
                    continue
                t = src.get(k)
                if not torch.is_tensor(t):
                    t = state[k]
                state[k] = t.to(device=p.device, dtype=torch.float32,
                                copy=True)

    def _update_strided(self, group, strided):
        for p, fresh in strided:
            self._update_param(p, group, fresh)

    def _update_param(self, p, group, fresh, q=None):
        """Plain stride-aware SGD math for one parameter, with fp32 master
        handling for bf16 params. `fresh`: first step of this parameter.
        `q`: a 0-dim tensor that scales g + wd*w (HIPLARS), or None."""
        lr = group["lr"]
        mu = group["momentum"]
        damp = group["dampening"]
        wd = group["weight_decay"]
        state = self.state[p]
        low_prec = p.dtype in (torch.bfloat16, torch.float16)
        g = p.grad.float()
        w = state["master"] if low_prec else p.data
        if wd != 0:
            g = g.add(w, alpha=wd)
        if q is not None:
            g = g * q
        if mu != 0:
            buf = state["momentum_buffer"]
            if fresh:
                buf.copy_(g)
            else:
                buf.mul_(mu).add_(g, alpha=1 - damp)
            upd = g.add(buf, alpha=mu) if group["nesterov"] else buf
        else:
            upd = g
        w.add_(upd, alpha=-lr)
        if low_prec:
            p.data.copy_(w.to(p.dtype))

    def _fallback_step(self, loss):
        """Whole step in tensor ops (CPU / extension not built)."""
        for group in self.param_groups:
            self._fallback_group(group)
        return loss

    def _fallback_group(self, group):
        for p in group["params"]:
            if p.grad is None:
                continue
            fresh = self._init_state(p)
            self._update_param(p, group, fresh)


_SLOT_SHIFT = 8  # lars.hip: a chunk's tensor slot sits above the flag bits


class HIPLARS(HIPSGD):
    """HIPSGD with layer-wise adaptive rate scaling (You, Gitman, Ginsburg
    2017). Per parameter tensor, with w the fp32 master and g the gradient:

        W = sum(w*w), G = sum(g*g)
        q = trust_coef * sqrt(W) / (sqrt(G) + wd*sqrt(W) + eps)
            if p.ndim > 1 and W > 0 and G > 0, else 1

    and the SGD-momentum update of HIPSGD runs on q * (g + wd*w). Tensors
    with ndim <= 1 (BN weight and bias, biases) are never adapted.

    The fused step is three launches on the group's chunk table (lars.hip):
    per-chunk squared norms, a per-tensor combine that forms q, the update.
    ``last_trust[gi]`` (float32 [len(params)]) and ``last_sqnorms[gi]``
    (float32 [len(params), 2]: W, G) are device tensors holding what the
    latest step of group ``gi`` computed; a parameter without a grad holds
    q = 1 and zero norms.
    """

    _step_op = "lars_step"
    _dev_op = "lars_step_dev"
    _rows_per_tensor = 1

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0,
                 weight_decay=0, nesterov=False, trust_coef=1e-3, eps=1e-8,
                 fused=True):
        if trust_coef < 0.0:
            raise ValueError(f"Invalid trust_coef value: {trust_coef}")
        if eps < 0.0:
            raise ValueError(f"Invalid eps value: {eps}")
        self._lars_defaults = dict(trust_coef=trust_coef, eps=eps)
        super().__init__(params, lr=lr, momentum=momentum,
                         dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov)
        self.defaults.update(self._lars_defaults)
        self._fused = bool(fused)
        self.last_trust = {}
        self.last_sqnorms = {}

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for k, v in self._lars_defaults.items():
            self.param_groups[-1].setdefault(k, v)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # groups saved by HIPSGD or torch.optim.SGD carry neither key
        for group in self.param_groups:
            for k, v in self._lars_defaults.items():
                group.setdefault(k, v)

    # -- table ---------------------------------------------------------------
    def _extra_flags(self, pi):
        return pi << _SLOT_SHIFT

    def _tensor_records(self, tensors):
        return [[first, n, pi, 1 if p.ndim > 1 else 0, 0, 0]
                for first, n, pi, p in tensors]

    def _workspace(self, group, nrec):
        n = len(group["params"])
        device = group["params"][0].device
        return {"part": torch.empty(2 * nrec, dtype=torch.float32,
                                    device=device),
                "sqnorm": torch.zeros((n, 2), dtype=torch.float32,
                                      device=device),
                "q": torch.ones(n, dtype=torch.float32, device=device),
                "nchunks": 0}

    def _private_pair(self, gi, group, nrec):
        pair = super()._private_pair(gi, group, nrec)
        if len(pair) == 3:
            pair.append(self._workspace(group, nrec))
        return pair

    def _table_built(self, group, pair, nchunks):
        ws = pair[3] if pair is not None else group["_hip_table_ws"]
        ws["nchunks"] = nchunks
        # the kernels write the slots of tensors in the table; the others
        # (no grad, or on the stride-aware path until its update) read so
        ws["q"].fill_(1.0)
        ws["sqnorm"].zero_()

    def _launch(self, gi, group, table):
        pair = (self._private or {}).get(gi)
        private = pair is not None and table is pair[1]
        ws = pair[3] if private else group["_hip_table_ws"]
        if table.numel():
            damp = group["dampening"] if group["momentum"] != 0 else 0.0
            args = (group["momentum"], damp, group["weight_decay"],
                    group["nesterov"], group["trust_coef"], group["eps"])
            head = (table, ws["nchunks"], ws["part"], ws["sqnorm"], ws["q"])
            if self._lr_dev is not None:
                ext().lars_step_dev(*head, self._lr_dev[gi], *args)
            else:
                ext().lars_step(*head, group["lr"], *args)
        if not private and pair is not None and pair[2]:
            # a graph owns the private copy and its replays write there:
            # that copy is the one to read, so an eager step in between
            # (a batch of another shape) leaves its figures in it too
            for k in ("q", "sqnorm"):
                pair[3][k].copy_(ws[k])
            ws = pair[3]
        self.last_trust[gi] = ws["q"]
        self.last_sqnorms[gi] = ws["sqnorm"]

    # -- tensor-op path ------------------------------------------------------
    def _trust(self, p, group, sqnorm):
        """Writes (W, G) into `sqnorm` ([2]); returns q as a 0-dim tensor,
        or None for a tensor that is not adapted. No host sync."""
        state = self.state[p]
        w = state["master"] if state.get("master") is not None else p.data
        g = p.grad.float()
        w2 = (w.float() * w.float()).sum()
        g2 = (g * g).sum()
        sqnorm[0] = w2
        sqnorm[1] = g2
        if p.ndim <= 1:
            return None
        nw, ng = w2.sqrt(), g2.sqrt()
        q = group["trust_coef"] * nw / (
            ng + group["weight_decay"] * nw + group["eps"])
        return torch.where((w2 > 0) & (g2 > 0), q, torch.ones_like(q))

    def _update_strided(self, group, strided):
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        index = {id(p): i for i, p in enumerate(group["params"])}
        for p, fresh in strided:
            pi = index[id(p)]
            q = self._trust(p, group, self.last_sqnorms[gi][pi])
            if q is not None:
                self.last_trust[gi][pi] = q
            self._update_param(p, group, fresh, q)

    def _fallback_group(self, group):
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        n = len(group["params"])
        device = group["params"][0].device
        trust = torch.ones(n, dtype=torch.float32, device=device)
        sqnorms = torch.zeros((n, 2), dtype=torch.float32, device=device)
        for pi, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            fresh = self._init_state(p)
            q = self._trust(p, group, sqnorms[pi])
            if q is not None:
                trust[pi] = q
            self._update_param(p, group, fresh, q)
        self.last_trust[gi] = trust
        self.last_sqnorms[gi] = sqnorms
