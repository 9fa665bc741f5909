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
"""

import warnings

import torch
from torch.optim import SGD

from .dispatch import hip_op_available, ext

_CHUNK = 16384
_FLAG_FRESH = 4  # sgd.hip: momentum uninitialised (first step)


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
        whether any record carries the first-step flag)."""
        recs = []
        strided = []
        any_fresh = False
        # momentum == 0 never reads the buffer's history: no first-step case
        seed_first = group["dampening"] != 0 and group["momentum"] != 0
        for p in group["params"]:
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
                2 if p.grad.dtype == torch.bfloat16 else 0)
            if fresh and seed_first:
                flags |= _FLAG_FRESH
                any_fresh = True
            n = p.numel()
            off = 0
            while off < n:
                cnt = min(_CHUNK, n - off)
                recs.append([p.grad.data_ptr(), p.data_ptr(),
                             state["momentum_buffer"].data_ptr(),
                             master.data_ptr(), off,
                             cnt | (flags << 32)])
                off += _CHUNK
        device = group["params"][0].device
        # pinned staging + async copy. The pinned buffer and device table are
        # allocated on the FIRST build (outside any hipGraph capture, during
        # warmup); capture-time rebuilds (grad pointers change under
        # zero_grad(set_to_none=True)) only do host writes + one capturable
        # async H2D copy into the existing device tensor.
        cpu = torch.tensor(recs, dtype=torch.int64).reshape(-1, 6)
        pin = group.get("_hip_table_pin")
        table = group.get("_hip_table_dev")
        if pin is None or pin.numel() != cpu.numel():
            pin = cpu.pin_memory()
            table = pin.to(device, non_blocking=True)
            group["_hip_table_pin"] = pin
            group["_hip_table_dev"] = table
        else:
            pin.copy_(cpu)
            table.copy_(pin, non_blocking=True)
        return table, strided, any_fresh

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        if not hip_op_available("sgd_step"):
            return self._fallback_step(loss)

        for group in self.param_groups:
            if not group["params"][0].is_cuda:
                # host-resident model on a GPU machine: tensor ops
                self._fallback_group(group)
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
            if table.numel():
                # torch ignores dampening when there is no momentum
                damp = group["dampening"] if group["momentum"] != 0 else 0.0
                ext().sgd_step(table, group["lr"], group["momentum"],
                               damp, group["weight_decay"],
                               group["nesterov"])
            if strided:
                for p, fresh in strided:
                    self._update_param(p, group, fresh)
                # first-step status is spent
                group["_hip_table"] = (table, group["_hip_table"][1],
                                       [(p, False) for p, _ in strided])
        return loss

    def _drop_table_cache(self):
        for group in self.param_groups:
            group.pop("_hip_table", None)
            group.pop("_hip_table_pin", None)
            group.pop("_hip_table_dev", None)

    def state_dict(self):
        # drop the pointer cache from serialized state
        self._drop_table_cache()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        # loading replaces momentum/master tensors; the cached device table
        # embeds their raw pointers, so it must be rebuilt on the next step
        super().load_state_dict(state_dict)
        self._drop_table_cache()
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

    def _update_param(self, p, group, fresh):
        """Plain stride-aware SGD math for one parameter, with fp32 master
        handling for bf16 params. `fresh`: first step of this parameter."""
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
