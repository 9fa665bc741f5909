"""Concat-free dense blocks: one NHWC slab per block (csrc/dense_bn.hip).

``DenseSlab`` holds a block's features in one ``[N, Ctot, H, W]``
channels_last buffer. ``append`` writes a layer's new channels behind the
ones already there and forms their BN sum / sum-of-squares in the same pass;
``bn_relu`` runs a layer's norm1 on the channel prefix straight from those
sums; ``output`` hands the slab itself on as the block's output.

Backward (the ``_Fork`` protocol of functional.py): the gradient of the
block's output IS the gradient slab. Each append's backward takes its own
slice out densely (for conv2's backward) and passes the channel prefix on;
each norm1's backward adds its input gradient into that prefix in place and
returns the same buffer, and the fork node of that slab version sees two
gradients with one address and skips the add. Data dependencies order it: a
layer's slice is taken only after every later layer has accumulated.
"""

import os

import torch

from .dispatch import ext
from .functional import _Fork, _cl

_PACK = {torch.bfloat16: 8, torch.float32: 4}


def slab_enabled():
    return os.environ.get("DISTRIBUUUU_DENSE_SLAB", "1") != "0"


def slab_shape_ok(x, c0, growth):
    """dtype / width gate of the slab kernels: 16-byte channel packs at
    every channel offset. Meta tensors stand in for GPU ones in shape-only
    checks; the caller still asks use_hip() before taking the route."""
    pack = _PACK.get(x.dtype)
    return (pack is not None and x.dim() == 4
            and x.device.type in ("cuda", "meta")
            and c0 % pack == 0 and growth % pack == 0)


def _prefix(buf, c):
    """buf[:, :c] as a tensor of its own on buf's storage. Not an autograd
    view: the slab is written after handles to it were handed out, and a
    gradient prefix must keep its address through the fork."""
    n, ctot, h, w = buf.shape
    return buf.new_empty(0).set_(buf.untyped_storage(), buf.storage_offset(),
                                 (n, c, h, w), (h * w * ctot, 1, w * ctot,
                                                ctot))


class _SlabAppend(torch.autograd.Function):
    """handle' = append(handle, y). Backward: grad(handle') is a gradient
    slab ``c_off + g`` channels wide - dense as it arrives for the block's
    output, else the prefix handed on by the append after this one."""

    @staticmethod
    def forward(ctx, prev, y, st, slot):
        y = _cl(y)
        ctx.st, ctx.slot = st, slot
        ctx.c_off, ctx.g = st.c, y.shape[1]
        ext().dense_append(st.slab, y, st.c, st.sums)
        st.c += y.shape[1]
        return _prefix(st.slab, st.c)

    @staticmethod
    def backward(ctx, gh):
        st, c_off, g = ctx.st, ctx.c_off, ctx.g
        gs = st.gslab
        if not (gs is not None and gh.data_ptr() == gs.data_ptr()
                and gs.shape[1] >= c_off + g):
            # the block's output gradient, or a prefix that autograd had to
            # re-materialise: any dense NHWC tensor serves as gradient slab
            gs = _cl(gh)
        gy = (ext().dense_take(gs, c_off, g) if ctx.needs_input_grad[1]
              else None)
        if c_off == 0:
            st.gslab = None  # consumed: a later backward starts afresh
            return None, gy, None, None
        st.gslab = gs
        gprev = _prefix(gs, c_off)
        if ctx.slot is not None:
            ctx.slot["g"] = (gs, gprev)
        return gprev, gy, None, None


class _SlabBNReLU(torch.autograd.Function):
    """relu(bn(slab[:, :cin])) as a dense tensor. The slab is kept on ctx,
    not in save_for_backward: channels behind cin are written after this
    node saved it."""

    @staticmethod
    def forward(ctx, handle, weight, bias, running_mean, running_var,
                momentum, eps, training, st, slot):
        cin = handle.shape[1]
        gamma = weight.float().contiguous()
        beta = bias.float().contiguous()
        rm, rv = running_mean, running_var
        copy_back = rm is not None and rm.dtype != torch.float32
        if copy_back:
            rm, rv = rm.float(), rv.float()
        y, mean, rstd, scale, shift = ext().dense_bn_fwd(
            st.slab, cin, st.sums if training else None, gamma, beta, rm, rv,
            momentum, eps, training)
        if copy_back and training:
            running_mean.copy_(rm)
            running_var.copy_(rv)
        ctx.save_for_backward(weight, mean, rstd, scale, shift)
        ctx.st, ctx.slot, ctx.cin, ctx.training = st, slot, cin, training
        return y

    @staticmethod
    def backward(ctx, gy):
        weight, mean, rstd, scale, shift = ctx.saved_tensors
        st, cin = ctx.st, ctx.cin
        dep = ctx.slot.pop("g", None) if ctx.slot is not None else None
        if dep is not None:
            gs, gx = dep
        elif ctx.needs_input_grad[0]:
            # no prefix was deposited: accumulate into zeros, the fork adds
            n, _, h, w = st.slab.shape
            gs = gx = torch.zeros((n, cin, h, w), dtype=gy.dtype,
                                  device=gy.device,
                                  memory_format=torch.channels_last)
        else:
            gs = gx = None
        gw, gb, _ = ext().dense_bn_bwd(
            _cl(gy), st.slab, cin, gs, mean, rstd,
            weight.float().contiguous(), scale, shift, ctx.training)
        return (gx, gw.to(weight.dtype), gb.to(weight.dtype), None, None,
                None, None, None, None, None)


class DenseSlab:
    """One dense block's feature slab, its BN sums and, during backward, its
    gradient slab. ``stats``: form sum / sumsq on append (training)."""

    def __init__(self, x, ctot, stats):
        n, _, h, w = x.shape
        self.slab = torch.empty((n, ctot, h, w), dtype=x.dtype,
                                device=x.device,
                                memory_format=torch.channels_last)
        self.sums = (torch.empty((2, ctot), dtype=torch.float32,
                                 device=x.device) if stats else None)
        self.c = 0
        self.gslab = None
        self._handle = None
        self._slot = None
        self.append(x)

    def append(self, y):
        self._handle = _SlabAppend.apply(self._handle, y, self, self._slot)
        self._slot = None

    def bn_relu(self, norm):
        """norm(current features) for a plain BatchNorm2d with act relu."""
        h = self._handle
        slot = None
        if torch.is_grad_enabled() and h.requires_grad:
            # this slab version has two consumers: norm and the next append
            h, self._handle = _Fork.apply(h)
            slot = self._slot = {}
        if norm.training:
            norm._nbt_pending += 1
        return _SlabBNReLU.apply(h, norm.weight, norm.bias, norm.running_mean,
                                 norm.running_var, norm.momentum, norm.eps,
                                 norm.training, self, slot)

    def output(self):
        assert self.c == self.slab.shape[1], "dense slab is not full"
        out, self._handle = self._handle, None
        if self.sums is not None:
            # [nblocks=1, 2C] sum/sumsq partials: the consuming BatchNorm
            # (transition norm, norm5) skips its stats pass
            out._bn_partials = self.sums.view(1, -1)
        return out
