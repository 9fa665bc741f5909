"""Functional op layer: CPU = plain ATen composition (autograd handles backward);
GPU = custom autograd.Functions over the gfx950 HIP kernels.

Kernel inventory mirrors SURVEY.md §2b (K1-K20). All GPU compute tensors are
NHWC (PyTorch ``channels_last``): logical NCHW with [N,H,W,C] physical layout,
weights [K,C,R,S] logical → [K,R,S,C] physical.
"""

import os

import torch
import torch.nn.functional as F

from .dispatch import ext, fallback_warn, use_hip

_ACTS = {"none": 0, "relu": 1, "silu": 2, "sigmoid": 3}

_WGRAD_STREAM = None


def _wgrad_stream():
    """Side HIP stream for weight-gradient kernels. dgrad and wgrad of a
    conv are independent consumers of the same gy; both kernel families are
    latency- (not bandwidth-) bound on MI355X (profiles/wgrad_pmc_r2.md), so
    co-residency on two streams fills each other's stall slots. Ordering is
    by stream events (wait_stream both ways), which hipGraph capture turns
    into graph edges, and the join happens before backward returns — so
    DDP's reducer (which orders against the autograd stream) stays correct
    at any world size. Env DISTRIBUUUU_WGRAD_STREAM=0 disables."""
    global _WGRAD_STREAM
    if _WGRAD_STREAM is None:
        if os.environ.get("DISTRIBUUUU_WGRAD_STREAM", "1") == "0":
            _WGRAD_STREAM = False
        else:
            _WGRAD_STREAM = torch.cuda.Stream()
    return _WGRAD_STREAM


def _cl(x):
    """Ensure channels_last physical layout for 4-D GPU tensors."""
    if x.dim() == 4:
        return x.contiguous(memory_format=torch.channels_last)
    return x.contiguous()


# ---------------------------------------------------------------------------
# Convolution (K1-K5): implicit-GEMM MFMA kernels on GPU
# ---------------------------------------------------------------------------
def _pad8(n):
    return (n + 7) // 8 * 8


def _pad_k(w, k8):
    """Zero-pad output channels (dim 0) of a channels_last weight."""
    k, c, r, s = w.shape
    wp = w.new_zeros((k8, c, r, s)).contiguous(
        memory_format=torch.channels_last)
    wp[:k] = w
    return wp


def _conv_wgrad(e, gyp, x, w, stride, padding, dilation, groups, cin, kout,
                cpad, kpad):
    xw = e.pad_channels(x, _pad8(cin)) if cpad else x
    gw = e.conv2d_wgrad(gyp, xw, w.shape[2], w.shape[3], stride[0], stride[1],
                        padding[0], padding[1], dilation[0], dilation[1],
                        groups)
    if kpad:
        gw = gw[:kout]
    if cpad:
        gw = gw[:, :cin]
    if kpad or cpad:
        gw = _cl(gw)
    return gw


class _HIPConv2d(torch.autograd.Function):
    """groups==1 convs whose C or K is not a multiple of 8 (stem C=3, SE
    squeeze widths like 58) run on zero-padded channels — padding C cannot
    change the output, and padded-K rows are sliced off. Without this, such
    shapes fell back to ATen/MIOpen naive kernels (~230 us per tiny SE conv
    on RegNetY).

    ``emit_part``: the conv's epilogue also emits BN sum/sumsq partials
    (F1 of docs/DESIGN_bn_conv_fusion.md), returned as a non-differentiable
    second output — the consuming BatchNorm skips its whole stats pass over
    y. Enabled lazily: batch_norm_act flags the producing conv's weight the
    first time it sees its output (see conv2d/batch_norm_act below)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, dilation, groups, emit_part,
                fork_slot):
        x = _cl(x)
        w = _cl(w)
        e = ext()
        cin = x.shape[1]
        kout = w.shape[0]
        cpad = groups == 1 and cin % 8 != 0
        kpad = groups == 1 and kout % 8 != 0
        xp, wp = x, w
        if cpad:
            xp = e.pad_channels(x, _pad8(cin))
            wp = e.pad_channels(w, _pad8(cin))
        if kpad:
            wp = _pad_k(wp, _pad8(kout))
        if emit_part and not kpad and bias is None:
            y, part = e.conv2d_fwd_bn(xp, wp, stride[0], stride[1],
                                      padding[0], padding[1], dilation[0],
                                      dilation[1], groups)
        else:
            y = e.conv2d_fwd(xp, wp, stride[0], stride[1], padding[0],
                             padding[1], dilation[0], dilation[1], groups)
            part = y.new_empty(0)
        if kpad:
            y = _cl(y[:, :kout])
        if bias is not None:
            y = y + bias.reshape(1, -1, 1, 1)
        wt_pre = wt_kind = wt_ev = None
        if (torch.is_grad_enabled() and x.requires_grad and not cpad
                and not kpad):
            ts = _wgrad_stream()
            if ts is not False:
                # precompute the dgrad weight transform (flipT / span-flip)
                # on the side stream NOW, overlapping forward compute —
                # backward's critical path skips those kernels entirely
                cur = torch.cuda.current_stream()
                ts.wait_stream(cur)
                with torch.cuda.stream(ts):
                    wt_pre, wt_kind = e.conv2d_dgrad_prep(
                        w, kout, stride[0], stride[1], padding[0],
                        padding[1], dilation[0], dilation[1], groups)
                wt_ev = torch.cuda.Event()
                wt_ev.record(ts)
        ctx.wt_pre = (wt_pre, wt_kind, wt_ev)
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, padding, dilation, groups, bias is not None, cin,
                    kout, cpad, kpad)
        ctx.fork_slot = fork_slot
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    def backward(ctx, gy, _gpart):
        x, w = ctx.saved_tensors
        (stride, padding, dilation, groups, has_bias, cin, kout, cpad,
         kpad) = ctx.conf
        gy = _cl(gy)
        e = ext()
        gx = gw = gb = None
        gyp = e.pad_channels(gy, _pad8(kout)) if kpad else gy
        side = _wgrad_stream() if ctx.needs_input_grad[1] else False
        if side is not False:
            # launch wgrad on the side stream FIRST so it co-runs with the
            # dgrad enqueued on the main stream below (both are
            # latency-bound; see _wgrad_stream)
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                gw = _conv_wgrad(e, gyp, x, w, stride, padding, dilation,
                                 groups, cin, kout, cpad, kpad)
        if ctx.needs_input_grad[0]:
            wd = e.pad_channels(w, _pad8(cin)) if cpad else w
            if kpad:
                wd = _pad_k(wd, _pad8(kout))
            pre, pkind, pev = ctx.wt_pre
            if pre is not None:
                torch.cuda.current_stream().wait_event(pev)
                if not torch.cuda.is_current_stream_capturing():
                    pre.record_stream(torch.cuda.current_stream())
            fslot = ctx.fork_slot
            fbuf = fslot.get("g") if fslot is not None else None
            geom = (gyp, wd, x.shape[2], x.shape[3], stride[0], stride[1],
                    padding[0], padding[1], dilation[0], dilation[1], groups)
            if fbuf is not None and not cpad and fbuf.dtype == gyp.dtype:
                # residual fork (see _Fork): the other branch's gradient is
                # already in fbuf — accumulate this dgrad into it inside the
                # epilogue (one extra read stream) instead of letting
                # autograd run a separate whole-tensor add
                gx, acc_done = e.conv2d_dgrad_acc(
                    *geom, fbuf, pre, pkind if pre is not None else -1)
            elif pre is not None:
                gx = e.conv2d_dgrad(*geom, pre, pkind)
            else:
                gx = e.conv2d_dgrad(*geom)
            if cpad:
                gx = _cl(gx[:, :cin])
            if fslot is not None and fbuf is None:
                fslot["g"] = gx
        if side is not False:
            main.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                gw.record_stream(main)
                gyp.record_stream(side)
                x.record_stream(side)
        elif ctx.needs_input_grad[1]:
            gw = _conv_wgrad(e, gyp, x, w, stride, padding, dilation, groups,
                             cin, kout, cpad, kpad)
        if has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None, None, None, None, None


class _HIPDepthwiseConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padding):
        x = _cl(x)
        w = _cl(w)
        y = ext().dwconv_fwd(x, w, stride[0], stride[1], padding[0], padding[1])
        if bias is not None:
            y = y + bias.reshape(1, -1, 1, 1)
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, padding, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, has_bias = ctx.conf
        gy = _cl(gy)
        e = ext()
        gx = gw = gb = None
        side = _wgrad_stream() if ctx.needs_input_grad[1] else False
        if side is not False:
            # co-run the depthwise wgrad with the dgrad (see _wgrad_stream)
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                gw = e.dwconv_wgrad(gy, x, w.shape[2], w.shape[3], stride[0],
                                    stride[1], padding[0], padding[1])
        if ctx.needs_input_grad[0]:
            gx = e.dwconv_dgrad(gy, w, x.shape[2], x.shape[3], stride[0],
                                stride[1], padding[0], padding[1])
        if side is not False:
            main.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                gw.record_stream(main)
                gy.record_stream(side)
                x.record_stream(side)
        elif ctx.needs_input_grad[1]:
            gw = e.dwconv_wgrad(gy, x, w.shape[2], w.shape[3], stride[0],
                                stride[1], padding[0], padding[1])
        if has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None


def _is_depthwise(x, weight, groups, dilation):
    return (groups > 1 and groups == x.shape[1] and weight.shape[0] == groups
            and weight.shape[1] == 1 and dilation == (1, 1)
            and x.shape[1] % 8 == 0)


def _hip_conv_ok(x, weight, groups):
    if x.dtype not in (torch.bfloat16, torch.float32):
        fallback_warn("conv2d", f"dtype {x.dtype} (bf16/fp32 MFMA kernels)")
        return False
    if groups == 1:
        return True  # any C/K: the pad-channels path covers %8 misfits
    cg = weight.shape[1]
    kg = weight.shape[0] // groups
    if cg % 8 != 0 or kg % 8 != 0:
        fallback_warn("conv2d",
                      f"grouped conv width C/g={cg} K/g={kg} not %8")
        return False  # odd group widths: dedicated kernels pending
    return True


def _pack_narrow_groups(weight, groups, f):
    """Block-diagonal packing for sub-8-wide groups (ResNeXt-50's 4-channel
    stage-1 groups): f neighbouring groups of width cg merge into one compute
    group of width f*cg with zeros off the diagonal, putting the conv on the
    MFMA path at f x the MACs (still far ahead of a naive fallback).
    Differentiable: autograd routes the packed grads back to the original
    weight and discards the zero blocks' grads (docs/DESIGN_grouped_conv.md)."""
    kt, cg, r, s = weight.shape
    kg = kt // groups
    w6 = weight.reshape(groups // f, f, kg, cg, r, s)
    z = weight.new_zeros(groups // f, 1, kg, cg, r, s)
    rows = []
    for i in range(f):
        blocks = [w6[:, i:i + 1] if j == i else z for j in range(f)]
        rows.append(torch.cat(blocks, dim=3))
    return torch.cat(rows, dim=1).reshape(kt, f * cg, r, s)


def conv2d(x, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
           groups=1):
    stride, padding, dilation = tuple(stride), tuple(padding), tuple(dilation)
    if (x.dtype == torch.bfloat16 and _is_depthwise(x, weight, groups, dilation)
            and use_hip(x, "dwconv_fwd")):
        return _HIPDepthwiseConv2d.apply(x, weight, bias, stride, padding)
    if (x.is_cuda and groups > 1 and weight.shape[1] < 8
            and 8 % weight.shape[1] == 0
            and x.dtype in (torch.bfloat16, torch.float32)):
        f = 8 // weight.shape[1]
        kg = weight.shape[0] // groups
        if groups % f == 0 and (kg * f) % 8 == 0 and use_hip(x, "conv2d_fwd"):
            wp = _pack_narrow_groups(_cl(weight), groups, f)
            return conv2d(x, wp, bias, stride, padding, dilation, groups // f)
    if use_hip(x, "conv2d_fwd") and _hip_conv_ok(x, weight, groups):
        emit = (bias is None and torch.is_grad_enabled()
                and getattr(weight, "_emit_bn_partials", False))
        fslot = (getattr(x, "_fork_slot", None)
                 if torch.is_grad_enabled() else None)
        y, part = _HIPConv2d.apply(x, weight, bias, stride, padding, dilation,
                                   groups, emit, fslot)
        if part.numel():
            y._bn_partials = part
        elif bias is None:
            # discovery hook: if a BatchNorm consumes this output it flags the
            # weight, and from the next step on the epilogue emits partials
            y._bn_src_weight = weight
        return y
    return F.conv2d(x, weight, bias, stride, padding, dilation, groups)


# ---------------------------------------------------------------------------
# BatchNorm (+residual add + activation) — K6/K8/K20 fused
# ---------------------------------------------------------------------------
class _HIPBatchNormAct(torch.autograd.Function):
    """Training-mode fused BN. Stats (from conv-epilogue partials when
    available — F1) are computed in the batch_norm_act wrapper; this Function
    covers normalize(+add)(+act) forward and the backward chain, with the act
    mask recomputed from x (F3a — the y stream is never re-read), or read
    from the bitmask the residual-relu apply emitted."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean, rstd, scale, shift, training,
                act_id, residual, fork_slot):
        e = ext()
        res = _cl(residual) if residual is not None else None
        mask = None
        if (res is not None and act_id == 1 and training
                and torch.is_grad_enabled()
                and os.environ.get("DISTRIBUUUU_BN_MASK", "1") != "0"):
            # emit the act' bitmask (1 bit/elem): backward then skips the
            # res stream and the z recompute on the big residual BNs
            y, mask = e.bn_apply_act_mask(x, scale, shift, act_id, res)
        else:
            y = e.bn_apply_act(x, scale, shift, act_id, res)
        ctx.save_for_backward(x, weight, scale, shift, mean, rstd,
                              res if res is not None else x.new_empty(0),
                              mask if mask is not None else x.new_empty(0))
        ctx.act_id = act_id
        ctx.training = training
        ctx.has_res = residual is not None
        ctx.fork_slot = fork_slot
        return y

    @staticmethod
    def backward(ctx, gy):
        (x, weight, scale, shift, mean, rstd, res,
         mask) = ctx.saved_tensors
        if mask.numel() == 0:
            mask = None
        e = ext()
        gy = _cl(gy)
        gamma = weight.float().contiguous()
        gx, gw, gb, gres = e.bn_bwd(
            gy, x, res if ctx.has_res else None, mean, rstd, gamma,
            scale, shift, ctx.act_id, ctx.training, ctx.has_res,
            mask=mask)
        if (ctx.has_res and ctx.fork_slot is not None
                and "g" not in ctx.fork_slot):
            # the shortcut branch of a residual fork: deposit gres so the
            # main branch's final dgrad can accumulate into it (see _Fork)
            ctx.fork_slot["g"] = gres
        return (gx, gw.to(weight.dtype), gb.to(weight.dtype), None, None,
                None, None, None, None, gres if ctx.has_res else None, None)


def _bn_stats_half(x, weight, bias, running_mean, running_var, training,
                   momentum, eps):
    """Stats half of a HIP BatchNorm: conv-epilogue partials (F1) when the
    producing conv emitted them, running-stat update, and the fused
    scale/shift coefficients. Returns (x_cl, mean, rstd, scale, shift)."""
    part = getattr(x, "_bn_partials", None) if training else None
    if training and part is None:
        srcw = getattr(x, "_bn_src_weight", None)
        if srcw is not None:
            # flag the producing conv: it emits partials from now on
            srcw._emit_bn_partials = True
    e = ext()
    x = _cl(x)
    rm, rv = running_mean, running_var
    with torch.no_grad():
        gamma = weight.float().contiguous()
        beta = bias.float().contiguous()
        copy_back = False
        if rm is not None and rm.dtype != torch.float32:
            rm, rv = rm.float(), rv.float()
            copy_back = True
        mean, rstd, scale, shift = e.bn_stats(
            x, gamma, beta, rm, rv, momentum, eps, training, part)
        if copy_back:
            running_mean.copy_(rm)
            running_var.copy_(rv)
    return x, mean, rstd, scale, shift


def batch_norm_act(x, weight, bias, running_mean, running_var, training=False,
                   momentum=0.1, eps=1e-5, act="none", residual=None):
    if use_hip(x, "bn_sums"):
        act_id = _ACTS[act]
        x, mean, rstd, scale, shift = _bn_stats_half(
            x, weight, bias, running_mean, running_var, training, momentum,
            eps)
        res_fslot = (getattr(residual, "_fork_slot", None)
                     if residual is not None and torch.is_grad_enabled()
                     else None)
        return _HIPBatchNormAct.apply(x, weight, bias, mean, rstd, scale,
                                      shift, training, act_id, residual,
                                      res_fslot)
    y = F.batch_norm(x, running_mean, running_var, weight, bias, training,
                     momentum, eps)
    if residual is not None:
        y = y + residual
    return _apply_act(y, act)


def _bn_fuse_on(part):
    # DISTRIBUUUU_BN_FUSE: unset/1 = both fused paths, 0 = neither (the tests
    # compare both ways bit for bit), "stem" / "shortcut" = that one alone
    # (A/B measurements)
    v = os.environ.get("DISTRIBUUUU_BN_FUSE", "1")
    return v == part or v not in ("0", "stem", "shortcut")


def _pack_ok(x):
    """dtype/channel gate of the packed BN kernels (16-byte channel packs)."""
    if x.dtype == torch.bfloat16:
        return x.shape[1] % 8 == 0
    return x.dtype == torch.float32 and x.shape[1] % 4 == 0


class _HIPBatchNormActMaxPool(torch.autograd.Function):
    """BN(+relu) -> maxpool(3, 2, 1) of the stem as one forward kernel and a
    reduce/dx backward pair that gathers g from the pooled gradient: neither
    the full-size BN output nor the full-size pooled-gradient tensor exists.
    Bit-identical to batch_norm_act -> max_pool2d."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean, rstd, scale, shift, training,
                act_id):
        y, idx = ext().bn_act_maxpool_fwd(x, scale, shift, act_id)
        ctx.save_for_backward(x, weight, scale, shift, mean, rstd, idx)
        ctx.act_id = act_id
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, scale, shift, mean, rstd, idx = ctx.saved_tensors
        gamma = weight.float().contiguous()
        gx, gw, gb = ext().bn_pool_bwd(_cl(gy), idx, x, mean, rstd, gamma,
                                       scale, shift, ctx.act_id, ctx.training)
        return (gx, gw.to(weight.dtype), gb.to(weight.dtype), None, None,
                None, None, None, None)


def batch_norm_act_maxpool(x, weight, bias, running_mean, running_var,
                           training=False, momentum=0.1, eps=1e-5, act="none",
                           kernel_size=3, stride=2, padding=1):
    """max_pool2d(batch_norm_act(x, ...)) — fused on the HIP path for the
    (3, 2, 1) pool with act none/relu, today's two calls everywhere else."""
    if (x.is_cuda and x.dim() == 4 and act in ("none", "relu")
            and (kernel_size, stride, padding) == (3, 2, 1) and _pack_ok(x)
            # one grid row per pooled output row
            and x.shape[0] * ((x.shape[2] - 1) // 2 + 1) <= 65535
            and _bn_fuse_on("stem") and use_hip(x, "bn_act_maxpool_fwd")):
        x, mean, rstd, scale, shift = _bn_stats_half(
            x, weight, bias, running_mean, running_var, training, momentum,
            eps)
        return _HIPBatchNormActMaxPool.apply(x, weight, bias, mean, rstd,
                                             scale, shift, training,
                                             _ACTS[act])
    y = batch_norm_act(x, weight, bias, running_mean, running_var, training,
                       momentum, eps, act)
    return max_pool2d(y, kernel_size, stride, padding)


class _HIPBatchNormActDual(torch.autograd.Function):
    """Residual-join BN of a downsample block with the shortcut BN applied in
    the same pass: y = relu(bn(x) + bn_s(xr)), xr the RAW shortcut-conv
    output. The identity tensor is never materialised. Backward is today's
    chain on the same values: masked bn_bwd for the join BN, then
    bn_bwd(act none) for the shortcut BN on the resulting gres."""

    @staticmethod
    def forward(ctx, x, weight, bias, xr, rweight, rbias, mean, rstd, scale,
                shift, rmean, rrstd, rscale, rshift):
        y, mask = ext().bn_apply_act_mask(x, scale, shift, 1, xr, rscale,
                                          rshift)
        ctx.save_for_backward(x, weight, scale, shift, mean, rstd, xr,
                              rweight, rscale, rshift, rmean, rrstd, mask)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x, weight, scale, shift, mean, rstd, xr, rweight, rscale, rshift,
         rmean, rrstd, mask) = ctx.saved_tensors
        e = ext()
        # the masked kernels never read the residual stream; xr only fills
        # the pointer slot
        gx, gw, gb, gres = e.bn_bwd(
            _cl(gy), x, xr, mean, rstd, weight.float().contiguous(), scale,
            shift, 1, True, True, mask=mask)
        gxr, grw, grb, _ = e.bn_bwd(
            gres, xr, None, rmean, rrstd, rweight.float().contiguous(),
            rscale, rshift, 0, True, False, mask=None)
        return (gx, gw.to(weight.dtype), gb.to(weight.dtype), gxr,
                grw.to(rweight.dtype), grb.to(rweight.dtype), None, None,
                None, None, None, None, None, None)


def dual_bn_ok(x):
    """Whether the join BN of a downsample block can apply the shortcut BN
    itself: exactly the conditions of the relu bitmask path (training-mode
    module checks are the caller's)."""
    return (x.is_cuda and torch.is_grad_enabled() and _pack_ok(x)
            and os.environ.get("DISTRIBUUUU_BN_MASK", "1") != "0"
            and _bn_fuse_on("shortcut")
            and use_hip(x, "bn_apply_act_mask"))


def batch_norm_act_dual(x, bn, xr, rbn):
    """relu(bn(x) + rbn(xr)) for two training-mode (weight, bias,
    running_mean, running_var, momentum, eps) parameter tuples."""
    xr, rmean, rrstd, rscale, rshift = _bn_stats_half(xr, *rbn[:4], True,
                                                      *rbn[4:])
    x, mean, rstd, scale, shift = _bn_stats_half(x, *bn[:4], True, *bn[4:])
    return _HIPBatchNormActDual.apply(x, bn[0], bn[1], xr, rbn[0], rbn[1],
                                      mean, rstd, scale, shift, rmean, rrstd,
                                      rscale, rshift)


class _Fork(torch.autograd.Function):
    """Explicit residual fork: ``x1, x2 = fork(x)`` marks the two consumers
    of a residual-block input so their backwards can chain gradient
    accumulation. The reference (see torchvision-style blocks in
    distribuuuu) leans on autograd's implicit fan-in add — a whole-tensor
    2-read/1-write elementwise pass per block. Here the first branch to
    finish deposits its gradient in a shared slot, the second accumulates
    into that buffer inside its dgrad epilogue (conv2d_dgrad_acc) or
    deposits gres (BN shortcut), and this backward detects pointer identity
    and skips the add. Falls back to g1 + g2 whenever a route could not
    accumulate."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None:
            return g2
        if g2 is None:
            return g1
        if g1.data_ptr() == g2.data_ptr():
            return g1
        return g1 + g2


def fork(x):
    """Split a residual-block input into (main, shortcut) fork handles."""
    if not (x.is_cuda and torch.is_grad_enabled() and x.requires_grad
            and x.dtype == torch.bfloat16 and use_hip(x, "conv2d_fwd")):
        return x, x
    x1, x2 = _Fork.apply(x)
    slot = {}
    x1._fork_slot = slot
    x2._fork_slot = slot
    return x1, x2


def _apply_act(y, act):
    if act == "relu":
        return F.relu(y, inplace=True)
    if act == "silu":
        return F.silu(y, inplace=True)
    if act == "sigmoid":
        return torch.sigmoid(y)
    return y


# ---------------------------------------------------------------------------
# Elementwise residual add + ReLU (K20/K8)
# ---------------------------------------------------------------------------
class _HIPAddReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        y = ext().add_relu_fwd(_cl(a), _cl(b))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        g = ext().relu_bwd(_cl(gy), y)
        return g, g


def add_relu(a, b):
    if use_hip(a, "add_relu_fwd"):
        return _HIPAddReLU.apply(a, b)
    return F.relu(a + b)


class _HIPSEScale(torch.autograd.Function):
    """SE gate application y = x * s[n, c] with fused backward
    (gx = gy * s and gs = sum_hw(gy * x) in one kernel pass — ATen needed
    two broadcast muls plus a reduction)."""

    @staticmethod
    def forward(ctx, x, s):
        x = _cl(x)
        s = _cl(s)
        y = ext().se_scale_fwd(x, s)
        ctx.save_for_backward(x, s)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, s = ctx.saved_tensors
        gx, gs = ext().se_scale_bwd(_cl(gy), x, s)
        return gx, gs


def se_scale(x, s):
    """x [N, C, H, W] * s [N, C, 1, 1] (the SE excite gate)."""
    if (use_hip(x, "se_scale_fwd") and x.shape[1] % 8 == 0
            and x.dtype == s.dtype):
        return _HIPSEScale.apply(x, s)
    return x * s


class _HIPReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ext().relu_fwd(_cl(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return ext().relu_bwd(_cl(gy), y)


def relu(x):
    if use_hip(x, "relu_fwd"):
        return _HIPReLU.apply(x)
    return F.relu(x)


# ---------------------------------------------------------------------------
# Pooling (K9/K10)
# ---------------------------------------------------------------------------
class _HIPMaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        x = _cl(x)
        y, idx = ext().maxpool_fwd(x, kernel, stride, padding)
        ctx.save_for_backward(idx)
        ctx.conf = (x.shape, kernel, stride, padding)
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        shape, kernel, stride, padding = ctx.conf
        gx = ext().maxpool_bwd(_cl(gy), idx, shape[2], shape[3], kernel,
                               stride, padding)
        return gx, None, None, None


def max_pool2d(x, kernel_size, stride, padding):
    if use_hip(x, "maxpool_fwd"):
        return _HIPMaxPool2d.apply(x, kernel_size, stride, padding)
    return F.max_pool2d(x, kernel_size, stride, padding)


class _HIPGlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        ctx.in_shape = x.shape
        return ext().gap_fwd(x)  # [N, C, 1, 1]

    @staticmethod
    def backward(ctx, gy):
        n, c, h, w = ctx.in_shape
        return ext().gap_bwd(gy.contiguous(), h, w)


def adaptive_avg_pool2d(x, output_size=1):
    if output_size in (1, (1, 1)) and use_hip(x, "gap_fwd"):
        return _HIPGlobalAvgPool.apply(x)
    return F.adaptive_avg_pool2d(x, output_size)


def avg_pool2d(x, kernel_size, stride=None):
    if use_hip(x, "avgpool_fwd"):
        return _HIPAvgPool2d.apply(x, kernel_size, stride or kernel_size)
    return F.avg_pool2d(x, kernel_size, stride)


class _HIPAvgPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride):
        x = _cl(x)
        ctx.conf = (x.shape, kernel, stride)
        return ext().avgpool_fwd(x, kernel, stride)

    @staticmethod
    def backward(ctx, gy):
        shape, kernel, stride = ctx.conf
        gx = ext().avgpool_bwd(_cl(gy), kernel, stride, shape[2], shape[3])
        return gx, None, None


# ---------------------------------------------------------------------------
# Linear / fc (K11) — MFMA GEMM
# ---------------------------------------------------------------------------
class _HIPLinear(torch.autograd.Function):
    """fc via the MFMA NT GEMM (K11). The fc is tiny next to the convs; the
    transposes in backward are ATen copies of <2 MB tensors."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.contiguous()
        w2 = w.contiguous()
        y = ext().gemm_nt(x2, w2)
        if b is not None:
            y = y + b
        ctx.save_for_backward(x2, w2)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        e = ext()
        gx = e.gemm_nt(gy, w.t().contiguous())
        gyt, xt = gy.t(), x.t()
        pad = _pad8(gy.shape[0]) - gy.shape[0]
        if pad:
            # the GEMM reduces over the batch and needs it 8-aligned: zero
            # rows add nothing (a loader's last, shorter batch)
            gyt, xt = F.pad(gyt, (0, pad)), F.pad(xt, (0, pad))
        gw = e.gemm_nt(gyt.contiguous(), xt.contiguous())
        gb = gy.sum(0) if ctx.has_bias else None
        return gx, gw, gb


def linear(x, weight, bias=None):
    if (use_hip(x, "gemm_nt")
            and x.dtype in (torch.bfloat16, torch.float32) and x.dim() == 2
            and x.shape[1] % 8 == 0 and weight.shape[0] % 8 == 0):
        return _HIPLinear.apply(x, weight, bias)
    if x.is_cuda:
        fallback_warn("linear",
                      f"dtype {x.dtype} dim {x.dim()} shape {tuple(x.shape)}")
    return F.linear(x, weight, bias)


# ---------------------------------------------------------------------------
# Cross-entropy (K12)
# ---------------------------------------------------------------------------
class _HIPCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.contiguous()
        loss, lse = ext().ce_fwd(logits, target)
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, gl):
        logits, target, lse = ctx.saved_tensors
        gx = ext().ce_bwd(logits, target, lse, gl.contiguous())
        return gx, None


class _HIPSoftCrossEntropy(torch.autograd.Function):
    """Cross-entropy on smoothed, batch-mixed targets (soft_targets below).
    `lam` is a float32 device tensor of one element that both kernels read
    from memory, never a launch argument: a hipGraph replay follows the value
    filled in before it. None means lam = 1."""

    @staticmethod
    def forward(ctx, logits, target, lam, eps):
        logits = logits.contiguous()
        loss, lse = ext().ce_soft_fwd(logits, target, lam, eps)
        ctx.save_for_backward(logits, target, lse)
        ctx.lam = lam
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, gl):
        logits, target, lse = ctx.saved_tensors
        gx = ext().ce_soft_bwd(logits, target, lse, gl.contiguous(), ctx.lam,
                               ctx.eps)
        return gx, None, None, None


def soft_targets(target, num_classes, label_smoothing=0.0, lam=None,
                 dtype=torch.float32):
    """q[n, j] = (1-eps) * (lam*[j==a] + (1-lam)*[j==b]) + eps/K with
    a = target[n] and b = target[N-1-n]: sample n is paired with sample
    N-1-n (the batch against its own reversal), lam weighs its own label."""
    q = F.one_hot(target, num_classes).to(dtype)
    if lam is not None:
        lam = lam.to(device=q.device, dtype=dtype).reshape(())
        q = lam * q + (1 - lam) * q.flip(0)
    return (1.0 - label_smoothing) * q + label_smoothing / num_classes


def cross_entropy(logits, target, label_smoothing=0.0, lam=None):
    """Mean cross-entropy. `label_smoothing` (host float in [0, 1)) and `lam`
    (one-element float32 tensor, the weight of each sample's own label
    against its batch-reversal partner's) select the soft-target loss; with
    both at their defaults this is the hard-target loss and kernels."""
    if label_smoothing == 0.0 and lam is None:
        if use_hip(logits, "ce_fwd"):
            return _HIPCrossEntropy.apply(logits, target)
        return F.cross_entropy(logits, target)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got "
                         f"{label_smoothing}")
    if use_hip(logits, "ce_soft_fwd"):
        return _HIPSoftCrossEntropy.apply(logits, target, lam,
                                          float(label_smoothing))
    q = soft_targets(target, logits.shape[1], label_smoothing, lam,
                     logits.dtype)
    return F.cross_entropy(logits, q)


# ---------------------------------------------------------------------------
# Batch mixing (mixup / CutMix) against the reversed batch
# ---------------------------------------------------------------------------
def batch_mix(x, lam, box=None):
    """Mix every sample of x [N, C, H, W] with its partner x[N-1-n], out of
    place. box None: mixup, lam * x + (1 - lam) * partner in fp32, rounded
    once to x's dtype (lam 1 and 0 return x and x.flip(0) to the bit).
    box (y0, y1, x0, x1): CutMix, the partner's pixels inside
    [y0, y1) x [x0, x1) and x's own outside; lam is not used."""
    if x.dim() != 4:
        raise ValueError("batch_mix expects [N, C, H, W]")
    if not (x.is_contiguous()
            or x.is_contiguous(memory_format=torch.channels_last)):
        # dense in its own memory format
        nhwc = x.shape[1] > 1 and x.stride(1) == 1
        x = x.contiguous(memory_format=torch.channels_last if nhwc
                         else torch.contiguous_format)
    if box is not None:
        y0, y1, x0, x1 = (int(v) for v in box)
        h, w = x.shape[2], x.shape[3]
        if not (0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w):
            raise ValueError(f"box {box} outside the {h}x{w} image")
    elif not 0.0 <= lam <= 1.0:
        raise ValueError(f"lam must be in [0, 1], got {lam}")
    if (x.dtype in (torch.float32, torch.bfloat16)
            and use_hip(x, "batch_mix")):
        if box is None:
            return ext().batch_mix(x, 0, float(lam), 0, 0, 0, 0)
        return ext().batch_mix(x, 1, 1.0, y0, y1, x0, x1)
    if x.is_cuda and x.dtype not in (torch.float32, torch.bfloat16):
        fallback_warn("batch_mix", f"dtype {x.dtype} (fp32/bf16 kernels)")
    if box is not None:
        inside = torch.zeros(1, 1, x.shape[2], x.shape[3], dtype=torch.bool,
                             device=x.device)
        inside[:, :, y0:y1, x0:x1] = True
        return torch.where(inside, x.flip(0), x)
    lam32 = torch.tensor(lam, dtype=torch.float32)
    if lam32 == 1:
        return x.clone()
    if lam32 == 0:
        return x.flip(0)
    return (lam32 * x.float() + (1 - lam32) * x.flip(0).float()).to(x.dtype)


# ---------------------------------------------------------------------------
# Dropout (K19): counter-based mask — backward regenerates it from the same
# (seed, index) hash instead of storing a mask tensor
# ---------------------------------------------------------------------------
class _HIPDropout(torch.autograd.Function):
    """Mask = hash(seed, element index) in the channels_last layout, so
    backward regenerates it bit-exactly. The seed is drawn host-side per
    call; under hipGraph capture it would freeze across replays, which is
    what the step counter below is for."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p = p
        ctx.seed = seed
        return ext().dropout_fwd(_cl(x), p, seed)

    @staticmethod
    def backward(ctx, gy):
        return ext().dropout_fwd(_cl(gy), ctx.p, ctx.seed), None, None


class _HIPDropoutDev(torch.autograd.Function):
    """Same mask hash with the seed formed in the kernel from a host-drawn
    salt (fixed per call site once captured) and a device step counter. The
    counter only advances between steps, so backward regenerates the
    forward's mask."""

    @staticmethod
    def forward(ctx, x, p, salt, step):
        ctx.p = p
        ctx.salt = salt
        ctx.step = step
        return ext().dropout_fwd_dev(_cl(x), p, salt, step)

    @staticmethod
    def backward(ctx, gy):
        return (ext().dropout_fwd_dev(_cl(gy), ctx.p, ctx.salt, ctx.step),
                None, None, None)


# int64[1] device tensor while a captured train step is being recorded
# (graph_step.GraphedTrainStep), else None
_STEP_COUNTER = None
_STEP_COUNTER_USES = 0


def install_step_counter(counter):
    """Key every GPU dropout mask drawn from now on by `counter` (an int64
    device tensor of one element) instead of a host-drawn seed alone."""
    global _STEP_COUNTER, _STEP_COUNTER_USES
    if counter.dtype != torch.int64 or counter.numel() != 1:
        raise ValueError("step counter must be an int64 tensor of one element")
    _STEP_COUNTER = counter
    _STEP_COUNTER_USES = 0


def remove_step_counter():
    """Back to host-drawn seeds; returns how many dropout calls used the
    counter while it was installed."""
    global _STEP_COUNTER
    _STEP_COUNTER = None
    return _STEP_COUNTER_USES


def dropout(x, p, training):
    global _STEP_COUNTER_USES
    if p == 0.0 or not training:
        return x
    if use_hip(x, "dropout_fwd"):
        import random as _random

        seed = _random.getrandbits(62)
        if _STEP_COUNTER is not None and use_hip(x, "dropout_fwd_dev"):
            _STEP_COUNTER_USES += 1
            return _HIPDropoutDev.apply(x, p, seed, _STEP_COUNTER)
        return _HIPDropout.apply(x, p, seed)
    return F.dropout(x, p, training)
