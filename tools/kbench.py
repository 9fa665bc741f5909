"""Per-kernel micro-benchmarks on representative ResNet-50 shapes.

Usage (on a GPU box): python tools/kbench.py [--deterministic] [group ...]
Groups: bn conv wgrad pool fused gemm sgd mix se dw gconv dense fp32
mhsa_stream mhsa_f32 all
Prints achieved GB/s (memory-bound ops) or TF/s (MFMA ops) per shape.
--deterministic: the wgrad rows time each shape in both modes, atomic and
deterministic (docs/DETERMINISM.md), side by side.
Without it the wgrad group ends with the accumulate-mode table: every distinct
ResNet-50 wgrad launch under DISTRIBUUUU_WGRAD_ACC=atomic and =slab, alternated
over three passes; --slab-blocks=256,384 adds slab columns with another
block-count target (DISTRIBUUUU_WGRAD_SLAB_BLOCKS).
"""

import sys
import time

import torch

sys.path.insert(0, ".")
from distribuuuu_amd.ops.dispatch import require_ext  # noqa: E402

e = require_ext()
DEV = "cuda"


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


BN_SHAPES = [
    (256, 64, 112, 112),
    (256, 256, 56, 56),
    (256, 512, 28, 28),
    (256, 1024, 14, 14),
    (256, 2048, 7, 7),
]

CONV_SHAPES = [
    # (N, C, H, W, K, R, stride) — ResNet-50 hot layers
    (256, 64, 56, 56, 64, 3, 1),
    (256, 64, 56, 56, 256, 1, 1),
    (256, 256, 56, 56, 64, 1, 1),
    (256, 128, 28, 28, 128, 3, 1),
    (256, 256, 14, 14, 256, 3, 1),
    (256, 512, 7, 7, 512, 3, 1),
    (256, 256, 56, 56, 512, 1, 2),
    (256, 128, 56, 56, 128, 3, 2),
    (256, 3, 224, 224, 64, 7, 2),
]


def bench_bn():
    print("== bn kernels (GB/s moved) ==")
    for shp in BN_SHAPES:
        n, c, h, w = shp
        x = _cl(torch.randn(*shp, device=DEV, dtype=torch.bfloat16))
        nbytes = x.numel() * 2
        t = timeit(lambda: e.bn_sums(x))
        print(f"bn_sums      {str(shp):22s} {t*1e6:8.1f} us  {nbytes/t/1e9:7.0f} GB/s")
        scale = torch.randn(c, device=DEV)
        shift = torch.randn(c, device=DEV)
        res = _cl(torch.randn_like(x))
        t = timeit(lambda: e.bn_apply_act(x, scale, shift, 1, res))
        print(f"bn_apply+res {str(shp):22s} {t*1e6:8.1f} us  {3*nbytes/t/1e9:7.0f} GB/s")
        gy = _cl(torch.randn_like(x))
        y = _cl(torch.randn_like(x))
        mean = torch.zeros(c, device=DEV)
        rstd = torch.ones(c, device=DEV)
        g = torch.ones(c, device=DEV)
        b = torch.zeros(c, device=DEV)
        sc = torch.ones(c, device=DEV)
        sh = torch.zeros(c, device=DEV)
        t = timeit(lambda: e.bn_bwd(gy, x, res, mean, rstd, g, sc, sh, 1,
                                    True, True))
        print(f"bn_bwd(all)  {str(shp):22s} {t*1e6:8.1f} us  {8*nbytes/t/1e9:7.0f} GB/s")


def bench_conv():
    print("== conv fwd/dgrad (TF/s) ==")
    for shp in CONV_SHAPES:
        n, c, h, w, k, r, s = shp
        cc = 8 if c < 8 else c
        x = _cl(torch.randn(n, cc, h, w, device=DEV, dtype=torch.bfloat16))
        wt = _cl(torch.randn(k, cc, r, r, device=DEV, dtype=torch.bfloat16))
        p = r // 2
        ho = (h + 2 * p - r) // s + 1
        flops = 2.0 * n * ho * ho * k * cc * r * r
        t = timeit(lambda: e.conv2d_fwd(x, wt, s, s, p, p, 1, 1, 1))
        line = f"fwd   {str(shp):26s} {t*1e6:8.1f} us  {flops/t/1e12:6.1f} TF"
        gy = _cl(torch.randn(n, k, ho, ho, device=DEV, dtype=torch.bfloat16))
        if c >= 8:
            t2 = timeit(lambda: e.conv2d_dgrad(gy, wt, h, w, s, s, p, p, 1, 1, 1))
            line += f" | dgrad {t2*1e6:8.1f} us {flops/t2/1e12:6.1f} TF"
        print(line)
        if (c, k, r, s) == (64, 64, 3, 1) and e.conv3x3_halo_admits(n, h, w):
            _bench_halo_routes(x, wt, flops)


def _bench_halo_routes(x, wt, flops, passes=3):
    """3x3 64->64: global-fed kernel vs halo-staged kernel, alternated, through
    the debug entry that forces the route. The dgrad is the same launch with
    the flipped weight."""
    wf = e.weight_flip_t(wt, 1)
    nbytes = 2 * x.numel() * 2 + wt.numel() * 2
    for i in range(passes):
        for name, wgt in (("fwd", wt), ("dgrad", wf)):
            row = f"  pass {i} {name:5s}"
            for label, halo in (("old", False), ("halo", True)):
                t = timeit(lambda: e.conv2d_fwd_halo_dbg(x, wgt, False, halo))
                row += (f" | {label:4s} {t*1e6:7.1f} us {flops/t/1e12:6.1f} TF"
                        f" {nbytes/t/1e9:6.0f} GB/s")
            print(row)


def bench_wgrad(deterministic=False, slab_blocks=()):
    from distribuuuu_amd import ops

    print("== conv wgrad (TF/s) ==" if not deterministic else
          "== conv wgrad, atomic vs deterministic (TF/s) ==")
    for shp in CONV_SHAPES:
        n, c, h, w, k, r, s = shp
        cc = 8 if c < 8 else c
        x = _cl(torch.randn(n, cc, h, w, device=DEV, dtype=torch.bfloat16))
        p = r // 2
        ho = (h + 2 * p - r) // s + 1
        gy = _cl(torch.randn(n, k, ho, ho, device=DEV, dtype=torch.bfloat16))
        flops = 2.0 * n * ho * ho * k * cc * r * r
        t = timeit(lambda: e.conv2d_wgrad(gy, x, r, r, s, s, p, p, 1, 1, 1))
        line = f"wgrad {str(shp):26s} {t*1e6:8.1f} us  {flops/t/1e12:6.1f} TF"
        if deterministic:
            ops.set_deterministic(True)
            try:
                td = timeit(
                    lambda: e.conv2d_wgrad(gy, x, r, r, s, s, p, p, 1, 1, 1))
            finally:
                ops.set_deterministic(False)
            line += (f" | det {td*1e6:8.1f} us {flops/td/1e12:6.1f} TF"
                     f"  x{td/t:4.2f}")
        print(line)
    if not deterministic:
        _bench_wgrad_acc(slab_blocks)


def _resnet50_wgrad_shapes(n=256):
    """ResNet-50's distinct weight-gradient launches at batch n, in network
    order: ((N, C, H, W, K, R, stride, pad), calls per step). The stem sees
    its input zero-padded to 8 channels."""
    shapes = {(n, 8, 224, 224, 64, 7, 2, 3): 1}
    cin, h = 64, 56
    for width, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2),
                                  (512, 3, 2)):
        for b in range(blocks):
            st = stride if b == 0 else 1
            convs = [(n, cin, h, h, width, 1, 1, 0),
                     (n, width, h, h, width, 3, st, 1),
                     (n, width, h // st, h // st, 4 * width, 1, 1, 0)]
            if b == 0:
                convs.append((n, cin, h, h, 4 * width, 1, st, 0))
            for c in convs:
                shapes[c] = shapes.get(c, 0) + 1
            cin, h = 4 * width, h // st
    return list(shapes.items())


def _bench_wgrad_acc(slab_blocks=(), passes=3):
    """Accumulate modes of the split-m wgrad (DISTRIBUUUU_WGRAD_ACC), forced
    through the knob and alternated over `passes` passes per shape. Op time is
    the whole conv2d_wgrad call: accumulator setup (memset or nothing), the
    wgrad kernel, and the cast or the ordered reduction. `auto` is what the
    classifier picks at default gates; extra `slab@B` columns run slab with
    the csteps shrink loop aiming at B blocks instead of 512."""
    import os

    print("== conv wgrad accumulate modes, ResNet-50 batch 256 (us; family "
          "csteps x chunks; slot = Kt*RSC*4) ==")
    cols = [("atomic", {"DISTRIBUUUU_WGRAD_ACC": "atomic"}),
            ("slab", {"DISTRIBUUUU_WGRAD_ACC": "slab"})]
    for b in slab_blocks:
        cols.append((f"slab@{b}", {"DISTRIBUUUU_WGRAD_ACC": "slab",
                                   "DISTRIBUUUU_WGRAD_SLAB_BLOCKS": str(b)}))
    knobs = ("DISTRIBUUUU_WGRAD_ACC", "DISTRIBUUUU_WGRAD_SLAB_BLOCKS")
    saved = {k: os.environ.pop(k, None) for k in knobs}

    def with_env(env, fn):
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k in knobs:
                os.environ.pop(k, None)

    try:
        for shp, calls in _resnet50_wgrad_shapes():
            n, c, h, w, k, r, s, p = shp
            x = _cl(torch.randn(n, c, h, w, device=DEV, dtype=torch.bfloat16))
            ho = (h + 2 * p - r) // s + 1
            gy = _cl(torch.randn(n, k, ho, ho, device=DEV,
                                 dtype=torch.bfloat16))
            args = (gy, x, r, r, s, s, p, p, 1, 1, 1)
            route = lambda: e.conv2d_wgrad_route(*args)
            auto = with_env({}, route)
            head = f"{str(shp):38s} x{calls} slot {k*r*r*c*4/1024:7.0f} KB"
            for label, env in cols:
                fam, cs, ch, acc = with_env(env, route)
                head += f" | {label} {fam} {cs}x{ch} {acc}"
            print(head + f" | auto -> {auto[3]}")
            for i in range(passes):
                row = f"  pass {i}"
                for label, env in cols:
                    t = with_env(env, lambda: timeit(
                        lambda: e.conv2d_wgrad(*args)))
                    row += f" | {label} {t*1e6:7.1f}"
                print(row)
            del x, gy
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def bench_pool():
    print("== pool (GB/s) ==")
    x = _cl(torch.randn(256, 64, 112, 112, device=DEV, dtype=torch.bfloat16))
    nb = x.numel() * 2
    t = timeit(lambda: e.maxpool_fwd(x, 3, 2, 1))
    print(f"maxpool_fwd  {t*1e6:8.1f} us  {nb/t/1e9:7.0f} GB/s (input read)")
    y, idx = e.maxpool_fwd(x, 3, 2, 1)
    gy = _cl(torch.randn_like(y))
    t = timeit(lambda: e.maxpool_bwd(gy, idx, 112, 112, 3, 2, 1))
    print(f"maxpool_bwd  {t*1e6:8.1f} us  {nb/t/1e9:7.0f} GB/s (gx write)")
    x2 = _cl(torch.randn(256, 2048, 7, 7, device=DEV, dtype=torch.bfloat16))
    t = timeit(lambda: e.gap_fwd(x2))
    print(f"gap_fwd      {t*1e6:8.1f} us  {x2.numel()*2/t/1e9:7.0f} GB/s")


def bench_fused():
    """Fused stem BN+ReLU+maxpool and the dual (join + shortcut BN) apply,
    each next to the kernels it replaces. GB/s counts the fused op's own
    compulsory bytes (gathers of the pooled gradient counted once per
    kernel)."""
    print("== fused bn ops vs the chains they replace ==")
    shp = (256, 64, 112, 112)
    c = shp[1]
    x = _cl(torch.randn(*shp, device=DEV, dtype=torch.bfloat16))
    nb = x.numel() * 2
    g = torch.rand(c, device=DEV) + 0.5
    b = torch.zeros(c, device=DEV)
    mean, rstd, sc, sh = e.bn_stats(x, g, b, None, None, 0.1, 1e-5, True, None)
    t_ap = timeit(lambda: e.bn_apply_act(x, sc, sh, 1, None))
    y = e.bn_apply_act(x, sc, sh, 1, None)
    t_mp = timeit(lambda: e.maxpool_fwd(y, 3, 2, 1))
    t_f = timeit(lambda: e.bn_act_maxpool_fwd(x, sc, sh, 1))
    fb = nb + nb // 4 + nb // 8
    print(f"stem fwd  bn_apply {t_ap*1e6:7.1f} + maxpool_fwd {t_mp*1e6:7.1f} "
          f"= {(t_ap+t_mp)*1e6:7.1f} us | fused {t_f*1e6:7.1f} us "
          f"{fb/t_f/1e9:6.0f} GB/s")
    yp, idx = e.bn_act_maxpool_fwd(x, sc, sh, 1)
    del y
    gp = _cl(torch.randn_like(yp))
    t_mb = timeit(lambda: e.maxpool_bwd(gp, idx, shp[2], shp[3], 3, 2, 1))
    gfull = e.maxpool_bwd(gp, idx, shp[2], shp[3], 3, 2, 1)
    t_bb = timeit(lambda: e.bn_bwd(gfull, x, None, mean, rstd, g, sc, sh, 1,
                                   True, False))
    del gfull
    t_fb = timeit(lambda: e.bn_pool_bwd(gp, idx, x, mean, rstd, g, sc, sh, 1,
                                        True))
    bb = 3 * nb + 2 * (nb // 4 + nb // 8)
    print(f"stem bwd  maxpool_bwd {t_mb*1e6:7.1f} + bn_bwd {t_bb*1e6:7.1f} "
          f"= {(t_mb+t_bb)*1e6:7.1f} us | fused {t_fb*1e6:7.1f} us "
          f"{bb/t_fb/1e9:6.0f} GB/s")
    shp = (256, 256, 56, 56)
    c = shp[1]
    x = _cl(torch.randn(*shp, device=DEV, dtype=torch.bfloat16))
    xr = _cl(torch.randn_like(x))
    nb = x.numel() * 2
    sc, sh, rsc, rsh = (torch.randn(c, device=DEV) for _ in range(4))
    t_id = timeit(lambda: e.bn_apply_act(xr, rsc, rsh, 0, None))
    ident = e.bn_apply_act(xr, rsc, rsh, 0, None)
    t_jn = timeit(lambda: e.bn_apply_act_mask(x, sc, sh, 1, ident))
    t_du = timeit(lambda: e.bn_apply_act_mask(x, sc, sh, 1, xr, rsc, rsh))
    db = 3 * nb + nb // 16
    print(f"dual apply {str(shp):20s} shortcut apply {t_id*1e6:7.1f} + join "
          f"{t_jn*1e6:7.1f} = {(t_id+t_jn)*1e6:7.1f} us | fused "
          f"{t_du*1e6:7.1f} us {db/t_du/1e9:6.0f} GB/s")


def bench_gemm():
    print("== gemm_nt (TF/s) ==")
    for m, n, k in [(256, 1000, 2048), (4096, 4096, 4096), (8192, 8192, 8192)]:
        a = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)
        b = torch.randn(n, k, device=DEV, dtype=torch.bfloat16)
        t = timeit(lambda: e.gemm_nt(a, b))
        print(f"gemm_nt {m}x{n}x{k}: {t*1e6:8.1f} us  {2.0*m*n*k/t/1e12:6.1f} TF")


def _resnet50_shapes():
    """Parameter shapes of torchvision-style ResNet-50 (161 tensors, 25.6M
    elements): conv weights, BN weight/bias pairs, the classifier."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    cin = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            for k, c, r in ((width, cin, 1), (width, width, 3),
                            (4 * width, width, 1)):
                shapes += [(k, c, r, r), (k,), (k,)]
            if b == 0:
                shapes += [(4 * width, cin, 1, 1), (4 * width,), (4 * width,)]
            cin = 4 * width
    return shapes + [(1000, 2048), (1000,)]


def bench_sgd():
    from distribuuuu_amd.ops.optim import HIPLARS, HIPSGD

    print("== optimizer step over ResNet-50's parameters (bf16 params and "
          "grads, fp32 master + momentum) ==")
    shapes = _resnet50_shapes()
    numel = sum(torch.Size(s).numel() for s in shapes)
    kw = dict(lr=0.0, momentum=0.9, weight_decay=5e-5, nesterov=True)
    # bytes per element: grad 2 + master 4+4 + momentum 4+4 + param 2; the
    # LARS norm pass reads master and grad once more
    for name, klass, nbytes in (("sgd_step", HIPSGD, 20),
                                ("lars_step", HIPLARS, 26)):
        params = []
        for s in shapes:
            p = torch.randn(s, device=DEV).to(torch.bfloat16)
            if len(s) == 4:
                p = _cl(p)
            p.grad = torch.randn_like(p)
            params.append(p)
        opt = klass(params, **kw)
        opt.step()  # first step: state and the cached chunk table
        group = opt.param_groups[0]
        table = group["_hip_table_dev"]
        tail = (0.0, 0.9, 0.0, 5e-5, True)  # lr, momentum, dampening, wd
        if klass is HIPSGD:
            t = timeit(lambda: e.sgd_step(table, *tail))
        else:
            ws = group["_hip_table_ws"]
            t = timeit(lambda: e.lars_step(
                table, ws["nchunks"], ws["part"], ws["sqnorm"], ws["q"],
                *tail, 1e-3, 1e-8))
        print(f"{name:10s} {len(shapes)} tensors {numel/1e6:5.1f}M elem "
              f"{t*1e6:8.1f} us  {nbytes*numel/t/1e9:7.0f} GB/s")


def bench_mix(passes=3):
    """batch_mix next to the ATen composition it replaces, alternated in one
    session. Bytes are computed from the shape: the fused mixup reads x twice
    and writes once (3 tensors), CutMix reads and writes once (the box is
    read from the partner INSTEAD of the sample itself: 2 tensors). ATen's
    mixup is flip (2) + two muls (2 + 2) + add (3) = 9 tensors, its CutMix
    flip (2) + where (3, plus the broadcast mask) = 5."""
    print("== batch_mix vs ATen composition (256, 3, 224, 224) bf16 "
          "channels_last ==")
    x = _cl(torch.randn(256, 3, 224, 224, device=DEV, dtype=torch.bfloat16))
    nb = x.numel() * 2
    lam = 0.3
    h, w = x.shape[2], x.shape[3]
    box = (37, 37 + 112, 51, 51 + 112)  # a quarter of the image, odd offsets
    inside = torch.zeros(1, 1, h, w, dtype=torch.bool, device=DEV)
    inside[:, :, box[0]:box[1], box[2]:box[3]] = True
    rows = [
        ("mixup  fused", lambda: e.batch_mix(x, 0, lam, 0, 0, 0, 0), 3 * nb),
        ("mixup  aten ", lambda: x * lam + x.flip(0) * (1 - lam), 9 * nb),
        ("cutmix fused", lambda: e.batch_mix(x, 1, 1.0, *box), 2 * nb),
        ("cutmix aten ", lambda: torch.where(inside, x.flip(0), x),
         5 * nb + inside.numel()),
    ]
    for p in range(passes):
        for name, fn, moved in rows:
            t = timeit(fn, iters=500, warmup=20)  # windows of 12-60 ms
            print(f"pass {p} {name} {t*1e6:8.1f} us  {moved/1e6:7.1f} MB "
                  f"{moved/t/1e9:7.0f} GB/s")


def bench_se(passes=3):
    """se_gate forward + backward: the fused kernels next to the conv2d / act /
    conv2d / sigmoid composition (DISTRIBUUUU_SE_FUSE=0), alternated in one
    session, on every distinct SE (C, Cr) of EfficientNet-B0 at N=256 and of
    RegNetY-320 at N=64."""
    import os

    from distribuuuu_amd import models
    from distribuuuu_amd.ops import functional as DF

    print("== se_gate fwd+bwd, fused vs composition (us) ==")
    for arch, n, act in (("efficientnet_b0", 256, "silu"),
                         ("regnety_320", 64, "relu")):
        with torch.device("meta"):
            net = getattr(models, arch)()
        pairs = sorted({(m.shape[1], m.shape[0])
                        for k, m in net.state_dict().items()
                        if k.endswith(("se.conv_reduce.weight",
                                       "se.fc1.weight"))})
        for c, cr in pairs:
            bf = dict(device=DEV, dtype=torch.bfloat16)
            args = [torch.randn(n, c, 1, 1, **bf),
                    torch.randn(cr, c, 1, 1, **bf) / c ** 0.5,
                    torch.zeros(cr, **bf),
                    torch.randn(c, cr, 1, 1, **bf) / cr ** 0.5,
                    torch.zeros(c, **bf)]
            args = [a.requires_grad_() for a in args]
            gs = torch.randn(n, c, 1, 1, **bf)

            def step():
                s = DF.se_gate(*args, act)
                torch.autograd.grad(s, args, gs)

            row = {"1": [], "0": []}
            for _ in range(passes):
                for fuse in ("1", "0"):
                    os.environ["DISTRIBUUUU_SE_FUSE"] = fuse
                    row[fuse].append(timeit(step, iters=100, warmup=10) * 1e6)
            os.environ.pop("DISTRIBUUUU_SE_FUSE")
            fmt = lambda v: " ".join(f"{t:7.1f}" for t in v)  # noqa: E731
            print(f"{arch:16s} N={n:3d} C={c:4d} Cr={cr:3d}  fused "
                  f"{fmt(row['1'])}   composition {fmt(row['0'])}")


# EfficientNet-B0's distinct depthwise convs: (C, H, R, stride), pad R // 2
DW_SHAPES = [(32, 112, 3, 1), (96, 112, 3, 2), (144, 56, 3, 1),
             (144, 56, 5, 2), (240, 28, 5, 1), (240, 28, 3, 2),
             (480, 14, 3, 1), (480, 14, 5, 1), (672, 14, 5, 1),
             (672, 14, 5, 2), (1152, 7, 5, 1), (1152, 7, 3, 1)]


def bench_dw(n=256, passes=3):
    """Depthwise fwd / dgrad / wgrad: the LDS-tiled route next to the generic
    kernels (DISTRIBUUUU_DW_TILE=0), alternated over `passes` passes in one
    session. GB/s is against each pass's minimum traffic: every operand read
    once and the result written once."""
    import os

    print(f"== depthwise, tiled vs generic, EfficientNet-B0 at N={n} "
          "(us per call; GB/s of minimum traffic) ==")
    saved = os.environ.pop("DISTRIBUUUU_DW_TILE", None)
    try:
        for c, h, r, s in DW_SHAPES:
            p = r // 2
            ho = (h + 2 * p - r) // s + 1
            bf = dict(device=DEV, dtype=torch.bfloat16)
            x = _cl(torch.randn(n, c, h, h, **bf))
            wt = _cl(torch.randn(c, 1, r, r, **bf))
            gy = _cl(torch.randn(n, c, ho, ho, **bf))
            io = (x.numel() + gy.numel()) * 2
            ops = (("fwd", lambda: e.dwconv_fwd(x, wt, s, s, p, p)),
                   ("dgrad", lambda: e.dwconv_dgrad(gy, wt, h, h, s, s, p, p)),
                   ("wgrad", lambda: e.dwconv_wgrad(gy, x, r, r, s, s, p, p)))
            for name, fn in ops:
                route = e.dwconv_route(x, r, r, s, s, p, p, name)
                rows = {"1": [], "0": []}
                for _ in range(passes):
                    for knob in ("1", "0"):
                        os.environ["DISTRIBUUUU_DW_TILE"] = knob
                        rows[knob].append(timeit(fn, iters=50, warmup=5))
                os.environ.pop("DISTRIBUUUU_DW_TILE")
                fmt = lambda v: " ".join(  # noqa: E731
                    f"{t*1e6:7.1f}" for t in v)
                best = {k: min(v) for k, v in rows.items()}
                print(f"C={c:4d} {h:3d}x{h:<3d} {r}x{r} s{s} {name:5s} "
                      f"tiled {fmt(rows['1'])} ({io/best['1']/1e9:5.0f} GB/s)"
                      f" | generic {fmt(rows['0'])} "
                      f"({io/best['0']/1e9:5.0f} GB/s) | {route[:6]}")
            del x, gy
    finally:
        if saved is not None:
            os.environ["DISTRIBUUUU_DW_TILE"] = saved


def bench_dw_f32(n=128, passes=3):
    """fp32 depthwise fwd / dgrad / wgrad through functional.conv2d: the
    exact-fp32 tiled route next to the path the same call took before
    (DISTRIBUUUU_DW_TILE=0: eight channels packed into a block-diagonal group
    on the fp32 implicit GEMM), alternated over `passes` passes in one
    session. GB/s is against each pass's minimum traffic: both activations
    once. A conv keeps the route only if the sum of its three tiled passes
    beats the packed path in every pass."""
    import os

    from distribuuuu_amd.ops import functional as DF

    print(f"== fp32 depthwise, tiled vs packed igemm, EfficientNet-B0 at "
          f"N={n} (us per call; GB/s of minimum traffic) ==")
    saved = os.environ.pop("DISTRIBUUUU_DW_TILE", None)
    try:
        for c, h, r, s in DW_SHAPES:
            p = r // 2
            ho = (h + 2 * p - r) // s + 1
            f32 = dict(device=DEV, dtype=torch.float32)
            x = _cl(torch.randn(n, c, h, h, **f32)).requires_grad_()
            wt = _cl(torch.randn(c, 1, r, r, **f32)).requires_grad_()
            gy = _cl(torch.randn(n, c, ho, ho, **f32))
            io = (x.numel() + gy.numel()) * 4
            conv = lambda a, b: DF.conv2d(  # noqa: E731
                a, b, None, (s, s), (p, p), (1, 1), c)
            # one autograd graph per route and pass, as in bench_gconv
            yd, yw = {}, {}
            for knob in ("1", "0"):
                os.environ["DISTRIBUUUU_DW_TILE"] = knob
                yd[knob] = conv(x, wt.detach())
                yw[knob] = conv(x.detach(), wt)

            def fwd(_knob):
                with torch.no_grad():
                    conv(x, wt)

            ops = (("fwd", fwd),
                   ("dgrad", lambda k: torch.autograd.grad(
                       yd[k], x, gy, retain_graph=True)),
                   ("wgrad", lambda k: torch.autograd.grad(
                       yw[k], wt, gy, retain_graph=True)))
            tot = {"1": [0.0] * passes, "0": [0.0] * passes}
            for name, fn in ops:
                rows = {"1": [], "0": []}
                for i in range(passes):
                    for knob in ("1", "0"):
                        os.environ["DISTRIBUUUU_DW_TILE"] = knob
                        rows[knob].append(timeit(lambda: fn(knob),
                                                 iters=30, warmup=5))
                        tot[knob][i] += rows[knob][-1]
                fmt = lambda v: " ".join(  # noqa: E731
                    f"{t*1e6:7.1f}" for t in v)
                print(f"C={c:4d} {h:3d}x{h:<3d} {r}x{r} s{s} {name:5s} "
                      f"tiled {fmt(rows['1'])} "
                      f"({io/min(rows['1'])/1e9:5.0f} GB/s)"
                      f" | packed {fmt(rows['0'])}")
            os.environ.pop("DISTRIBUUUU_DW_TILE")
            verdict = "keep" if max(tot["1"]) < min(tot["0"]) else "LOSES"
            print(f"C={c:4d} {h:3d}x{h:<3d} {r}x{r} s{s} sum   "
                  f"tiled {fmt(tot['1'])} | packed {fmt(tot['0'])} | "
                  f"{verdict}")
            del x, gy, yd, yw
    finally:
        os.environ.pop("DISTRIBUUUU_DW_TILE", None)
        if saved is not None:
            os.environ["DISTRIBUUUU_DW_TILE"] = saved


# The in-range grouped 3x3 convs (C, w, H, stride), pad 1, of
# resnext50_32x4d, then those only resnext101_32x8d has
GCONV_SHAPES = [(128, 4, 56, 1), (256, 8, 56, 2), (256, 8, 28, 1),
                (512, 16, 28, 2), (512, 16, 14, 1), (1024, 32, 14, 2),
                (1024, 32, 7, 1),
                (256, 8, 56, 1), (512, 16, 56, 2), (512, 16, 28, 1),
                (1024, 32, 28, 2), (1024, 32, 14, 1)]


def bench_gconv(n=128, passes=3, dtype="bf16"):
    """Narrow-group 3x3 conv fwd / dgrad / wgrad through functional.conv2d:
    the LDS-tiled MFMA route next to the implicit-GEMM path
    (DISTRIBUUUU_GCONV_TILE=0; w = 4 packs 2:1 there), alternated over
    `passes` passes in one session. GB/s is against each pass's minimum
    traffic: both activations once, the weight left out. dtype "fp32" runs
    the exact-fp32 family (gconv_f32_route) the same way."""
    import os

    from distribuuuu_amd.ops import functional as DF

    f32 = dtype == "fp32"
    route_of = e.gconv_f32_route if f32 else e.gconv_route
    print(f"== grouped 3x3 conv {dtype}, tile vs igemm, ResNeXt at N={n} "
          "(us per call; GB/s of minimum traffic) ==")
    saved = os.environ.pop("DISTRIBUUUU_GCONV_TILE", None)
    try:
        for c, w, h, s in GCONV_SHAPES:
            g, ho = c // w, (h - 1) // s + 1
            bf = dict(device=DEV,
                      dtype=torch.float32 if f32 else torch.bfloat16)
            x = _cl(torch.randn(n, c, h, h, **bf)).requires_grad_()
            wt = _cl(torch.randn(c, w, 3, 3, **bf) * 0.1).requires_grad_()
            gy = _cl(torch.randn(n, c, ho, ho, **bf))
            io = (x.numel() + gy.numel()) * x.element_size()
            conv = lambda a, b: DF.conv2d(  # noqa: E731
                a, b, None, (s, s), (1, 1), (1, 1), g)
            # one autograd graph per route and pass: a backward runs the
            # gradient of every input that requires one
            yd, yw = {}, {}
            for knob in ("1", "0"):
                os.environ["DISTRIBUUUU_GCONV_TILE"] = knob
                yd[knob] = conv(x, wt.detach())
                yw[knob] = conv(x.detach(), wt)
            os.environ.pop("DISTRIBUUUU_GCONV_TILE")

            def fwd(_knob):
                with torch.no_grad():
                    conv(x, wt)

            ops = (("fwd", fwd),
                   ("dgrad", lambda k: torch.autograd.grad(
                       yd[k], x, gy, retain_graph=True)),
                   ("wgrad", lambda k: torch.autograd.grad(
                       yw[k], wt, gy, retain_graph=True)))
            for name, fn in ops:
                route = route_of(x, c, g, 3, 3, s, s, 1, 1, 1, 1, name)
                rows = {"1": [], "0": []}
                for _ in range(passes):
                    for knob in ("1", "0"):
                        os.environ["DISTRIBUUUU_GCONV_TILE"] = knob
                        rows[knob].append(timeit(lambda: fn(knob),
                                                 iters=50, warmup=5))
                os.environ.pop("DISTRIBUUUU_GCONV_TILE")
                fmt = lambda v: " ".join(  # noqa: E731
                    f"{t*1e6:7.1f}" for t in v)
                best = {k: min(v) for k, v in rows.items()}
                verdict = "keep" if max(rows["1"]) < min(rows["0"]) else "LOSES"
                print(f"C={c:4d} w={w:2d} {h:3d}x{h:<3d} s{s} {name:5s} "
                      f"tile {fmt(rows['1'])} ({io/best['1']/1e9:5.0f} GB/s)"
                      f" | igemm {fmt(rows['0'])} "
                      f"({io/best['0']/1e9:5.0f} GB/s) | {verdict} {route[1:]}")
            del x, gy, yd, yw
    finally:
        if saved is not None:
            os.environ["DISTRIBUUUU_GCONV_TILE"] = saved


# densenet121's dense blocks: (layers, C0, H); growth 32, bn_size 4
DENSE_BLOCKS = [(6, 64, 56), (12, 128, 28), (24, 256, 14), (16, 512, 7)]


def bench_dense(n=128, passes=3):
    """One dense block forward + backward in eager mode: the slab route next
    to the concat path (DISTRIBUUUU_DENSE_SLAB=0), alternated over `passes`
    passes in one session, on densenet121's four blocks at N=128."""
    import os

    from distribuuuu_amd.models.densenet import _DenseBlock

    print(f"== dense block fwd+bwd, slab vs concat, densenet121 at N={n} "
          "(us per block) ==")
    saved = os.environ.pop("DISTRIBUUUU_DENSE_SLAB", None)
    try:
        for layers, c0, h in DENSE_BLOCKS:
            torch.manual_seed(0)
            block = _DenseBlock(layers, c0, 4, 32, 0.0).to(DEV).to(
                torch.bfloat16).to(memory_format=torch.channels_last)
            for m in block.modules():
                if hasattr(m, "running_mean"):
                    m.float()
            x = _cl(torch.randn(n, c0, h, h, device=DEV,
                                dtype=torch.bfloat16)).requires_grad_()
            gout = _cl(torch.randn(n, c0 + 32 * layers, h, h, device=DEV,
                                   dtype=torch.bfloat16))
            params = [x] + list(block.parameters())

            def step():
                # the slab route accumulates into the output gradient
                torch.autograd.grad(block(x), params, gout.clone())

            rows = {"1": [], "0": []}
            for _ in range(passes):
                for knob in ("1", "0"):
                    os.environ["DISTRIBUUUU_DENSE_SLAB"] = knob
                    rows[knob].append(timeit(step, iters=20, warmup=5) * 1e6)
            os.environ.pop("DISTRIBUUUU_DENSE_SLAB")
            fmt = lambda v: " ".join(f"{t:8.1f}" for t in v)  # noqa: E731
            print(f"L={layers:2d} C0={c0:3d} {h:2d}x{h:<2d}  slab "
                  f"{fmt(rows['1'])}   concat {fmt(rows['0'])}   "
                  f"best {min(rows['1']) / min(rows['0']):.3f}x")
            del block, x, gout, params
    finally:
        if saved is not None:
            os.environ["DISTRIBUUUU_DENSE_SLAB"] = saved


def bench_fp32(n=128, passes=3):
    """fp32 conv fwd / dgrad / wgrad on ResNet-50's distinct shapes at batch
    n: the 3xBF16 split kernels (ops.set_fp32_precision("high")) next to the
    exact fp32 MFMA kernels ("highest"), alternated over `passes` passes in
    one session. A (shape, pass) keeps the split route only if its slowest
    "high" pass beats the fastest "highest" pass."""
    from distribuuuu_amd import ops

    print(f"== fp32 conv, split (high) vs exact (highest), ResNet-50 at N={n}"
          " (us per call; TF/s of the best pass) ==")
    was = ops.get_fp32_precision()
    tot = {"high": 0.0, "highest": 0.0}
    try:
        for (nn, c, h, w_, k, r, s, p), calls in _resnet50_wgrad_shapes(n):
            ho = (h + 2 * p - r) // s + 1
            f32 = dict(device=DEV, dtype=torch.float32)
            x = _cl(torch.randn(nn, c, h, w_, **f32))
            wt = _cl(torch.randn(k, c, r, r, **f32) * 0.1)
            gy = _cl(torch.randn(nn, k, ho, ho, **f32))
            geom = (s, s, p, p, 1, 1, 1)
            flops = 2.0 * nn * ho * ho * k * c * r * r
            fns = (("fwd", lambda: e.conv2d_fwd(x, wt, *geom)),
                   ("dgrad", lambda: e.conv2d_dgrad(gy, wt, h, w_, *geom)),
                   ("wgrad", lambda: e.conv2d_wgrad(gy, x, r, r, *geom)))
            for name, fn in fns:
                rows = {"high": [], "highest": []}
                for _ in range(passes):
                    for mode in rows:
                        ops.set_fp32_precision(mode)
                        rows[mode].append(timeit(fn, iters=10, warmup=3))
                ops.set_fp32_precision("high")
                route = e.fp32_conv_route(c, k, name)
                fmt = lambda v: " ".join(  # noqa: E731
                    f"{t*1e6:8.1f}" for t in v)
                best = {m: min(v) for m, v in rows.items()}
                for m in tot:
                    tot[m] += best[m] * calls
                verdict = ("keep" if max(rows["high"]) < min(rows["highest"])
                           else "LOSES")
                print(f"C={c:4d} K={k:4d} {h:3d}x{h:<3d} {r}x{r} s{s} x{calls} "
                      f"{name:5s} high {fmt(rows['high'])} "
                      f"({flops/best['high']/1e12:5.1f} TF) | highest "
                      f"{fmt(rows['highest'])} "
                      f"({flops/best['highest']/1e12:5.1f} TF) | "
                      f"{best['highest']/best['high']:.2f}x {verdict} {route}")
            del x, wt, gy
        print(f"sum of best x calls per step: high {tot['high']*1e3:.1f} ms, "
              f"highest {tot['highest']*1e3:.1f} ms")
    finally:
        ops.set_fp32_precision(was)


def bench_mhsa_stream(passes=3):
    """Streaming MHSA (csrc/attention_stream.hip) forward + backward next to
    the bf16 torch composition the same call took before, alternated in one
    session: time per call and peak allocated memory above the inputs, at
    heads = 4, D = 128 on a 24x24 map (N = 32) and a 32x32 map (N = 16).
    Two layouts: the dense mhsa_relpos call, and the route MHSA.forward takes,
    mhsa_stream_nhwc on the qkv convs' channels_last outputs, against the
    chunk / transpose / compose / transpose sequence of its fallback."""
    from distribuuuu_amd.ops.attention import (_torch_mhsa, mhsa_relpos,
                                               mhsa_stream_nhwc)

    print("== mhsa_stream fwd+bwd vs bf16 composition (ms, peak MiB) ==")
    for n, hw in ((32, 24), (16, 32)):
        heads, d, l = 4, 128, hw * hw
        sc = d ** -0.5
        bf = dict(device=DEV, dtype=torch.bfloat16)
        q, k, v = (torch.randn(n, heads, l, d, **bf).requires_grad_()
                   for _ in range(3))
        rel_h, rel_w = (torch.randn(2 * hw - 1, d, **bf).mul_(sc)
                        .requires_grad_() for _ in range(2))
        gout = torch.randn(n, heads, l, d, **bf)
        qk4 = _cl(torch.randn(n, 2 * heads * d, hw, hw, **bf)).requires_grad_()
        v4 = _cl(torch.randn(n, heads * d, hw, hw, **bf)).requires_grad_()
        gout4 = _cl(torch.randn(n, heads * d, hw, hw, **bf))

        def stream():
            out = mhsa_relpos(q * sc, k, v, rel_h, rel_w, hw, hw)
            torch.autograd.grad(out, [q, k, v, rel_h, rel_w], gout)

        def composed():
            out = _torch_mhsa(q * sc, k, v, rel_h, rel_w, hw, hw)
            torch.autograd.grad(out, [q, k, v, rel_h, rel_w], gout)

        def stream_nhwc():
            out = mhsa_stream_nhwc(qk4, v4, rel_h, rel_w, heads, d, hw, hw, sc)
            torch.autograd.grad(out, [qk4, v4, rel_h, rel_w], gout4)

        def composed_nhwc():  # MHSA.forward's fallback lines
            q_, k_ = qk4.chunk(2, dim=1)
            q_ = q_.reshape(n, heads, d, l).transpose(2, 3)
            k_ = k_.reshape(n, heads, d, l).transpose(2, 3)
            v_ = v4.reshape(n, heads, d, l).transpose(2, 3)
            out = _torch_mhsa(q_ * sc, k_, v_, rel_h, rel_w, hw, hw)
            out = out.transpose(2, 3).reshape(n, heads * d, hw, hw)
            torch.autograd.grad(out, [qk4, v4, rel_h, rel_w], gout4)

        for tag, pair in (("dense", (("stream", stream),
                                     ("composed", composed))),
                          ("nhwc", (("stream", stream_nhwc),
                                    ("composed", composed_nhwc)))):
            row = {"stream": [], "composed": []}
            peak = {}
            for _ in range(passes):
                for name, fn in pair:
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    row[name].append(timeit(fn, iters=10, warmup=3) * 1e3)
                    peak[name] = ((torch.cuda.max_memory_allocated() - base)
                                  / 2 ** 20)
            fmt = lambda v: " ".join(f"{t:8.2f}" for t in v)  # noqa: E731
            print(f"N={n:3d} {hw}x{hw} heads={heads} D={d} {tag:5s} stream "
                  f"{fmt(row['stream'])} peak {peak['stream']:8.1f}   "
                  f"composition {fmt(row['composed'])} "
                  f"peak {peak['composed']:8.1f}")
        del q, k, v, gout, qk4, v4, gout4


class _Const(torch.nn.Module):
    """Stands in for a conv whose output is already recorded."""

    def __init__(self, t):
        super().__init__()
        self.t = [t]

    def forward(self, x):
        return self.t[0]


def bench_mhsa_f32(passes=3):
    """Exact-fp32 MHSA (csrc/attention_fp32.hip) forward + backward next to
    the fp32 torch composition the same call took before
    (DISTRIBUUUU_MHSA_F32=0), alternated in one session: time per call and
    peak allocated memory above the inputs, at heads = 4, D = 128 on 14x14
    (N = 64), 24x24 (N = 32) and 32x32 (N = 16). Two layouts: the dense
    mhsa_relpos call, and the route MHSA.forward takes (the module's own lines
    from the qkv convs' channels_last outputs on)."""
    import os
    import warnings

    from distribuuuu_amd.models.botnet import MHSA
    from distribuuuu_amd.ops.attention import mhsa_relpos

    print("== mhsa_f32 fwd+bwd vs fp32 composition (ms, peak MiB) ==")
    for n, hw in ((64, 14), (32, 24), (16, 32)):
        heads, d, l = 4, 128, hw * hw
        sc = d ** -0.5
        f32 = dict(device=DEV, dtype=torch.float32)
        q, k, v = (torch.randn(n, heads, l, d, **f32).requires_grad_()
                   for _ in range(3))
        gout = torch.randn(n, heads, l, d, **f32)
        # the module with its two convs replaced by their recorded outputs
        m = MHSA(8, (hw, hw), heads=heads, dim_qk=d, dim_v=d).to(DEV)
        qk4 = _cl(torch.randn(n, 2 * heads * d, hw, hw, **f32)).requires_grad_()
        v4 = _cl(torch.randn(n, heads * d, hw, hw, **f32)).requires_grad_()
        gout4 = _cl(torch.randn(n, heads * d, hw, hw, **f32))
        m.to_qk, m.to_v = _Const(qk4), _Const(v4)
        x0 = torch.empty(n, 8, hw, hw, **f32)

        def dense():
            out = mhsa_relpos(q * sc, k, v, m.rel_h, m.rel_w, hw, hw)
            torch.autograd.grad(out, [q, k, v, m.rel_h, m.rel_w], gout)

        def nhwc():
            torch.autograd.grad(m(x0), [qk4, v4, m.rel_h, m.rel_w], gout4)

        for tag, fn in (("dense", dense), ("nhwc", nhwc)):
            row = {"1": [], "0": []}
            peak = {}
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # the composition warns
                    for _ in range(passes):
                        for on in ("1", "0"):
                            os.environ["DISTRIBUUUU_MHSA_F32"] = on
                            torch.cuda.synchronize()
                            base = torch.cuda.memory_allocated()
                            torch.cuda.reset_peak_memory_stats()
                            row[on].append(timeit(fn, iters=10, warmup=3) * 1e3)
                            peak[on] = ((torch.cuda.max_memory_allocated()
                                         - base) / 2 ** 20)
            finally:
                os.environ.pop("DISTRIBUUUU_MHSA_F32")
            fmt = lambda v: " ".join(f"{t:8.2f}" for t in v)  # noqa: E731
            print(f"N={n:3d} {hw}x{hw} heads={heads} D={d} {tag:5s} kernels "
                  f"{fmt(row['1'])} peak {peak['1']:8.1f}   "
                  f"composition {fmt(row['0'])} peak {peak['0']:8.1f}")
        del q, k, v, gout, qk4, v4, gout4, m


if __name__ == "__main__":
    args = sys.argv[1:]
    deterministic = "--deterministic" in args
    slab_blocks = ()
    for a in args:
        if a.startswith("--slab-blocks="):
            slab_blocks = tuple(int(v) for v in a.split("=")[1].split(","))
    dtype = "bf16"
    for i, a in enumerate(args):
        if a.startswith("--dtype"):  # --dtype fp32 or --dtype=fp32
            dtype = a.split("=")[1] if "=" in a else args.pop(i + 1)
    groups = [a for a in args if not a.startswith("--")] or ["all"]
    if "bn" in groups or "all" in groups:
        bench_bn()
    if "conv" in groups or "all" in groups:
        bench_conv()
    if "wgrad" in groups or "all" in groups:
        bench_wgrad(deterministic, slab_blocks)
    if "pool" in groups or "all" in groups:
        bench_pool()
    if "fused" in groups or "all" in groups:
        bench_fused()
    if "gemm" in groups or "all" in groups:
        bench_gemm()
    if "sgd" in groups or "all" in groups:
        bench_sgd()
    if "mix" in groups or "all" in groups:
        bench_mix()
    if "se" in groups or "all" in groups:
        bench_se()
    if "dw" in groups or "all" in groups:
        bench_dw_f32() if dtype == "fp32" else bench_dw()
    if "gconv" in groups or "all" in groups:
        bench_gconv(dtype=dtype)
    if "dense" in groups or "all" in groups:
        bench_dense()
    if "fp32" in groups or "all" in groups:
        bench_fp32()
    if "mhsa_stream" in groups or "all" in groups:
        bench_mhsa_stream()
    if "mhsa_f32" in groups or "all" in groups:
        bench_mhsa_f32()
