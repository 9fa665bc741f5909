"""Per-kernel micro-benchmarks on representative ResNet-50 shapes.

Usage (on a GPU box): python tools/kbench.py [--deterministic] [group ...]
Groups: bn conv wgrad pool fused gemm sgd mix all
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


if __name__ == "__main__":
    args = sys.argv[1:]
    deterministic = "--deterministic" in args
    slab_blocks = ()
    for a in args:
        if a.startswith("--slab-blocks="):
            slab_blocks = tuple(int(v) for v in a.split("=")[1].split(","))
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
