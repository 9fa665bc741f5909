"""Throughput of trainer.train_epoch itself, eager and hipGraph-captured.

bench.py times a bare replay loop over one fixed batch; this drives the real
epoch loop (meters, PRINT_FREQ-gated readout, per-step input copy, accuracy
kernel) over a finite DeviceSyntheticLoader, alternating the eager loop and a
graph_step.GraphedTrainStep in one process on one network:

    python tools/trainbench.py --steps 300 --rounds 2

Each timed epoch is a host clock around train_epoch plus a device sync, and
starts after a short untimed epoch in the same mode (for the captured mode
that is where the eager warm-up steps and the capture happen, so the capture
is never inside the timing). The untimed epoch reads its metrics every step
(PRINT_FREQ 1), which drains the device after each step: eager steps whose
gradient pointers still move must not run ahead of the device
(docs/BENCHMARKING.md, "The warm-up sync"); the timed epoch runs at
--print-freq. Like bench.py the default rate is 0: same kernels, weights stay
put. Every round of every mode starts from the seeded weights (restored in
place). Prints one JSON line; `weights_finite` says, per timed epoch, whether
the weights were still finite after it.
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default="resnet50")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--steps", type=int, default=300,
                   help="batches per timed epoch")
    p.add_argument("--rounds", type=int, default=2,
                   help="timed epochs per mode, alternated eager/captured")
    p.add_argument("--prime", type=int, default=6,
                   help="batches of the untimed epoch before each timed one")
    p.add_argument("--lr", type=float, default=0.0)
    p.add_argument("--print-freq", type=int, default=30)
    p.add_argument("--im-size", type=int, default=224)
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars"],
                   help="OPTIM.OPTIMIZER: fused SGD-momentum, or LARS on it")
    p.add_argument("--label-smooth", type=float, default=0.0,
                   help="TRAIN.LABEL_SMOOTH")
    p.add_argument("--mixup-alpha", type=float, default=0.0,
                   help="TRAIN.MIXUP_ALPHA")
    p.add_argument("--cutmix-alpha", type=float, default=0.0,
                   help="TRAIN.CUTMIX_ALPHA")
    p.add_argument("--mix-prob", type=float, default=1.0,
                   help="TRAIN.MIX_PROB")
    p.add_argument("--mix-switch-prob", type=float, default=0.5,
                   help="TRAIN.MIX_SWITCH_PROB")
    p.add_argument("--modes", default="eager,captured",
                   help="comma list; one mode alone is for profiling it")
    return p.parse_args()


def main():
    args = parse_args()
    has_gpu = torch.cuda.is_available()
    device = torch.device("cuda:0" if has_gpu else "cpu")
    if has_gpu:
        torch.cuda.set_device(0)

    from distribuuuu_amd.config import cfg
    from distribuuuu_amd import trainer as T
    from distribuuuu_amd import utils
    from distribuuuu_amd.data import DeviceSyntheticLoader
    from distribuuuu_amd.graph_step import GraphedTrainStep

    use_bf16 = args.dtype == "bf16" and has_gpu
    batch = args.batch if has_gpu else 8
    steps = args.steps if has_gpu else 4
    im_size = args.im_size if has_gpu else 32
    cfg.defrost()
    cfg.MODEL.ARCH = args.arch
    cfg.TRAIN.DTYPE = "bfloat16" if use_bf16 else "float32"
    cfg.TRAIN.CHANNELS_LAST = bool(has_gpu)
    cfg.TRAIN.BATCH_SIZE = batch
    cfg.TRAIN.PRINT_FREQ = args.print_freq
    cfg.OPTIM.BASE_LR = args.lr
    cfg.OPTIM.OPTIMIZER = args.optimizer
    cfg.OPTIM.WARMUP_EPOCHS = 0
    cfg.TRAIN.LABEL_SMOOTH = args.label_smooth
    cfg.TRAIN.MIXUP_ALPHA = args.mixup_alpha
    cfg.TRAIN.CUTMIX_ALPHA = args.cutmix_alpha
    cfg.TRAIN.MIX_PROB = args.mix_prob
    cfg.TRAIN.MIX_SWITCH_PROB = args.mix_switch_prob
    cfg.OUT_DIR = os.environ.get("BENCH_OUT_DIR", "/tmp/bench_out")
    cfg.freeze()

    dtype = torch.bfloat16 if use_bf16 else torch.float32
    torch.manual_seed(1234)
    net = T.build_network(device)
    optimizer = utils.construct_optimizer(net)
    # DF.cross_entropy itself unless a soft-target flag is set
    criterion = T.build_criterion()
    runner = GraphedTrainStep(net, criterion, optimizer,
                              cfg.TRAIN.TOPK, device=device, dtype=dtype)

    # built once, outside every timed window (its batch is drawn on the host)
    loader = DeviceSyntheticLoader(
        batch, im_size=im_size, num_classes=cfg.MODEL.NUM_CLASSES,
        device=device, dtype=dtype, channels_last=bool(has_gpu))

    def epoch(n, graphed, print_freq):
        cfg.defrost()
        cfg.TRAIN.PRINT_FREQ = print_freq
        cfg.freeze()
        loader.length = n
        T.train_epoch(loader, net, criterion, optimizer, 0, device,
                      dtype, graph_step=runner if graphed else None)
        if has_gpu:
            torch.cuda.synchronize()

    live = list(net.parameters()) + list(net.buffers())
    start = [t.detach().clone() for t in live]

    @torch.no_grad()
    def restore():
        """Seeded weights, zero momentum, in place (a captured graph points
        at these tensors): every mode starts each round from the same sane
        state, whatever the epoch before it did to the weights."""
        for t, s0 in zip(live, start):
            t.copy_(s0)
        for p in net.parameters():
            state = optimizer.state.get(p, {})
            if state.get("momentum_buffer") is not None:
                state["momentum_buffer"].zero_()
            if state.get("master") is not None:
                state["master"].copy_(p)

    series = {"eager": [], "captured": []}
    finite = {"eager": [], "captured": []}
    for _ in range(args.rounds):
        for mode in args.modes.split(","):
            graphed = mode == "captured"
            restore()
            epoch(args.prime, graphed, 1)
            t0 = time.perf_counter()
            epoch(steps, graphed, args.print_freq)
            dt = time.perf_counter() - t0
            series[mode].append(round(steps * batch / dt, 1))
            finite[mode].append(all(
                bool(torch.isfinite(p).all()) for p in net.parameters()))

    print(json.dumps({
        "metric": f"images/sec {args.arch} trainer.train_epoch",
        "eager_img_s": series["eager"],
        "captured_img_s": series["captured"],
        "steps_per_epoch": steps,
        "batch": batch,
        "dtype": "bf16" if use_bf16 else "fp32",
        "print_freq": args.print_freq,
        "lr": args.lr,
        "optimizer": args.optimizer,
        "label_smooth": args.label_smooth,
        "mixup_alpha": args.mixup_alpha,
        "cutmix_alpha": args.cutmix_alpha,
        "weights_finite": finite,
        "runner": runner.stats,
    }))


if __name__ == "__main__":
    main()
