"""Flagship benchmark: ResNet-50 DDP bf16 training step on N MI355X GPUs.

Driver contract: ``python bench.py --gpus N --steps K --warmup W`` (N>1 is
launched by the driver via torch.distributed.run, one rank per GPU over RCCL).
Measures the BASELINE.json metric — images/sec, whole node, synthetic
3x224x224 data, random-init weights, bf16 compute, per-rank batch 256,
SyncBN on RCCL when world_size > 1 — and prints ONE JSON line from rank 0.
The steps run at ``--lr`` (default 0: same kernels, weights stay put, so
outputs repeat run to run). ``--dump-outputs DIR`` also writes what the last
timed step handed back; ``--full`` is where secondary measurements belong (none today).
"""

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--arch", type=str, default="resnet50")
    p.add_argument("--batch", type=int, default=256, help="per-rank batch size")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--syncbn", type=int, default=-1,
                   help="-1: auto (on when world>1), 0/1: force")
    p.add_argument("--graph", type=int, default=-1,
                   help="capture the step in a hipGraph: -1 auto "
                        "(on for 1 GPU), 0/1 force")
    p.add_argument("--lr", type=float, default=0.0,
                   help="SGD learning rate, reported as config.lr. 0 "
                        "(default) runs the whole step but leaves the weights "
                        "at their seeded values, so outputs repeat from run "
                        "to run; 0.2 is the project's base rate")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write what the last step "
                        "handed back (logits, loss, BN/classifier gradients "
                        "and momentum) to DIR/<name>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements; bench.py has "
                        "none beyond the headline figure, so this is "
                        "currently the same as a plain run")
    return p.parse_args()


def _dump_outputs(out_dir, arrays, max_bytes=60 << 20):
    """Write ``arrays`` (name -> tensor) as float32 ``out_dir/<name>.npy``.
    The arrays share ``max_bytes``; one over its share is cut to a fixed,
    seeded sample of its rows (dim 0), kept in order; an array whose single
    row is over the share is flattened and sampled by element."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    share = max_bytes // max(len(arrays), 1)
    for name, t in arrays.items():
        t = t.detach().float().cpu()
        if t.dim() == 0 or 4 * t.shape[1:].numel() > share:
            t = t.reshape(-1)
        max_rows = share // (4 * max(t.shape[1:].numel(), 1))
        if t.shape[0] > max_rows:
            g = torch.Generator(device="cpu").manual_seed(1234)
            rows = torch.randperm(t.shape[0], generator=g)[:max_rows]
            t = t[rows.sort().values]
        np.save(os.path.join(out_dir, name + ".npy"), t.numpy())


def _step_results(net, optimizer, last):
    """What the last step handed back: its return values, and the gradients
    and momentum it left on the parameters that no atomic-add kernel feeds
    (1-D BN/bias parameters and the 2-D classifier weight). Those depend on
    the loss backward, every dgrad and BN-backward kernel and the SGD
    kernel, and are the same from run to run; the conv weight gradients come
    out of fp32 atomics and differ by a bf16 ulp between runs, so they stay
    out of the dump."""
    logits, loss = last
    grads, moms = [], []
    for p in net.parameters():
        if p.dim() > 2 or p.grad is None:
            continue
        grads.append(p.grad.detach().float().reshape(-1))
        buf = optimizer.state.get(p, {}).get("momentum_buffer")
        if buf is not None:
            moms.append(buf.detach().float().reshape(-1))
    arrays = {"logits": logits, "loss": loss}
    if grads:
        arrays["grads_bn_fc"] = torch.cat(grads)
    if moms:
        arrays["momentum_bn_fc"] = torch.cat(moms)
    return arrays


def _self_launch(args):
    """`python bench.py --gpus N` without torchrun must NOT silently measure
    1 GPU: spawn torch.distributed.run ourselves, one rank per GPU."""
    import socket
    import subprocess
    import sys

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(args)
    world_size = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    has_gpu = torch.cuda.is_available()

    if world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29566")
        dist.init_process_group(backend="nccl" if has_gpu else "gloo",
                                rank=rank, world_size=world_size)
    if has_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device(f"cuda:{local_rank}")
    else:
        device = torch.device("cpu")

    from distribuuuu_amd.config import cfg
    from distribuuuu_amd import trainer as T
    from distribuuuu_amd import utils
    from distribuuuu_amd.data import DeviceSyntheticLoader
    from distribuuuu_amd.parallel import DistributedDataParallel
    from distribuuuu_amd.ops import functional as DF

    use_bf16 = args.dtype == "bf16" and has_gpu
    use_syncbn = (world_size > 1) if args.syncbn == -1 else bool(args.syncbn)
    batch = args.batch if has_gpu else 8  # CPU smoke keeps it tiny

    cfg.defrost()
    cfg.MODEL.ARCH = args.arch
    cfg.MODEL.SYNCBN = use_syncbn
    cfg.TRAIN.DTYPE = "bfloat16" if use_bf16 else "float32"
    cfg.TRAIN.CHANNELS_LAST = bool(has_gpu)
    cfg.OUT_DIR = os.environ.get("BENCH_OUT_DIR", "/tmp/bench_out")
    cfg.freeze()

    dtype = torch.bfloat16 if use_bf16 else torch.float32
    # fixed seed: same arguments -> same initial weights (the synthetic batch
    # is seeded by the loader), so two builds can be compared output for output
    torch.manual_seed(1234)
    net = T.build_network(device)
    if world_size > 1:
        net = DistributedDataParallel(net, bucket_cap_mb=cfg.TRAIN.BUCKET_CAP_MB)
    optimizer = utils.construct_optimizer(net)
    # default rate 0: the same kernels run, the weights stay put, and the
    # outputs repeat from run to run (why: docs/BENCHMARKING.md)
    utils.set_lr(optimizer, args.lr)
    net.train()

    loader = DeviceSyntheticLoader(batch, im_size=224, num_classes=1000,
                                   device=device, dtype=dtype,
                                   channels_last=bool(has_gpu))
    it = iter(loader)

    # world==1: set_to_none avoids 161 per-step grad memsets (no DDP bucket
    # views to preserve); DDP needs stable bucket-view grads.
    zero_none = world_size == 1

    def step():
        inputs, targets = next(it)
        outputs = net(inputs)
        loss = DF.cross_entropy(outputs.float(), targets)
        optimizer.zero_grad(set_to_none=zero_none)
        loss.backward()
        optimizer.step()
        return outputs.detach(), loss.detach()

    def untimed_step():
        # With set_to_none the grad pointers move every step, so HIPSGD
        # rewrites its pinned chunk table on the host and copies it to the
        # device asynchronously; a host that runs a step ahead overwrites the
        # table before the previous copy has executed and the update reads
        # wrong pointers (NaN weights from the third step on). Draining the
        # device after each untimed eager step keeps the state that the timed
        # steps start from, and the dumped outputs, well defined.
        step()
        if has_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        untimed_step()

    # hipGraph capture of the whole train step: the inner loop replays one
    # graph instead of ~900 eager launches. Multi-rank too — RCCL collectives
    # (DDP buckets, SyncBN stats) are capture-legal on ROCm, and an
    # eager-launch-bound rank would cap scaling; capture failure falls back
    # to eager below.
    use_graph = bool(has_gpu) if args.graph == -1 else bool(args.graph)
    graph = None
    last = None  # (logits, loss) of the most recent timed step
    if use_graph:
        try:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(2):
                    untimed_step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                last = step()  # static tensors, refilled by every replay
            graph.replay()
            torch.cuda.synchronize()
        except Exception as exc:  # pragma: no cover - fall back to eager
            print(f"[bench] graph capture failed ({exc}); eager mode",
                  flush=True)
            graph = None
        if world_size > 1:
            # every rank must agree (a replaying rank paired with an eager
            # one still matches collective order, but keep it uniform)
            ok = torch.tensor([1.0 if graph is not None else 0.0],
                              device=device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if ok.item() < 1.0:
                graph = None

    if world_size > 1:
        dist.barrier()
    if has_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if graph is not None:
            graph.replay()
        else:
            last = step()
    if has_gpu:
        torch.cuda.synchronize()
    if world_size > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if world_size > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device
                         if has_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    global_batch = batch * world_size
    images_per_sec = args.steps * global_batch / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if args.dump_outputs and rank == 0 and last is not None:
        _dump_outputs(args.dump_outputs, _step_results(net, optimizer, last))

    if rank == 0:
        print(json.dumps({
            "metric": f"images/sec {args.arch} train (whole node)",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_bf16 else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.arch,
                "global_batch": global_batch,
                "seq_len": None,
                "im_size": 224,
                "parallelism": f"dp{world_size}",
                "syncbn": use_syncbn,
                "hipgraph": graph is not None,
                "lr": args.lr,
            },
        }))

    if world_size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
