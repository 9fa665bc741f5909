"""Tutorial ladder smoke tests (the reference's teaching scripts are its
de-facto regression suite — SURVEY.md §4)."""

import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_env():
    """Environment for a child that must take the CPU path (two gloo ranks,
    bit-exact repeats) also where a GPU is visible to the test run."""
    env = dict(os.environ)
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    return env


def test_snsc_golden_transcript():
    """The docstring transcript is a regression oracle (the reference embeds
    expected stdout in every tutorial docstring, e.g. snsc.py:85-114)."""
    from tutorial import snsc

    losses = snsc.main(epochs=3)
    assert len(losses) == len(snsc.EXPECTED_LOSSES)
    for got, want in zip(losses, snsc.EXPECTED_LOSSES):
        assert abs(got - want) < 5e-3, (losses, snsc.EXPECTED_LOSSES)


def test_ddp_launch_tutorial_2proc_gloo_golden():
    from tutorial.mnmc_ddp_launch import EXPECTED_LOSSES

    env = _cpu_env()
    env["MASTER_ADDR"] = "127.0.0.1"
    env["MASTER_PORT"] = "29621"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29621", "tutorial/mnmc_ddp_launch.py"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [float(line.rsplit(" ", 1)[1]) for line in r.stdout.splitlines()
           if " loss " in line]
    assert len(got) == len(EXPECTED_LOSSES), r.stdout
    for g, want in zip(got, EXPECTED_LOSSES):
        assert abs(g - want) < 5e-3, (got, EXPECTED_LOSSES)


def test_imagenet_tutorial_single_proc():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "tutorial/imagenet.py"], cwd=REPO,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "checkpoint round-trip OK" in r.stdout


def test_bench_2proc_gloo():
    """bench.py under torchrun world 2 on CPU (the driver's multi-GPU launch
    shape) — checks the DDP/SyncBN/metric-aggregation path end to end."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29631", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import json

    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2
    assert d["config"]["syncbn"] is True


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes what the last timed step handed back as float32
    .npy, and two runs with the same arguments see identical inputs (seeded
    weights + batch), so on CPU the dumps match bit for bit. Run at a rate
    above 0 so that a lost seed would show in the weights too."""
    import json

    import numpy as np

    env = _cpu_env()
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--arch", "resnet18", "--full", "--lr", "0.05",
             "--dump-outputs", str(out)],
            cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines()
                        if l.startswith("{")][-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        assert d["config"]["lr"] == 0.05
        dumps.append({f: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == ["grads_bn_fc.npy", "logits.npy", "loss.npy",
                         "momentum_bn_fc.npy"]
    assert a["grads_bn_fc.npy"].shape == a["momentum_bn_fc.npy"].shape
    assert np.abs(a["grads_bn_fc.npy"]).max() > 0
    assert a["logits.npy"].dtype == np.float32
    assert a["logits.npy"].shape == (8, 1000)  # CPU run uses batch 8
    assert a["loss.npy"].shape == (1,) and np.isfinite(a["loss.npy"]).all()
    for f in a:
        assert np.array_equal(a[f], b[f]), f


def test_bench_dump_outputs_sampling(tmp_path):
    """An array over its share of the byte cap is cut to a seeded sample of
    its rows, in order and the same every time; smaller ones are whole."""
    import numpy as np
    import torch

    import bench

    big = torch.arange(1000 * 16, dtype=torch.float32).reshape(1000, 16)
    flat = torch.arange(5000, dtype=torch.float64)
    small = torch.tensor(3.5)
    for name in ("a", "b"):
        bench._dump_outputs(str(tmp_path / name),
                            {"big": big, "flat": flat, "small": small},
                            max_bytes=3 * 100 * 16 * 4)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["big.npy", "flat.npy", "small.npy"]
    assert sum(v.nbytes for v in a.values()) <= 3 * 100 * 16 * 4
    assert a["big.npy"].shape == (100, 16) and a["big.npy"].dtype == np.float32
    rows = a["big.npy"][:, 0] / 16
    assert (np.diff(rows) > 0).all() and rows.max() > 100  # ordered, spread
    assert (a["big.npy"] == big.numpy()[rows.astype(int)]).all()
    assert a["flat.npy"].shape == (1600,) and a["flat.npy"].dtype == np.float32
    assert a["small.npy"].tolist() == [3.5]
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    # one row wider than the share is sampled by element; empty stays empty
    wide = torch.arange(2 * 4000, dtype=torch.float32).reshape(2, 4000)
    bench._dump_outputs(str(tmp_path / "c"),
                        {"wide": wide, "none": torch.zeros(0, 8)},
                        max_bytes=2 * 1000 * 4)
    c = np.load(tmp_path / "c" / "wide.npy")
    assert c.shape == (1000,) and (np.diff(c) > 0).all() and c.max() > 4000
    assert np.load(tmp_path / "c" / "none.npy").shape == (0, 8)


@pytest.mark.gpu
def test_bench_dump_outputs_graph_path(tmp_path):
    """On the GPU the timed steps are hipGraph replays and the dump reads the
    capture's static tensors: they must hold one and the same last step, so
    the dumped loss is the cross-entropy of the dumped logits against the
    loader's seeded targets. Bound: fp32 accumulation of the 1000 exp terms
    per row and the 32 per-row atomics, n*eps*|loss| = 1032 * 6e-8 * 7 <
    1e-3; the bf16 logits are exact in float32."""
    import json

    import numpy as np

    from distribuuuu_amd.data import DeviceSyntheticLoader

    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--arch", "resnet18", "--batch", "32",
         "--dump-outputs", str(tmp_path)],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["hipgraph"] is True and d["config"]["lr"] == 0.0
    out = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(out) == ["grads_bn_fc.npy", "logits.npy", "loss.npy",
                           "momentum_bn_fc.npy"]
    for f, v in out.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), f
    assert np.abs(out["grads_bn_fc.npy"]).max() > 0
    assert np.abs(out["momentum_bn_fc.npy"]).max() > 0
    logits = out["logits.npy"].astype(np.float64)
    assert logits.shape == (32, 1000)
    y = DeviceSyntheticLoader(32, device="cpu").y.numpy()
    m = logits.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logits - m).sum(axis=1))
    want = float((lse - logits[np.arange(32), y]).mean())
    print("dumped loss", float(out["loss.npy"][0]), "from logits", want)
    assert abs(float(out["loss.npy"][0]) - want) < 1e-3
