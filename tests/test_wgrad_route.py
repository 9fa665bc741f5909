"""The bf16 wgrad route table (csrc/wgrad_route.h).

conv2d_wgrad_route only classifies: it reads shapes, dtypes, the deterministic
flag and the DISTRIBUUUU_WGRAD_* knobs, launches no kernel, and so runs on meta
tensors without a GPU. It answers (family, csteps, chunks, accumulate mode).

ATOMIC_ROWS is derived by hand from the code this classifier replaced (the
four inline copies in conv2d_wgrad), for ResNet-50's distinct batch-256 wgrad
launches and the cases of tests/test_deterministic_gpu.py::WGRAD_CASES:

* family: ring128 for 1x1 with Kg % 128 == 0, Cg >= 128 and
  ceil(Kg/128) * ceil(RSC/128) * ceil(M/4096) >= 320 (or grouped-deep, or
  forced); else tr128 for Kg >= 128 and RSC >= 128; else the 64x64 tile.
* the 64x64 kernels' chunk is 64 k-steps of 64 pixels: chunks = ceil(M/4096).
* tr128 / ring128 halve csteps from 64 down to the floor of 8 while
  tiles * chunks * groups < 512, tiles = ceil(Kg/128) * ceil(RSC/128).
  E.g. 3x3 256 at 14x14: M = 50176, tiles = 2 * 18 = 36; csteps 64 gives
  13 chunks = 468 blocks < 512, csteps 32 gives 25 chunks = 900: (32, 25).
  3x3 512 at 7x7: M = 12544, tiles = 4 * 36 = 144, 4 chunks = 576: (64, 4).
"""

import os

import pytest
import torch

BF = torch.bfloat16
KNOBS = ("WGRAD_RING", "WGRAD_128", "WGRAD_T128", "WGRAD_ACC",
         "WGRAD_SLAB_BLOCKS")
WS_CAP = 64 << 20


def _ext():
    from distribuuuu_amd.ops.dispatch import ext

    e = ext()
    if e is None:
        pytest.skip("HIP extension not importable")
    return e


@pytest.fixture(scope="module")
def e():
    set_ = [v for v in KNOBS if "DISTRIBUUUU_" + v in os.environ]
    assert not set_, f"route table is stated for default gates; set: {set_}"
    return _ext()


@pytest.fixture(autouse=True)
def _mode_off_after():
    """The deterministic flag is process-global: leave it off."""
    yield
    e = _ext()
    e.set_deterministic(False)


def _operands(case):
    n, c, h, w, k, r, s, p, g = case
    ho = (h + 2 * p - r) // s + 1
    wo = (w + 2 * p - r) // s + 1
    cl = torch.channels_last
    x = torch.empty(n, c, h, w, device="meta", dtype=BF, memory_format=cl)
    gy = torch.empty(n, k, ho, wo, device="meta", dtype=BF, memory_format=cl)
    return (gy, x, r, r, s, s, p, p, 1, 1, g)


def _slot_bytes(case):
    n, c, h, w, k, r, s, p, g = case
    return k * r * r * (c // g) * 4


# (N, C, H, W, K, R, stride, pad, groups), env -> family, csteps, chunks with
# the accumulate mode forced to atomic
ATOMIC_ROWS = [
    # ResNet-50 at batch 256, in network order (the stem's C is padded to 8)
    ((256, 8, 224, 224, 64, 7, 2, 3, 1), {}, "64x64", 64, 784),
    ((256, 64, 56, 56, 64, 1, 1, 0, 1), {}, "64x64", 64, 196),
    ((256, 64, 56, 56, 64, 3, 1, 1, 1), {}, "64x64", 64, 196),
    ((256, 64, 56, 56, 256, 1, 1, 0, 1), {}, "64x64", 64, 196),
    ((256, 256, 56, 56, 64, 1, 1, 0, 1), {}, "64x64", 64, 196),
    ((256, 256, 56, 56, 128, 1, 1, 0, 1), {}, "ring128", 32, 392),
    ((256, 128, 56, 56, 128, 3, 2, 1, 1), {}, "tr128", 32, 98),
    ((256, 128, 28, 28, 512, 1, 1, 0, 1), {}, "tr128", 16, 196),
    ((256, 256, 56, 56, 512, 1, 2, 0, 1), {}, "ring128", 32, 98),
    ((256, 512, 28, 28, 128, 1, 1, 0, 1), {}, "tr128", 16, 196),
    ((256, 128, 28, 28, 128, 3, 1, 1, 1), {}, "tr128", 32, 98),
    ((256, 512, 28, 28, 256, 1, 1, 0, 1), {}, "ring128", 32, 98),
    ((256, 256, 28, 28, 256, 3, 2, 1, 1), {}, "tr128", 32, 25),
    ((256, 256, 14, 14, 1024, 1, 1, 0, 1), {}, "tr128", 16, 49),
    ((256, 512, 28, 28, 1024, 1, 2, 0, 1), {}, "ring128", 32, 25),
    ((256, 1024, 14, 14, 256, 1, 1, 0, 1), {}, "tr128", 16, 49),
    ((256, 256, 14, 14, 256, 3, 1, 1, 1), {}, "tr128", 32, 25),
    ((256, 1024, 14, 14, 512, 1, 1, 0, 1), {}, "ring128", 32, 25),
    ((256, 512, 14, 14, 512, 3, 2, 1, 1), {}, "tr128", 64, 4),
    ((256, 512, 7, 7, 2048, 1, 1, 0, 1), {}, "tr128", 16, 13),
    ((256, 1024, 14, 14, 2048, 1, 2, 0, 1), {}, "ring128", 64, 4),
    ((256, 2048, 7, 7, 512, 1, 1, 0, 1), {}, "tr128", 16, 13),
    ((256, 512, 7, 7, 512, 3, 1, 1, 1), {}, "tr128", 64, 4),
    # WGRAD_CASES of tests/test_deterministic_gpu.py
    ((4, 64, 64, 64, 64, 3, 1, 1, 1), {}, "64x64", 64, 4),
    ((4, 128, 64, 64, 64, 3, 1, 1, 1), {}, "64x64", 64, 4),
    ((5, 64, 45, 37, 72, 3, 1, 1, 1), {}, "64x64", 64, 3),
    ((4, 64, 64, 64, 64, 3, 1, 1, 4), {}, "64x64", 64, 4),
    ((4, 128, 32, 32, 128, 3, 1, 1, 1), {}, "tr128", 8, 8),
    ((8, 464, 16, 16, 464, 3, 1, 1, 2), {"DISTRIBUUUU_WGRAD_128": "1"},
     "ring128", 8, 4),
    ((4, 64, 64, 64, 64, 3, 1, 1, 1), {"DISTRIBUUUU_WGRAD_RING": "1"},
     "ring", 64, 4),
    # the family knobs turned off
    ((256, 256, 56, 56, 512, 1, 2, 0, 1), {"DISTRIBUUUU_WGRAD_128": "0"},
     "tr128", 32, 98),
    ((256, 512, 7, 7, 512, 3, 1, 1, 1), {"DISTRIBUUUU_WGRAD_T128": "0"},
     "64x64", 64, 4),
]


def _row_id(row):
    return "-".join(map(str, row[0])) + "".join(
        f"-{k[11:]}={v}" for k, v in row[1].items())


@pytest.mark.parametrize("row", ATOMIC_ROWS, ids=_row_id)
def test_atomic_parity(e, row, monkeypatch):
    case, env, family, csteps, chunks = row
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", "atomic")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert e.conv2d_wgrad_route(*_operands(case)) == (
        family, csteps, chunks, "atomic")


# ResNet-50 at batch 256 under WGRAD_ACC=slab: csteps, chunks (the shrink loop
# stops at 384 blocks instead of 512), and whether the default gates pick slab
# by themselves. None: over the workspace cap, atomic whatever the knob says.
RESNET50_SLAB = {
    (256, 8, 224, 224, 64, 7, 2, 3, 1): None,
    (256, 64, 56, 56, 64, 1, 1, 0, 1): (64, 196, False),
    (256, 64, 56, 56, 64, 3, 1, 1, 1): (64, 196, False),
    (256, 64, 56, 56, 256, 1, 1, 0, 1): (64, 196, False),
    (256, 256, 56, 56, 64, 1, 1, 0, 1): (64, 196, False),
    (256, 256, 56, 56, 128, 1, 1, 0, 1): (64, 196, True),
    (256, 128, 56, 56, 128, 3, 2, 1, 1): (64, 49, True),
    (256, 128, 28, 28, 512, 1, 1, 0, 1): (32, 98, True),
    (256, 256, 56, 56, 512, 1, 2, 0, 1): (64, 49, True),
    (256, 512, 28, 28, 128, 1, 1, 0, 1): (32, 98, True),
    (256, 128, 28, 28, 128, 3, 1, 1, 1): (64, 49, True),
    (256, 512, 28, 28, 256, 1, 1, 0, 1): (64, 49, True),
    (256, 256, 28, 28, 256, 3, 2, 1, 1): (64, 13, True),
    (256, 256, 14, 14, 1024, 1, 1, 0, 1): (32, 25, True),
    (256, 512, 28, 28, 1024, 1, 2, 0, 1): (64, 13, True),
    (256, 1024, 14, 14, 256, 1, 1, 0, 1): (32, 25, True),
    (256, 256, 14, 14, 256, 3, 1, 1, 1): (64, 13, True),
    (256, 1024, 14, 14, 512, 1, 1, 0, 1): (64, 13, True),
    (256, 512, 14, 14, 512, 3, 2, 1, 1): (64, 4, True),
    (256, 512, 7, 7, 2048, 1, 1, 0, 1): (32, 7, True),
    (256, 1024, 14, 14, 2048, 1, 2, 0, 1): (64, 4, True),
    (256, 2048, 7, 7, 512, 1, 1, 0, 1): (32, 7, True),
    (256, 512, 7, 7, 512, 3, 1, 1, 1): (64, 4, True),
}


@pytest.mark.parametrize("row", ATOMIC_ROWS[:23], ids=_row_id)
def test_chosen_modes(e, row, monkeypatch):
    """Default gates: slab where the alternated kbench sweep measured it
    faster than the atomic chain in every pass (docs/ARCHITECTURE.md status
    entry 14): every tr128 / ring128 launch; the 64x64 tile stays atomic.
    A launch that is not routed keeps the atomic table's csteps and chunks."""
    case, env, family, csteps, chunks = row
    slab = RESNET50_SLAB[case]
    want = (family, csteps, chunks, "atomic")
    if slab and slab[2]:
        want = (family, slab[0], slab[1], "slab")
    assert e.conv2d_wgrad_route(*_operands(case)) == want
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", "auto")
    assert e.conv2d_wgrad_route(*_operands(case)) == want


@pytest.mark.parametrize("row", ATOMIC_ROWS[:23], ids=_row_id)
def test_forced_slab(e, row, monkeypatch):
    """WGRAD_ACC=slab keeps the family; csteps follows the slab block target,
    and WGRAD_SLAB_BLOCKS=512 restores the atomic table's csteps and chunks,
    which are deterministic mode's as long as the workspace fits."""
    case, env, family, csteps, chunks = row
    slab = RESNET50_SLAB[case]
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", "slab")
    want = (family, csteps, chunks, "atomic")
    if slab:
        want = (family, slab[0], slab[1], "slab")
        assert slab[1] * _slot_bytes(case) <= WS_CAP
    assert e.conv2d_wgrad_route(*_operands(case)) == want
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_SLAB_BLOCKS", "512")
    fits = chunks * _slot_bytes(case) <= WS_CAP
    assert e.conv2d_wgrad_route(*_operands(case)) == (
        family, csteps, chunks, "slab" if fits else "atomic")


@pytest.mark.parametrize("row", ATOMIC_ROWS[23:30], ids=_row_id)
def test_forced_slab_small_cases(e, row, monkeypatch):
    """The small cases sit at the csteps floor (or on a fixed-chunk kernel):
    forcing slab changes the accumulate mode and nothing else."""
    case, env, family, csteps, chunks = row
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", "slab")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert e.conv2d_wgrad_route(*_operands(case)) == (
        family, csteps, chunks, "slab")


def test_workspace_cap_keeps_atomic(e, monkeypatch):
    """tests/test_deterministic_gpu.py::GROW_CASE: 8 chunks of 9.4 MB slots
    are 75.5 MB > 64 MiB. The default mode does not grow csteps: the launch
    keeps (64, 8) and the atomic accumulator, also when slab is forced. The
    stem (784 chunks x 98 KB = 75 MB) is over the cap on the 64x64 kernel."""
    grow = (32, 512, 32, 32, 512, 3, 1, 1, 1)
    stem = (256, 8, 224, 224, 64, 7, 2, 3, 1)
    assert 8 * _slot_bytes(grow) > WS_CAP
    assert 784 * _slot_bytes(stem) > WS_CAP
    for acc in (None, "auto", "slab", "atomic"):
        if acc is None:
            monkeypatch.delenv("DISTRIBUUUU_WGRAD_ACC", raising=False)
        else:
            monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", acc)
        assert e.conv2d_wgrad_route(*_operands(grow)) == (
            "tr128", 64, 8, "atomic")
        assert e.conv2d_wgrad_route(*_operands(stem)) == (
            "64x64", 64, 784, "atomic")
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_128", "1")
    assert e.conv2d_wgrad_route(*_operands(grow)) == (
        "ring128", 64, 8, "atomic")


@pytest.mark.parametrize("acc", [None, "auto", "atomic", "slab"])
def test_deterministic_mode_ignores_the_knob(e, acc, monkeypatch):
    """Deterministic mode: slots + ordered reduction on every launch, the
    family / csteps / chunks of the atomic table, except that tr128 / ring128
    double csteps until the workspace fits the cap (GROW_CASE: 128, 4)."""
    if acc is None:
        monkeypatch.delenv("DISTRIBUUUU_WGRAD_ACC", raising=False)
    else:
        monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", acc)
    e.set_deterministic(True)
    try:
        for case, env, family, csteps, chunks in ATOMIC_ROWS:
            if env:
                continue
            got = e.conv2d_wgrad_route(*_operands(case))
            assert got == (family, csteps, chunks, "slab"), case
        grow = (32, 512, 32, 32, 512, 3, 1, 1, 1)
        assert e.conv2d_wgrad_route(*_operands(grow)) == (
            "tr128", 128, 4, "slab")
        monkeypatch.setenv("DISTRIBUUUU_WGRAD_128", "1")
        assert e.conv2d_wgrad_route(*_operands(grow)) == (
            "ring128", 128, 4, "slab")
    finally:
        e.set_deterministic(False)


def test_unknown_mode_is_an_error(e, monkeypatch):
    monkeypatch.setenv("DISTRIBUUUU_WGRAD_ACC", "bogus")
    with pytest.raises(RuntimeError, match="WGRAD_ACC"):
        e.conv2d_wgrad_route(*_operands((4, 128, 32, 32, 128, 3, 1, 1, 1)))


def test_fp32_is_not_classified(e):
    """The fp32 path (conv_fp32.hip) has its own accumulator and no route."""
    gy, x, *rest = _operands((4, 32, 32, 32, 32, 3, 1, 1, 1))
    with pytest.raises(RuntimeError, match="bf16"):
        e.conv2d_wgrad_route(gy.float(), x.float(), *rest)
