"""Accumulate modes of the bf16 split-m wgrad (csrc/wgrad_route.h).

The oracle is exact. A slab launch is the deterministic mode's kernel
instantiation and reduction at the same csteps, so for every case, with
DISTRIBUUUU_WGRAD_ACC=slab in the default (non-deterministic) mode:

* the result is torch.equal to the deterministic-mode result of the same
  call, five times in a row;
* it has the dtype, shape and strides of the atomic result;
* it is within 3e-2 * max(scale, 1) of fp32 ATen, the bound
  tests/test_deterministic_gpu.py uses for the same kernels.

Every case has at least three chunks per output element (two partials commute
and would prove nothing); the chunk counts follow from the split-m constants
(64x64 chunk 4096 px, tr128 / ring128 floor of 8 k-steps = 512 px) and are
asserted through conv2d_wgrad_route. The stride-2 shape
(4, 128, 32, 32, 128, 3, 2, 1, 1) has 4 * 16 * 16 = 1024 output pixels, two
chunks only; it is kept, and the same geometry at N = 8 (four chunks) is the
stride-2 case that meets the three-chunk rule.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPEATS = 5
ACC = "DISTRIBUUUU_WGRAD_ACC"


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


@pytest.fixture(autouse=True)
def _mode_off_after():
    """The deterministic flag is process-global: leave it off."""
    from distribuuuu_amd import ops

    ops.set_deterministic(False)
    yield
    ops.set_deterministic(False)


def _inputs(case, seed):
    n, c, h, w_, k, r, s, p, g = case
    torch.manual_seed(seed)
    x = _cl(torch.randn(n, c, h, w_, device="cuda", dtype=torch.bfloat16))
    ho = (h + 2 * p - r) // s + 1
    wo = (w_ + 2 * p - r) // s + 1
    gy = _cl(torch.randn(n, k, ho, wo, device="cuda", dtype=torch.bfloat16))
    return x, gy


def _args(case, x, gy):
    n, c, h, w_, k, r, s, p, g = case
    return (gy, x, r, r, s, s, p, p, 1, 1, g)


def _det(e, args):
    from distribuuuu_amd import ops

    ops.set_deterministic(True)
    try:
        return e.conv2d_wgrad(*args)
    finally:
        ops.set_deterministic(False)


def _aten(case, x, gy):
    n, c, h, w_, k, r, s, p, g = case
    wf = torch.zeros(k, c // g, r, r, device="cuda", requires_grad=True)
    F.conv2d(x.float(), wf, None, s, p, 1, g).backward(gy.float())
    return wf.grad.detach()


def _assert_same_layout(got, default):
    assert got.dtype == default.dtype
    assert got.shape == default.shape
    assert got.stride() == default.stride()
    for fmt in (torch.contiguous_format, torch.channels_last):
        assert (got.is_contiguous(memory_format=fmt)
                == default.is_contiguous(memory_format=fmt))


# (N, C, H, W, K, R, stride, pad, groups), env to force the family,
# family, chunks, minimum chunks the case must have
CASES = [
    pytest.param((4, 128, 32, 32, 128, 3, 1, 1, 1), {}, "tr128", 8, 3,
                 id="tr128-plain"),
    # K tail of 8 rows in the second k-tile, RSC = 648 with an 8-column tail
    # in the sixth n-tile, M = 2185: the fifth chunk holds 137 of 512 pixels
    pytest.param((5, 72, 19, 23, 136, 3, 1, 1, 1), {}, "tr128", 5, 3,
                 id="tr128-tails-ragged-m"),
    pytest.param((4, 128, 32, 32, 128, 3, 2, 1, 1), {}, "tr128", 2, 2,
                 id="tr128-stride2-two-chunks"),
    pytest.param((8, 128, 32, 32, 128, 3, 2, 1, 1), {}, "tr128", 4, 3,
                 id="tr128-stride2"),
    pytest.param((4, 144, 32, 32, 256, 3, 1, 1, 2), {}, "tr128", 8, 3,
                 id="tr128-grouped"),
    pytest.param((8, 464, 16, 16, 464, 3, 1, 1, 2),
                 {"DISTRIBUUUU_WGRAD_128": "1"}, "ring128", 4, 3,
                 id="ring128-kg-tail"),
    pytest.param((4, 64, 64, 64, 64, 3, 1, 1, 1), {}, "64x64", 4, 3,
                 id="64x64-xcd-grid"),
    pytest.param((5, 64, 45, 37, 72, 3, 1, 1, 1), {}, "64x64", 3, 3,
                 id="64x64-ragged"),
]


@pytest.mark.parametrize("case,env,family,chunks,min_chunks", CASES)
def test_slab_equals_deterministic(case, env, family, chunks, min_chunks,
                                   monkeypatch):
    e = _ext()
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    x, gy = _inputs(case, 5)
    args = _args(case, x, gy)

    monkeypatch.setenv(ACC, "atomic")
    assert e.conv2d_wgrad_route(*args)[0::2] == (family, chunks)
    assert chunks >= min_chunks
    atomic = e.conv2d_wgrad(*args)
    want = _det(e, args)

    monkeypatch.setenv(ACC, "slab")
    assert e.conv2d_wgrad_route(*args)[0::2] == (family, chunks)
    assert e.conv2d_wgrad_route(*args)[3] == "slab"
    outs = [e.conv2d_wgrad(*args) for _ in range(REPEATS)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert torch.equal(o, want), (
            f"call {i} differs from deterministic mode in "
            f"{(o != want).sum().item()} elements")
    _assert_same_layout(outs[0], atomic)

    ref = _aten(case, x, gy)
    scale = ref.abs().max().item()
    for name, got in (("slab", outs[0]), ("atomic", atomic)):
        err = (got.float() - ref).abs().max().item()
        print(f"wgrad {name} {case}: err {err} scale {scale}")
        assert err < 3e-2 * max(scale, 1.0), f"{name} {case}: err {err}"


def test_slab_more_blocks_than_resident():
    """36 tiles x 16 chunks = 576 blocks of 256 threads and 66 KB of LDS, more
    than the 256 CUs hold at once, so the order in which a tile's chunks
    finish is not fixed. Ten calls on two alternating input pairs of one
    shape (the allocator hands every call the same workspace, still holding
    the other pair's partials): each result equals the deterministic result
    for its input."""
    import os

    e = _ext()
    case = (8, 256, 32, 32, 256, 3, 1, 1, 1)
    pairs = [_inputs(case, seed) for seed in (3, 4)]
    argv = [_args(case, x, gy) for x, gy in pairs]
    saved = os.environ.get(ACC)
    try:
        os.environ[ACC] = "slab"
        assert e.conv2d_wgrad_route(*argv[0]) == ("tr128", 8, 16, "slab")
        want = [_det(e, a) for a in argv]
        assert not torch.equal(want[0], want[1])
        outs = [e.conv2d_wgrad(*argv[i % 2]) for i in range(10)]
        torch.cuda.synchronize()
    finally:
        if saved is None:
            del os.environ[ACC]
        else:
            os.environ[ACC] = saved
    for i, o in enumerate(outs):
        assert torch.equal(o, want[i % 2]), f"call {i}"
    for (x, gy), w in zip(pairs, want):
        ref = _aten(case, x, gy)
        err = (w.float() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"wgrad {case}: err {err} scale {scale}")
        assert err < 3e-2 * max(scale, 1.0)


# tr128, 36 tiles x 8 chunks of 2.36 MB slots: slab at default gates
CAPTURED_CASE = (4, 256, 32, 32, 256, 3, 1, 1, 1)


def test_captured_default_gates():
    """One tr128 launch that the classifier routes to slab by itself, captured
    on one stream and replayed three times with the static inputs refilled:
    every replay equals the eager deterministic result for those inputs."""
    import os

    e = _ext()
    assert ACC not in os.environ
    case = CAPTURED_CASE
    x, gy = _inputs(case, 7)
    args = _args(case, x, gy)
    assert e.conv2d_wgrad_route(*args) == ("tr128", 8, 8, "slab")
    e.conv2d_wgrad(*args)  # eager warm-up: allocations and lazy inits
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = e.conv2d_wgrad(*args)
    for seed in (8, 9, 10):
        x2, gy2 = _inputs(case, seed)
        x.copy_(x2)
        gy.copy_(gy2)
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = _det(e, _args(case, x2, gy2))
        assert torch.equal(got, want), (
            f"replay with seed {seed} differs in "
            f"{(got != want).sum().item()} elements")
        ref = _aten(case, x2, gy2)
        err = (got.float() - ref).abs().max().item()
        assert err < 3e-2 * max(ref.abs().max().item(), 1.0)
