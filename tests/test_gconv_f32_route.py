"""The fp32 narrow-group conv route (gconv_f32_route, csrc/gconv_route.h).

It only classifies, so it runs on meta tensors without a GPU, and answers
(route, TH, chunk width, chunks, items per block, blocks per chunk, lds_bytes).
"""

import pytest
import torch

LDS_BUDGET = 40 * 1024  # GC_LDS_BUDGET: four blocks per 160 KiB CU
PASSES = ("fwd", "dgrad", "wgrad")

# (N, groups, w, H, W, stride, pad): the grouped 3x3 convs of resnext50_32x4d
# and resnext101_32x8d at batch 128, and shapes of the GPU test
RESNEXT = [(128, 32, w, h, h, s, 1) for w, h, s in
           [(4, 56, 1), (8, 56, 2), (8, 28, 1), (16, 28, 2), (16, 14, 1),
            (32, 14, 2), (32, 7, 1), (8, 56, 1), (16, 56, 2), (32, 28, 2),
            (32, 14, 1)]]
SMALL = [(2, 6, 4, 1, 1, 1, 1), (3, 20, 8, 37, 19, 1, 1),
         (2, 3, 32, 37, 19, 2, 1), (2, 10, 16, 38, 20, 2, 1),
         (2, 5, 8, 20, 20, 1, 0), (2, 3, 16, 21, 21, 2, (1, 0)),
         (60, 5, 32, 17, 33, 1, 1), (2, 3, 32, 9, 13, 2, 1)]


def wgrad_gated(w, s, out):
    """The measured losers (kbench gconv --dtype fp32, N = 128, us, tile
    against conv2d_wgrad): w = 32 stride 2 from a 7x7 output map on (264 / 149
    at 7x7, 593 / 384 at 14x14), w = 16 stride 2 from 28x28 on (1004 / 804),
    w = 32 stride 1 below 14x14 (163 / 147 at 7x7)."""
    return ((w == 32 and s == 2 and out >= 49)
            or (w == 16 and s == 2 and out >= 784)
            or (w == 32 and s == 1 and out < 196))


@pytest.fixture(scope="module")
def e():
    from distribuuuu_amd.ops.dispatch import ext

    e = ext()
    assert e is not None, "HIP extension not importable: build it first"
    return e


def _x(n, c, h, w, dtype=torch.float32):
    return torch.empty(n, c, h, w, device="meta", dtype=dtype,
                       memory_format=torch.channels_last)


def route(e, case, pass_):
    n, g, w, h, wd, s, p = case
    p = p if isinstance(p, tuple) else (p, p)
    return e.gconv_f32_route(_x(n, g * w, h, wd), g * w, g, 3, 3, s, s, *p, 1,
                             1, pass_)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("case", RESNEXT + SMALL, ids=str)
def test_in_range_is_tiled_within_budget(e, case, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_GCONV_TILE", raising=False)
    n, g, w, h, wd, s, p = case
    kind, th, cw, chunks, per, slots, lds = route(e, case, pass_)
    ph, pw = p if isinstance(p, tuple) else (p, p)
    out = ((h + 2 * ph - 3) // s + 1) * ((wd + 2 * pw - 3) // s + 1)
    if pass_ == "wgrad" and wgrad_gated(w, s, out):
        assert kind == "generic"
        return
    assert kind == "tile"
    assert 1 <= th <= 8 and cw in (32, 64) and chunks * cw >= g * w
    assert (chunks - 1) * cw < g * w
    # the BN-partial epilogue needs 8 KiB whatever the patch
    assert 8192 <= lds <= LDS_BUDGET
    assert per >= 1 and 1 <= slots <= (512 if pass_ == "wgrad" else 1024)
    # the knob sends every shape back (read per call)
    monkeypatch.setenv("DISTRIBUUUU_GCONV_TILE", "0")
    assert route(e, case, pass_)[0] == "generic"


@pytest.mark.parametrize("pass_", PASSES)
def test_generic_outside_the_range(e, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_GCONV_TILE", raising=False)
    x = _x(4, 128, 28, 28)
    ok = (x, 128, 16, 3, 3, 1, 1, 1, 1, 1, 1)
    assert e.gconv_f32_route(*ok, pass_)[0] == "tile"
    generic = [
        (_x(4, 128, 28, 28, torch.bfloat16),) + ok[1:],  # bf16
        (x, 128, 2) + ok[3:],  # w = 64
        (x, 256, 16) + ok[3:],  # Cg = 8, Kg = 16
        (x, 128, 16, 5, 5, 1, 1, 1, 1, 1, 1),  # 5x5
        (x, 128, 16, 3, 3, 1, 1, 1, 1, 2, 2),  # dilation 2
        (x, 128, 16, 3, 3, 1, 1, 2, 2, 1, 1),  # pad 2
        (x, 128, 16, 3, 3, 1, 2, 1, 1, 1, 1),  # stride (1, 2)
        (x, 128, 1) + ok[3:],  # groups = 1
        (_x(4, 128, 28, 28).contiguous(),) + ok[1:],  # NCHW
    ]
    for args in generic:
        assert e.gconv_f32_route(*args, pass_)[0] == "generic", args[1:]
