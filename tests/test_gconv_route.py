"""The narrow-group conv route (csrc/gconv_route.h).

gconv_route only classifies: it reads the shape, dtype and layout of x, the
weight's K, the geometry, the pass and DISTRIBUUUU_GCONV_TILE, launches
nothing, and so runs on meta tensors without a GPU. It answers
(route, TH, chunk width, chunks, items per block, blocks per chunk, lds_bytes).
"""

import pytest
import torch

LDS_BUDGET = 40 * 1024  # GC_LDS_BUDGET: four blocks per 160 KiB CU
PASSES = ("fwd", "dgrad", "wgrad")

# (N, groups, w, H, W, stride, pad): the in-range grouped 3x3 convs of
# resnext50_32x4d and resnext101_32x8d at batch 128 ...
RESNEXT = [(128, 32, w, h, h, s, 1) for w, h, s in
           [(4, 56, 1), (8, 56, 2), (8, 28, 1), (16, 28, 2), (16, 14, 1),
            (32, 14, 2), (32, 7, 1), (8, 56, 1), (16, 56, 2), (32, 28, 2),
            (32, 14, 1)]]
# ... and the GPU test's list. Per width: a group count that leaves the last
# 32-channel block half empty, and one that makes C = 160 (three chunks).
GROUPS = {4: (6, 40), 8: (5, 20), 16: (3, 10), 32: (3, 5)}
GPU_CASES = [c for w, (ga, gb) in GROUPS.items() for c in [
    (2, ga, w, 1, 1, 1, 1), (1, ga, w, 2, 3, 2, 1),  # taps mostly halo
    (3, gb, w, 37, 19, 1, 1),  # ragged tiles on both axes
    (2, ga, w, 37, 19, 2, 1), (2, gb, w, 38, 20, 2, 1),  # dgrad parities
    (2, ga, w, 20, 20, 1, 0), (2, ga, w, 21, 21, 2, (1, 0)),  # pads
]]
# More (image, tile) items than blocks, nine tiles per image and a run length
# that does not divide nine: runs wrap tile rows and cross image seams.
RUN_CASES = [(60, 40, 4, 17, 33, 1, 1), (60, 5, 32, 17, 33, 1, 1)]


@pytest.fixture(scope="module")
def e():
    from distribuuuu_amd.ops.dispatch import ext

    e = ext()
    assert e is not None, "HIP extension not importable: build it first"
    return e


def tiles_per_image(case, pass_, th):
    """Tiles of the pass's output map (dgrad: gx) at tile height th."""
    _, _, _, h, wd, s, p = case
    ph, pw = p if isinstance(p, tuple) else (p, p)
    if pass_ != "dgrad":
        h, wd = (h + 2 * ph - 3) // s + 1, (wd + 2 * pw - 3) // s + 1
    return -(-h // th) * -(-wd // 16)


def _x(n, c, h, w, dtype=torch.bfloat16):
    return torch.empty(n, c, h, w, device="meta", dtype=dtype,
                       memory_format=torch.channels_last)


def route(e, case, pass_):
    n, g, w, h, wd, s, p = case
    p = p if isinstance(p, tuple) else (p, p)
    return e.gconv_route(_x(n, g * w, h, wd), g * w, g, 3, 3, s, s, *p, 1, 1,
                         pass_)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("case", RESNEXT + GPU_CASES + RUN_CASES, ids=str)
def test_in_range_is_tiled_within_budget(e, case, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_GCONV_TILE", raising=False)
    n, g, w, h, wd, s, p = case
    kind, th, cw, chunks, per, slots, lds = route(e, case, pass_)
    ph, pw = p if isinstance(p, tuple) else (p, p)
    out = ((h + 2 * ph - 3) // s + 1) * ((wd + 2 * pw - 3) // s + 1)
    if (pass_, w, s) == ("wgrad", 32, 2) and out >= 196:
        # the one measured loser (kbench gconv: 170 us against tr128's 148
        # at 28x28): stride-2 w = 32 wgrad from a 14x14 output map on
        assert kind == "generic"
        return
    assert kind == "tile"
    assert 1 <= th <= 8 and cw in (32, 64) and chunks * cw >= g * w
    assert (chunks - 1) * cw < g * w
    assert 0 < lds <= LDS_BUDGET
    assert per >= 1 and 1 <= slots <= (512 if pass_ == "wgrad" else 1024)
    if pass_ == "wgrad":
        assert th % 2 == 0
    # the knob sends every shape back (read per call)
    monkeypatch.setenv("DISTRIBUUUU_GCONV_TILE", "0")
    assert route(e, case, pass_)[0] == "generic"


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("case", RUN_CASES, ids=str)
def test_run_cases_cross_image_seams(e, case, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_GCONV_TILE", raising=False)
    _, th, _, _, per, slots, _ = route(e, case, pass_)
    tiles = tiles_per_image(case, pass_, th)
    assert tiles == 9  # three tile rows by three tile columns
    assert per > 1 and tiles % per != 0
    assert (slots - 1) * per < case[0] * tiles <= slots * per


@pytest.mark.parametrize("pass_", PASSES)
def test_generic_outside_the_range(e, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_GCONV_TILE", raising=False)
    x = _x(4, 128, 28, 28)
    ok = (x, 128, 16, 3, 3, 1, 1, 1, 1, 1, 1)
    assert e.gconv_route(*ok, pass_)[0] == "tile"
    generic = [
        (_x(4, 128, 28, 28, torch.float32),) + ok[1:],  # fp32
        (x, 128, 2) + ok[3:],  # w = 64
        (x, 256, 16) + ok[3:],  # Cg = 8, Kg = 16
        (x, 128, 16, 5, 5, 1, 1, 1, 1, 1, 1),  # 5x5
        (x, 128, 16, 3, 3, 1, 1, 1, 1, 2, 2),  # dilation 2
        (x, 128, 16, 3, 3, 1, 1, 2, 2, 1, 1),  # pad 2
        (x, 128, 16, 3, 3, 1, 2, 1, 1, 1, 1),  # stride (1, 2)
        (x, 128, 1) + ok[3:],  # groups = 1
        (_x(4, 12, 28, 28), 12, 3) + ok[3:],  # C % 8 != 0
    ]
    for args in generic:
        assert e.gconv_route(*args, pass_)[0] == "generic", args[1:]
