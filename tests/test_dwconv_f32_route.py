"""The fp32 depthwise route (dwconv_f32_route in csrc/dwconv_route.h).

It only classifies: it reads the shape, dtype and layout of x, the geometry,
the pass and DISTRIBUUUU_DW_TILE, launches nothing, and so runs on meta
tensors without a GPU. It answers (route, TH, TW, CB, NB, slots, lds_bytes).
"""

import pytest
import torch

LDS_BUDGET = 40 * 1024  # docs/ARCHITECTURE.md "Depthwise": per-block budget
PASSES = ("fwd", "dgrad", "wgrad")

# EfficientNet-B0's distinct depthwise convs: (C, H, R, stride)
B0 = [(32, 112, 3, 1), (96, 112, 3, 2), (144, 56, 3, 1), (144, 56, 5, 2),
      (240, 28, 5, 1), (240, 28, 3, 2), (480, 14, 3, 1), (480, 14, 5, 1),
      (672, 14, 5, 1), (672, 14, 5, 2), (1152, 7, 5, 1), (1152, 7, 3, 1)]


@pytest.fixture(scope="module")
def e():
    from distribuuuu_amd.ops.dispatch import ext

    e = ext()
    if e is None:
        pytest.skip("HIP extension not importable")
    return e


def _x(n, c, h, w, dtype=torch.float32):
    return torch.empty(n, c, h, w, device="meta", dtype=dtype,
                       memory_format=torch.channels_last)


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("case", B0, ids=lambda c: "-".join(map(str, c)))
def test_b0_shapes_are_tiled(e, case, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_DW_TILE", raising=False)
    c, h, r, s = case
    route, th, tw, cb, nb, slots, lds = e.dwconv_f32_route(
        _x(128, c, h, h), r, r, s, s, r // 2, r // 2, pass_)
    assert route == "tiled"
    assert th >= 1 and tw in (8, 16) and cb % 4 == 0 and 4 <= cb <= 32
    assert nb >= 1
    assert 0 < lds <= LDS_BUDGET
    if pass_ == "wgrad":
        assert 1 <= slots <= 512


@pytest.mark.parametrize("pass_", PASSES)
def test_generic_outside_the_range(e, pass_, monkeypatch):
    monkeypatch.delenv("DISTRIBUUUU_DW_TILE", raising=False)
    x = _x(4, 20, 28, 28)
    assert e.dwconv_f32_route(x, 3, 3, 1, 1, 1, 1, pass_)[0] == "tiled"
    generic = [
        (_x(4, 32, 28, 28, torch.bfloat16), 3, 3, 1, 1, 1, 1),  # bf16
        (_x(4, 18, 28, 28), 3, 3, 1, 1, 1, 1),  # C % 4 != 0
        (x, 7, 7, 1, 1, 3, 3),  # R = 7
        (x, 3, 3, 1, 2, 1, 1),  # stride (1, 2)
        (x, 3, 3, 1, 1, 3, 3),  # pad = R
        (x, 5, 5, 1, 1, 5, 5),
    ]
    for args in generic:
        assert e.dwconv_f32_route(*args, pass_)[0] == "generic", args[1:]
    monkeypatch.setenv("DISTRIBUUUU_DW_TILE", "0")  # read per call
    assert e.dwconv_f32_route(x, 3, 3, 1, 1, 1, 1, pass_)[0] == "generic"
    monkeypatch.setenv("DISTRIBUUUU_DW_TILE", "1")
    assert e.dwconv_f32_route(x, 3, 3, 1, 1, 1, 1, pass_)[0] == "tiled"
