"""The dgrad route table (csrc/conv_route.h) at default gates.

conv2d_dgrad_route only classifies: it reads shapes and dtypes, launches no
kernel, and so runs on meta tensors without a GPU. The rows pin what
conv2d_dgrad / conv2d_dgrad_prep / conv2d_dgrad_acc decide for every route
(V2_MINK = 192, V2_MINRSC = 512), including the places where the accumulate
gate is deliberately narrower than the plain one.
"""

import os

import pytest
import torch


def _ext():
    from distribuuuu_amd.ops.dispatch import ext

    e = ext()
    if e is None:
        pytest.skip("HIP extension not importable")
    return e


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


# C, K, (R, S), stride, pad, dilation, groups, dtype -> kind, wkind, and
# whether a matching `into` buffer gets the ACC epilogue
BF, FP = torch.bfloat16, torch.float32
ROWS = [
    (512, 512, (3, 3), 1, 1, 1, 1, BF, "V2Same", 1, True),
    (2048, 512, (1, 1), 1, 0, 1, 1, BF, "V2Same", 1, True),
    (512, 512, (3, 3), 1, 0, 1, 1, BF, "V2Same", 1, True),
    (256, 64, (1, 1), 1, 0, 1, 1, BF, "Same", 0, True),
    (64, 64, (3, 3), 1, 1, 1, 1, BF, "Same", 0, True),
    (64, 256, (1, 1), 1, 0, 1, 1, BF, "Same", 0, True),
    (512, 1024, (1, 1), 2, 0, 1, 1, BF, "Strided1x1", 0, True),
    (64, 64, (3, 3), 2, 1, 1, 1, BF, "Parity3x3", 0, True),
    (64, 64, (3, 3), 2, 1, 2, 1, BF, "Dilate", 0, False),
    (8, 64, (7, 7), 2, 3, 1, 1, BF, "Dilate", 0, False),
    # grouped: no ACC epilogue is offered
    (256, 256, (3, 3), 1, 1, 1, 32, BF, "Same", 0, False),
    (696, 696, (3, 3), 1, 1, 1, 3, BF, "V2Same", 1, False),
    # R == 1 with pw > 0: the v2 gate admits it, the accumulate gate does not
    (512, 512, (1, 3), 1, (0, 1), 1, 1, BF, "V2Same", 1, False),
    (512, 512, (3, 3), 1, 1, 1, 1, FP, "Same", 0, False),
]

GATE_VARS = ("CONV_V2", "V2_MINK", "V2_MINRSC", "V2INTO_MINRSC",
             "CONV_V2INTO", "CONV_SMALL", "CONV_HALO")


def _operands(C, K, RS, stride, pad, dil, groups, dtype, H=14, N=2):
    R, S = RS
    ph, pw = _pair(pad)
    ho = (H + 2 * ph - dil * (R - 1) - 1) // stride + 1
    wo = (H + 2 * pw - dil * (S - 1) - 1) // stride + 1
    cl = torch.channels_last
    gy = torch.empty(N, K, ho, wo, device="meta", dtype=dtype,
                     memory_format=cl)
    w = torch.empty(K, C // groups, R, S, device="meta", dtype=dtype,
                    memory_format=cl)
    geom = (gy, w, H, H, stride, stride, ph, pw, dil, dil, groups)
    into = torch.empty(N, C, H, H, device="meta", dtype=dtype,
                       memory_format=cl)
    return geom, into


@pytest.fixture(scope="module")
def e():
    set_ = [v for v in GATE_VARS if "DISTRIBUUUU_" + v in os.environ]
    assert not set_, f"route table is stated for default gates; set: {set_}"
    return _ext()


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(map(str, r[:7])))
def test_dgrad_route_table(e, row):
    *shape, kind, wkind, acc = row
    geom, into = _operands(*shape)
    assert e.conv2d_dgrad_route(*geom) == (kind, wkind, False)
    assert e.conv2d_dgrad_route(*geom, into) == (kind, wkind, acc)


def test_dgrad_route_rejects_unfit_into(e):
    """A buffer that is not exactly gx (shape, dtype, layout) never gets the
    ACC epilogue, on a route that otherwise has one."""
    geom, into = _operands(512, 512, (3, 3), 1, 1, 1, 1, BF)
    assert e.conv2d_dgrad_route(*geom, into) == ("V2Same", 1, True)
    n, c, h, w = into.shape
    cl = torch.channels_last
    unfit = [
        torch.empty(n, c, h + 1, w, device="meta", dtype=BF,
                    memory_format=cl),
        torch.empty(n, c // 2, h, w, device="meta", dtype=BF,
                    memory_format=cl),
        torch.empty(n, c, h, w, device="meta", dtype=FP, memory_format=cl),
        torch.empty(n, c, h, w, device="meta", dtype=BF),  # NCHW strides
    ]
    for bad in unfit:
        assert e.conv2d_dgrad_route(*geom, bad) == ("V2Same", 1, False)
