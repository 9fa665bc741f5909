"""Halo-staged 3x3 64->64 conv (conv_halo.hip) against the kernel it replaces.

The new route promises the old one's bits: same MFMA instruction, same
(r, s, c) k-step order per output element, same 256-row partial groups. So
y and the BN partials are compared as integers, NaNs included."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, H, W with C = K = 64
SHAPES = [
    (1, 1, 1),      # smallest
    (1, 3, 5),      # small, several rows
    (2, 7, 7),      # M=98, less than one tile
    (1, 16, 16),    # M=256, exactly one tile
    (5, 8, 8),      # M=320, several images in one tile, tail
    (3, 13, 9),     # M=351, tile crosses an image boundary mid-row
    (2, 56, 56),    # the workload's geometry at N=2: 24.5 tiles
    (1, 2, 300),    # one image row longer than a tile
    (48, 56, 56),   # 588 tiles: more tiles than CUs, so blocks loop over
                    # several tiles and prefetch the next one's input
]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    return require_ext()


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _inputs(n, h, w, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = _cl(torch.randn(n, 64, h, w, device="cuda", dtype=torch.bfloat16,
                        generator=g))
    wt = _cl(torch.randn(64, 64, 3, 3, device="cuda", dtype=torch.bfloat16,
                         generator=g))
    return x, wt


def _bits_equal(a, b):
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view),
                                              b.contiguous().view(view))


def _ref(x, wt):
    return F.conv2d(x.float(), wt.float(), padding=1)


def _assert_close_to_ref(y, x, wt):
    ref = _ref(x, wt)
    err = (y.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err < 2e-2 * max(scale, 1.0), f"err {err} scale {scale}"


def _check_routes_agree(e, x, wt):
    for emit in (False, True):
        old = e.conv2d_fwd_halo_dbg(x, wt, emit, False)
        new = e.conv2d_fwd_halo_dbg(x, wt, emit, True)
        assert len(old) == len(new) == (2 if emit else 1)
        assert _bits_equal(old[0], new[0]), f"y differs (emit={emit})"
        if emit:
            assert new[1].dtype == torch.float32
            assert _bits_equal(old[1], new[1]), "BN partials differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_halo_bit_equal_fwd_and_dgrad(shape):
    e = _ext()
    n, h, w = shape
    x, wt = _inputs(n, h, w)
    if not e.conv3x3_halo_admits(n, h, w):
        # outside the LDS budget: forcing the route is an error, and the
        # dispatcher keeps the old kernel
        with pytest.raises(RuntimeError):
            e.conv2d_fwd_halo_dbg(x, wt, False, True)
        y = e.conv2d_fwd(x, wt, 1, 1, 1, 1, 1, 1, 1)
        assert _bits_equal(y, e.conv2d_fwd_halo_dbg(x, wt, False, False)[0])
        _assert_close_to_ref(y, x, wt)
        return
    _check_routes_agree(e, x, wt)
    # the dgrad of this shape is the same launch with the flipped weight
    _check_routes_agree(e, x, e.weight_flip_t(wt, 1))
    # and the dispatcher takes the new route by itself
    y = e.conv2d_fwd(x, wt, 1, 1, 1, 1, 1, 1, 1)
    assert _bits_equal(y, e.conv2d_fwd_halo_dbg(x, wt, False, True)[0])


def test_halo_gate_admits_the_listed_shapes():
    e = _ext()
    for n, h, w in SHAPES:
        assert e.conv3x3_halo_admits(n, h, w) == ((n, h, w) != (1, 2, 300))
    assert e.conv3x3_halo_admits(256, 56, 56)


def test_halo_padding_is_exact_zero_next_to_inf():
    """+inf in the four corner pixels of every image. A pad pixel in LDS
    that kept an earlier tile's bytes instead of a written zero could hold
    one of these infinities and spoil outputs the old kernel keeps finite;
    the outputs next to the corners are inf/NaN in both and must agree in
    their bits."""
    e = _ext()
    x, wt = _inputs(3, 13, 9, seed=1)
    for hh in (0, -1):
        for ww in (0, -1):
            x[:, :, hh, ww] = float("inf")
    old = e.conv2d_fwd_halo_dbg(x, wt, True, False)
    new = e.conv2d_fwd_halo_dbg(x, wt, True, True)
    assert _bits_equal(old[0], new[0])
    assert _bits_equal(old[1], new[1])
    # pixels whose 3x3 window misses every corner stay finite
    assert torch.isfinite(new[0][:, :, 2:-2, 2:-2].float()).all()


def test_halo_matches_fp32_reference():
    e = _ext()
    x, wt = _inputs(2, 56, 56, seed=2)
    y = e.conv2d_fwd_halo_dbg(x, wt, False, True)[0]
    _assert_close_to_ref(y, x, wt)


_MODULE_SCRIPT = r"""
import sys
import torch
from distribuuuu_amd.ops import modules as M

torch.manual_seed(0)
conv = M.Conv2d(64, 64, 3, padding=1).cuda().to(torch.bfloat16)
bn = M.BatchNorm2d(64, act="relu").cuda().to(torch.bfloat16)
conv = conv.to(memory_format=torch.channels_last)
x = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
gy = torch.randn(2, 64, 14, 14, device="cuda", dtype=torch.bfloat16)
gy = gy.contiguous(memory_format=torch.channels_last)
y = bn(conv(x))
y.backward(gy)
torch.cuda.synchronize()
torch.save({"y": y.detach().cpu(), "gx": x.grad.cpu(),
            "gw": conv.weight.grad.cpu(), "ggamma": bn.weight.grad.cpu(),
            "gbeta": bn.bias.grad.cpu(), "rm": bn.running_mean.cpu(),
            "rv": bn.running_var.cpu()}, sys.argv[1])
"""


def test_halo_knob_modules_fwd_bwd_bit_equal(tmp_path):
    outs = {}
    for knob in ("1", "0"):
        path = tmp_path / f"out{knob}.pt"
        env = dict(os.environ)
        env["DISTRIBUUUU_CONV_HALO"] = knob
        subprocess.run([sys.executable, "-c", _MODULE_SCRIPT, str(path)],
                       cwd=REPO, env=env, check=True, timeout=300)
        outs[knob] = torch.load(path)
    assert outs["1"].keys() == outs["0"].keys()
    for k in outs["1"]:
        assert torch.equal(outs["1"][k], outs["0"][k]), k
