"""The MHSA bounds of mhsa_ref.py, proven on the CPU: a torch emulation that
rounds where the kernels round stays inside every bound at every tile shape,
and the same emulation with a known error class injected (the LDS row-store
clobber, H and W confused in the rel-pos gather) does not. test_mhsa_gpu.py
then holds the kernels themselves to the same bounds."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhsa_ref as R  # noqa: E402

B = 3
_CACHE = {}


def _case(shape, large=False):
    """One case per shape: inputs, fp64 forward reference and the clean
    emulation, computed once and shared (never modified) by the tests."""
    key = (shape, large)
    if key not in _CACHE:
        c = R.make_case(*shape, B=B, seed=R.SHAPES.index(shape) + 100 * large,
                        large=large)
        _CACHE[key] = (c, R.ref_forward(c), R.emulate(c))
    return _CACHE[key]


def _all_ratios(c, ref, em):
    out = R.forward_ratios(c, ref, em)
    out.update(R.backward_ratios(c, em["P"], em))
    return out


_AFFECTED = [s for s in R.SHAPES if R.spill_cols(s[0] * s[1]) > 0]
_NONSQUARE = [s for s in R.SHAPES if s[0] != s[1]]


def test_shape_list_covers_the_affected_lengths():
    # the L ranges whose roundup32(L) < 16*LT: one shape in each, and the
    # square sizes named in the defect report
    ls = {s[0] * s[1] for s in _AFFECTED}
    assert {16, 81, 144, 169} <= ls
    assert any(l <= 32 for l in ls) and any(65 <= l <= 96 for l in ls)
    assert any(129 <= l <= 192 for l in ls) and any(209 <= l <= 224 for l in ls)
    assert all(R.spill_cols(l) == 0 for l in (33, 49, 64, 196, 208, 256))
    assert R.spill_cols(16) == 32 and R.tile_geometry(169) == (13, 192)


def test_rel_index_matches_pad_shift_composition():
    """The brute-force gather maps against ops.attention's pad-shift logits,
    non-square both ways."""
    from distribuuuu_amd.ops.attention import _rel_pos_logits
    for h, w in ((3, 5), (5, 3)):
        torch.manual_seed(0)
        q = torch.randn(2, 1, h * w, 8, dtype=torch.float64)
        rel_h = torch.randn(2 * h - 1, 8, dtype=torch.float64)
        rel_w = torch.randn(2 * w - 1, 8, dtype=torch.float64)
        iw, ih = R.rel_index(h, w)
        mine = (R.gather_rel(q[:, 0] @ rel_w.t(), iw)
                + R.gather_rel(q[:, 0] @ rel_h.t(), ih))
        assert torch.allclose(mine, _rel_pos_logits(q, rel_h, rel_w, h, w)[:, 0],
                              atol=1e-12)


def test_reference_backward_matches_autograd():
    """ref_backward's closed forms against float64 autograd through the
    forward reference's own formulas."""
    c = R.make_case(3, 5, 32, B=2, seed=7)
    q, k, v, dO, rel_h, rel_w = (t.requires_grad_(True) for t in c.f64())
    _, _, S = R._logits64(q, k, rel_h, rel_w, c.scale, c.H, c.W)
    P = torch.softmax(S, -1)
    (P @ v).backward(dO.detach())
    ref, _ = R.ref_backward(c, P.detach())
    for name, t in (("dq", q), ("dk", k), ("dv", v), ("grw", rel_w),
                    ("grh", rel_h)):
        assert torch.allclose(ref[name], t.grad, atol=1e-11), name


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_softmax_spread(shape):
    _, ref, _ = _case(shape)
    med = ref["P"].max(-1).values.median().item()
    print(f"{R.shape_id(shape)}: median row max of P {med:.3f}")
    lo, hi = R.ROWMAX_MEDIAN_RANGE
    assert lo <= med <= hi


@pytest.mark.parametrize("shape", R.LARGE_LOGIT_SHAPES, ids=R.shape_id)
def test_large_logit_inputs(shape):
    _, ref, _ = _case(shape, large=True)
    m = ref["S"].abs().max().item()
    print(f"{R.shape_id(shape)}: max |S| {m:.2f}")
    assert 0.9 * R.LARGE_LOGIT <= m <= 1.1 * R.LARGE_LOGIT


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_emulator_within_bounds(shape):
    c, ref, em = _case(shape)
    ratios = _all_ratios(c, ref, em)
    print(f"{R.shape_id(shape)} emulator err/bound: {R.fmt(ratios)}")
    assert not R.failures(ratios)


@pytest.mark.parametrize("shape", R.LARGE_LOGIT_SHAPES, ids=R.shape_id)
def test_emulator_within_bounds_large_logits(shape):
    c, ref, em = _case(shape, large=True)
    ratios = _all_ratios(c, ref, em)
    print(f"{R.shape_id(shape)} large-logit emulator err/bound: {R.fmt(ratios)}")
    assert not R.failures(ratios)


@pytest.mark.parametrize("shape", _AFFECTED, ids=R.shape_id)
def test_clobber_is_caught(shape):
    """Zeroing the first 16*LT - lpad columns of rows 4, 8, 12 in the LDS
    copies of P and dS must break the O and dQ bounds."""
    c, ref, _ = _case(shape)
    bad = R.emulate(c, clobber=True)
    ratios = _all_ratios(c, ref, bad)
    print(f"{R.shape_id(shape)} clobbered err/bound: {R.fmt(ratios)}")
    failed = R.failures(ratios)
    assert {"O", "O_given_P", "dq"} <= set(failed), failed
    # the global copies come from registers: P, dk and dv stay correct
    assert not {"P", "dk", "dv"} & set(failed), failed


@pytest.mark.parametrize("shape", _NONSQUARE, ids=R.shape_id)
def test_hw_swap_is_caught(shape):
    c, ref, _ = _case(shape)
    bad = R.emulate(c, swap_hw=True)
    ratios = _all_ratios(c, ref, bad)
    print(f"{R.shape_id(shape)} H/W-swapped err/bound: {R.fmt(ratios)}")
    failed = R.failures(ratios)
    assert {"P", "O", "dq"} <= set(failed), failed
    # a one-column table (H or W = 1) gathers the same whichever way
    assert {"grw", "grh"} & set(failed), failed
