"""CPU side of the fp32 attention tests: the bounds of test_mhsa_f32_gpu.py
hold for the plain fp32 torch composition and its autograd backward at every
listed shape (so a kernel that misses them is wrong, not the bound), and the
range / switch helpers of the route."""

import pytest
import torch

from distribuuuu_amd.ops import attention as A
from test_mhsa_f32_gpu import SHAPES, _case, _sid, check


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_fp32_composition_stays_inside_the_bounds(shape):
    c, ref, bounds = _case(shape)
    q, k, v, rel_h, rel_w = (t.clone().requires_grad_()
                             for t in (c.q, c.k, c.v, c.rel_h, c.rel_w))
    out = A._torch_mhsa((q * c.scale).unsqueeze(1), k.unsqueeze(1),
                        v.unsqueeze(1), rel_h, rel_w, c.H, c.W)
    out.backward(c.dO.unsqueeze(1))
    got = {"O": out.detach()[:, 0], "dq": q.grad, "dk": k.grad, "dv": v.grad,
           "grw": rel_w.grad, "grh": rel_h.grad}
    check(f"{_sid(shape)}/torch-fp32", got, ref, bounds)


def test_f32_range_and_switch(monkeypatch):
    ok = A.hip_mhsa_f32_supported
    assert all(ok(h, w, d) for h, w in ((1, 1), (17, 3), (14, 14), (32, 32))
               for d in (32, 64, 96, 128))
    assert not any(ok(h, w, d) for h, w, d in (
        (33, 8, 32), (8, 33, 32), (0, 4, 32), (14, 14, 16), (14, 14, 48),
        (14, 14, 160)))
    monkeypatch.delenv("DISTRIBUUUU_MHSA_F32", raising=False)
    on = A.mhsa_f32_enabled
    assert on(196, True) and on(576, True) and not on(1024, True)
    assert on(196, False) and not on(576, False)
    monkeypatch.setenv("DISTRIBUUUU_MHSA_F32", "0")
    assert not on(196, True)
    monkeypatch.setenv("DISTRIBUUUU_MHSA_F32", "1")
    assert on(1024, True) and on(1024, False)
