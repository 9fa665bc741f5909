"""HIPSGD's tensor-op path (`_fallback_step`, taken on CPU and for parameters
the fused kernel cannot address) against torch.optim.SGD run on fp64 clones.

The fp32 state is compared with the fp64 trajectory at rtol=1e-5, atol=1e-6:
each step performs at most 6 roundings of O(1) values, so four steps stay
within tens of fp32 ulps.
"""

import pytest
import torch

from distribuuuu_amd.ops.optim import HIPSGD

TOL = dict(rtol=1e-5, atol=1e-6)

# (id, optimizer kwargs)
CONFIGS = [
    ("nesterov_wd", dict(momentum=0.9, nesterov=True, weight_decay=5e-5)),
    ("momentum", dict(momentum=0.9, weight_decay=0.0)),
    ("dampening", dict(momentum=0.9, dampening=0.5, weight_decay=0.0)),
    ("no_momentum", dict(momentum=0.0, weight_decay=1e-4)),
]

SHAPES = [(7,), (5, 3), (8, 4, 3, 3)]
LRS = [0.1, 0.1, 0.02, 0.02]  # lr changes between steps 2 and 3


def _force_fallback(monkeypatch):
    monkeypatch.setenv("DISTRIBUUUU_FORCE_TORCH", "1")


def _make(dtypes, seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g).to(dt)
              for s, dt in zip(SHAPES, dtypes)]
    refs = [p.double().clone() for p in params]
    return params, refs


def _run(params, refs, groups, ref_groups, kwargs, skip=None, seed=1):
    """4 steps of both optimizers with fresh grads each step; `skip` is the
    index of a parameter whose grad stays None."""
    opt = HIPSGD(groups, lr=LRS[0], **kwargs)
    ref = torch.optim.SGD(ref_groups, lr=LRS[0], **kwargs)
    g = torch.Generator().manual_seed(seed)
    for lr in LRS:
        for o in (opt, ref):
            for grp in o.param_groups:
                grp["lr"] = lr
        for i, (p, r) in enumerate(zip(params, refs)):
            if i == skip:
                continue
            p.grad = torch.randn(p.shape, generator=g).to(p.dtype)
            r.grad = p.grad.double()
        opt.step()
        ref.step()
    return opt, ref


@pytest.mark.parametrize("name,kwargs", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fallback_matches_torch_sgd(monkeypatch, name, kwargs):
    _force_fallback(monkeypatch)
    params, refs = _make([torch.float32] * 3, seed=0)
    opt, ref = _run(params, refs, params, refs, kwargs)
    for p, r in zip(params, refs):
        assert torch.allclose(p.double(), r, **TOL)
        if kwargs["momentum"] != 0:
            assert torch.allclose(
                opt.state[p]["momentum_buffer"].double(),
                ref.state[r]["momentum_buffer"], **TOL)


def test_fallback_two_groups_and_none_grad(monkeypatch):
    """Two param groups with different weight decay; one parameter never gets
    a grad and must stay untouched, without optimizer state."""
    _force_fallback(monkeypatch)
    params, refs = _make([torch.float32] * 3, seed=2)
    before = params[1].clone()
    groups = [dict(params=params[:2], weight_decay=1e-2),
              dict(params=params[2:], weight_decay=0.0)]
    ref_groups = [dict(params=refs[:2], weight_decay=1e-2),
                  dict(params=refs[2:], weight_decay=0.0)]
    opt, _ = _run(params, refs, groups, ref_groups,
                  dict(momentum=0.9, nesterov=True), skip=1)
    assert torch.equal(params[1], before)
    assert "momentum_buffer" not in opt.state[params[1]]
    for p, r in zip(params, refs):
        assert torch.allclose(p.double(), r, **TOL)


@pytest.mark.parametrize("name,kwargs", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fallback_bf16_master(monkeypatch, name, kwargs):
    """A bf16 parameter carries an fp32 master: the master follows the fp64
    trajectory (started from the bf16 values, fed the bf16 grads) and the
    parameter is the master rounded to bf16, bit for bit."""
    _force_fallback(monkeypatch)
    dtypes = [torch.bfloat16, torch.float32, torch.bfloat16]
    params, refs = _make(dtypes, seed=3)
    opt, _ = _run(params, refs, params, refs, kwargs)
    for p, r in zip(params, refs):
        if p.dtype == torch.bfloat16:
            master = opt.state[p]["master"]
            assert master.dtype == torch.float32
            assert torch.allclose(master.double(), r, **TOL)
            assert torch.equal(p, master.to(torch.bfloat16))
        else:
            assert "master" not in opt.state[p]
            assert torch.allclose(p.double(), r, **TOL)


def test_fallback_strided_grad_and_state(monkeypatch):
    """The tensor-op path is stride-aware: a channels_last parameter with a
    contiguous grad (and the converse) matches torch."""
    _force_fallback(monkeypatch)
    g = torch.Generator().manual_seed(4)
    a = torch.randn(8, 4, 3, 3, generator=g).contiguous(
        memory_format=torch.channels_last)
    b = torch.randn(8, 4, 3, 3, generator=g)
    params = [a, b]
    refs = [p.double().clone() for p in params]
    opt = HIPSGD(params, lr=0.1, momentum=0.9, dampening=0.5)
    ref = torch.optim.SGD(refs, lr=0.1, momentum=0.9, dampening=0.5)
    for _ in range(3):
        a.grad = torch.randn(8, 4, 3, 3, generator=g)
        b.grad = torch.randn(8, 4, 3, 3, generator=g).contiguous(
            memory_format=torch.channels_last)
        assert a.grad.stride() != a.stride() and b.grad.stride() != b.stride()
        for p, r in zip(params, refs):
            r.grad = p.grad.double()
        opt.step()
        ref.step()
    for p, r in zip(params, refs):
        assert torch.allclose(p.double(), r, **TOL)


def test_state_dict_round_trip_keeps_fp32_state(monkeypatch):
    """torch's load_state_dict casts state to the parameter's dtype; a bf16
    parameter's fp32 master and momentum must come back bit for bit."""
    _force_fallback(monkeypatch)
    g = torch.Generator().manual_seed(6)
    p = torch.randn(33, generator=g).to(torch.bfloat16)
    opt = HIPSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    for _ in range(2):
        p.grad = torch.randn(33, generator=g).to(torch.bfloat16)
        opt.step()
    want = {k: opt.state[p][k].clone() for k in ("momentum_buffer", "master")}
    # the test is vacuous unless the fp32 state holds more than bf16 can
    assert not torch.equal(want["master"],
                           want["master"].to(torch.bfloat16).float())
    sd = opt.state_dict()
    opt2 = HIPSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    opt2.load_state_dict(sd)
    for k, v in want.items():
        got = opt2.state[p][k]
        assert got.dtype == torch.float32
        assert torch.equal(got, v), k
        assert got.data_ptr() != sd["state"][0][k].data_ptr()
