"""HIPSGD's fused multi-tensor kernel against torch.optim.SGD on fp64 clones.

The fp32 state (parameter or master, momentum) must follow the fp64
trajectory within rtol=1e-5, atol=1e-6 after 4 steps: each step performs at
most 6 roundings of O(1) values, so this is tens of fp32 ulps. A bf16
parameter must be its fp32 master rounded to bf16, bit for bit.
"""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-6)
CHUNK = 16384  # elements per kernel block (ops/optim.py _CHUNK)

# chunk edges + a conv weight
SHAPES = [(1,), (255,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,),
          (2 * CHUNK + 7,), (64, 32, 3, 3)]
LRS = [0.1, 0.1, 0.02, 0.02]  # lr changes between steps 2 and 3

CONFIGS = [
    ("nesterov_wd", dict(momentum=0.9, nesterov=True, weight_decay=5e-5)),
    ("momentum", dict(momentum=0.9, weight_decay=0.0)),
    ("dampening", dict(momentum=0.9, dampening=0.5, weight_decay=0.0)),
    ("no_momentum", dict(momentum=0.0, weight_decay=1e-4)),
]

# (param dtype, grad dtype)
DTYPES = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
          (torch.bfloat16, torch.float32)]
DTYPE_IDS = ["fp32", "bf16", "bf16_fp32grad"]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _hipsgd(*a, **k):
    from distribuuuu_amd.ops.optim import HIPSGD
    from distribuuuu_amd.ops.dispatch import hip_op_available

    _ext()
    assert hip_op_available("sgd_step")
    return HIPSGD(*a, **k)


def _set_grad(p, g):
    if g.dtype != p.dtype:
        p.grad_dtype = None  # allow a grad wider than the parameter
    p.grad = g


def _check(opt, ref, params, refs, momentum):
    for p, r in zip(params, refs):
        st = opt.state.get(p, {})
        if p.dtype == torch.bfloat16 and "momentum_buffer" in st:
            master = st["master"]
            assert master.dtype == torch.float32
            assert torch.allclose(master.double(), r, **TOL), p.shape
            assert torch.equal(p, master.to(torch.bfloat16)), p.shape
        else:
            assert torch.allclose(p.double(), r, **TOL), p.shape
        if momentum != 0 and r in ref.state:
            assert torch.allclose(st["momentum_buffer"].double(),
                                  ref.state[r]["momentum_buffer"],
                                  **TOL), p.shape


def _steps(opt, ref, params, refs, gdtype, lrs, skip=None, seed=1):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    for lr in lrs:
        for o in (opt, ref):
            for grp in o.param_groups:
                grp["lr"] = lr
        for i, (p, r) in enumerate(zip(params, refs)):
            if i == skip:
                continue
            g = torch.randn(p.shape, device="cuda", generator=gen).to(gdtype)
            _set_grad(p, g)
            r.grad = g.double()
        opt.step()
        ref.step()


def _params(pdtype, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.randn(s, device="cuda", generator=gen).to(pdtype)
              for s in SHAPES]
    return params, [p.double().clone() for p in params]


@pytest.mark.parametrize("pdtype,gdtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name,kwargs", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fused_sgd_matches_torch_fp64(name, kwargs, pdtype, gdtype):
    params, refs = _params(pdtype)
    opt = _hipsgd(params, lr=LRS[0], **kwargs)
    ref = torch.optim.SGD(refs, lr=LRS[0], **kwargs)
    _steps(opt, ref, params, refs, gdtype, LRS)
    _check(opt, ref, params, refs, kwargs["momentum"])


@pytest.mark.parametrize("pdtype,gdtype", DTYPES, ids=DTYPE_IDS)
def test_fused_sgd_two_groups_and_none_grad(pdtype, gdtype):
    """Two groups with different weight decay (two kernel launches, two
    tables); one parameter never gets a grad and must stay untouched."""
    params, refs = _params(pdtype, seed=2)
    before = params[3].clone()
    kw = dict(momentum=0.9, nesterov=True)
    opt = _hipsgd([dict(params=params[:4], weight_decay=1e-2),
                   dict(params=params[4:], weight_decay=0.0)],
                  lr=LRS[0], **kw)
    ref = torch.optim.SGD([dict(params=refs[:4], weight_decay=1e-2),
                           dict(params=refs[4:], weight_decay=0.0)],
                          lr=LRS[0], **kw)
    _steps(opt, ref, params, refs, gdtype, LRS, skip=3)
    assert torch.equal(params[3], before)
    assert "momentum_buffer" not in opt.state.get(params[3], {})
    _check(opt, ref, params, refs, 0.9)


def test_dampening_late_parameter():
    """A parameter that first receives a grad at step 3 gets its own
    un-dampened first step then, while the others are already dampened."""
    params, refs = _params(torch.float32, seed=5)
    params, refs = params[:3], refs[:3]
    kw = dict(momentum=0.9, dampening=0.5)
    opt = _hipsgd(params, lr=0.1, **kw)
    ref = torch.optim.SGD(refs, lr=0.1, **kw)
    _steps(opt, ref, params, refs, torch.float32, LRS[:2], skip=1)
    _steps(opt, ref, params, refs, torch.float32, LRS[2:], seed=7)
    _check(opt, ref, params, refs, 0.9)


# ---------------------------------------------------------------------------
# layouts: the kernel indexes grad, param, momentum and master by ONE linear
# storage offset, so a tensor with other strides must never reach it as-is
# ---------------------------------------------------------------------------
def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _layout_run(p, make_grad, kw, steps=3, mutate=None):
    r = p.detach().double().contiguous().clone()
    opt = _hipsgd([p], lr=0.1, **kw)
    ref = torch.optim.SGD([r], lr=0.1, **kw)
    gen = torch.Generator(device="cuda").manual_seed(11)
    for step in range(steps):
        g = torch.randn(p.shape, device="cuda", generator=gen).to(p.dtype)
        make_grad(p, g)
        assert torch.equal(p.grad, g)
        r.grad = g.double()
        if mutate is not None and step == 1:
            mutate(opt)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt.step()
        ref.step()
    _check(opt, ref, [p], [r], kw["momentum"])


KW_LAYOUT = [dict(momentum=0.9, nesterov=True, weight_decay=5e-5),
             dict(momentum=0.9, dampening=0.5, weight_decay=0.0)]


@pytest.mark.parametrize("kw", KW_LAYOUT, ids=["nesterov_wd", "dampening"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_channels_last_param_with_flat_buffer_grad(dtype, kw):
    """channels_last parameter whose .grad is a contiguous-strided view of a
    flat bucket buffer (`view_as`, as a DDP bucket that ignores the memory
    format would install it)."""
    torch.manual_seed(0)
    p = _cl(torch.randn(16, 8, 3, 3, device="cuda").to(dtype))
    buffer = torch.zeros(p.numel() + 64, dtype=dtype, device="cuda")
    view = buffer[32:32 + p.numel()].view_as(p)
    assert view.stride() != p.stride()

    def make_grad(p_, g):
        view.copy_(g)
        p_.grad = view

    _layout_run(p, make_grad, kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_ddp_style_grad_view_takes_param_strides(dtype):
    """The view our DDP installs (`as_strided` with the parameter's strides
    on the flat buffer) is addressed correctly by the fused kernel and needs
    no out-of-kernel update."""
    from distribuuuu_amd.ops.optim import HIPSGD

    torch.manual_seed(0)
    p = _cl(torch.randn(16, 8, 3, 3, device="cuda").to(dtype))
    buffer = torch.zeros(p.numel() + 64, dtype=dtype, device="cuda")
    view = buffer[32:32 + p.numel()].as_strided(p.size(), p.stride())

    def make_grad(p_, g):
        view.copy_(g)
        p_.grad = view

    HIPSGD._warned_layout = False
    _layout_run(p, make_grad, KW_LAYOUT[0])
    assert not HIPSGD._warned_layout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_contiguous_param_with_channels_last_grad(dtype):
    torch.manual_seed(0)
    p = torch.randn(16, 8, 3, 3, device="cuda").to(dtype)

    def make_grad(p_, g):
        p_.grad = _cl(g)
        assert p_.grad.stride() != p_.stride()

    _layout_run(p, make_grad, KW_LAYOUT[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_load_state_dict_with_restrided_momentum(dtype):
    """After step 1 the state is round-tripped through load_state_dict with
    the momentum buffer (and master) in the OTHER memory format."""
    torch.manual_seed(0)
    p = _cl(torch.randn(16, 8, 3, 3, device="cuda").to(dtype))

    def make_grad(p_, g):
        p_.grad = _cl(g)

    def mutate(opt):
        sd = opt.state_dict()
        for st in sd["state"].values():
            for k in ("momentum_buffer", "master"):
                if k in st:
                    st[k] = st[k].contiguous().clone()  # NCHW strides
                    assert st[k].stride() != p.stride()
        opt.load_state_dict(sd)

    _layout_run(p, make_grad, KW_LAYOUT[0], mutate=mutate)


def test_host_resident_params_take_tensor_path():
    """A model left on the host, on a machine where the extension is loaded:
    the step must not hand host pointers to the kernel."""
    gen = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=gen) for s in [(5,), (8, 4, 3, 3)]]
    refs = [p.double().clone() for p in params]
    kw = dict(momentum=0.9, dampening=0.5, weight_decay=5e-5)
    opt = _hipsgd(params, lr=0.1, **kw)
    ref = torch.optim.SGD(refs, lr=0.1, **kw)
    for _ in range(3):
        for p, r in zip(params, refs):
            p.grad = torch.randn(p.shape, generator=gen)
            r.grad = p.grad.double()
        opt.step()
        ref.step()
    _check(opt, ref, params, refs, 0.9)
