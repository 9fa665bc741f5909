"""fp64 reference for HIPLARS, shared by test_lars_cpu.py and
test_lars_gpu.py: the trust ratio evaluated from given squared norms, and a
multi-step trajectory against torch.optim.SGD(weight_decay=0) on fp64 clones
fed q * (g + wd*w), with q read from the optimizer under test.

Tolerance on master and momentum after 4 steps is HIPSGD's (test_optim_gpu):
rtol=1e-5, atol=1e-6. q enters both sides with the same value, so the update
adds one rounding (q*g) to the six of an SGD step.
"""

import math

import torch

TOL = dict(rtol=1e-5, atol=1e-6)
CHUNK = 16384  # elements per kernel block (ops/optim.py _CHUNK)
U = 2.0 ** -24  # fp32 unit roundoff

SHAPES = [(1,), (255,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,),
          (2 * CHUNK + 7,), (64, 32, 3, 3)]
LRS = [0.1, 0.1, 0.02, 0.02]
TRUST = 0.1  # large: a 1% error in q moves the weights by about 1e-4

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


def adapted(shape):
    """1-D sizes viewed as (n, 1), so that LARS adapts them."""
    return shape if len(shape) > 1 else (shape[0], 1)


def trust_fp64(w2, g2, wd, trust_coef, eps, adapt=True):
    """The specification's q from squared norms, in Python floats (fp64)."""
    w2, g2 = float(w2), float(g2)
    if not adapt or not (w2 > 0 and g2 > 0):
        return 1.0
    nw, ng = math.sqrt(w2), math.sqrt(g2)
    return trust_coef * nw / (ng + wd * nw + eps)


def set_grad(p, g):
    if g is not None and g.dtype != p.dtype:
        p.grad_dtype = None  # allow a grad wider than the parameter
    p.grad = g


def make_params(shapes, pdtype, device, seed=0):
    gen = torch.Generator(device=device).manual_seed(seed)
    params = [torch.randn(s, device=device, generator=gen).to(pdtype)
              for s in shapes]
    return params, [p.double().clone() for p in params]


def trajectory(opt, params, refs, gdtype, lrs, late=None, seed=1,
               layout=None):
    """Steps `opt` over `params` (in param_groups order) and an fp64
    torch.optim.SGD over `refs` with the effective gradient built from
    opt.last_trust. `late`: index of a parameter that gets no grad during
    the first two steps. `layout`: applied to each gradient before it is
    installed (same values, other strides). Returns the reference optimizer."""
    g0 = opt.param_groups[0]
    ref = torch.optim.SGD(refs, lr=lrs[0], momentum=g0["momentum"],
                          dampening=g0["dampening"], nesterov=g0["nesterov"],
                          weight_decay=0.0)
    device = params[0].device
    gen = torch.Generator(device=device).manual_seed(seed)
    assert [id(p) for g in opt.param_groups for p in g["params"]] == \
        [id(p) for p in params]
    for step, lr in enumerate(lrs):
        for o in (opt, ref):
            for grp in o.param_groups:
                grp["lr"] = lr
        grads = []
        for i, p in enumerate(params):
            if i == late and step < 2:
                set_grad(p, None)
                grads.append(None)
                continue
            g = torch.randn(p.shape, device=device, generator=gen).to(gdtype)
            set_grad(p, g if layout is None else layout(g))
            grads.append(g)
        opt.step()
        i = 0
        for gi, grp in enumerate(opt.param_groups):
            q = opt.last_trust[gi].double()
            assert q.shape == (len(grp["params"]),)
            for pi in range(len(grp["params"])):
                r, g = refs[i], grads[i]
                if g is None:
                    r.grad = None
                    assert q[pi].item() == 1.0
                else:
                    r.grad = q[pi] * (g.double()
                                      + grp["weight_decay"] * r.detach())
                i += 1
        ref.step()
    return ref


def check(opt, ref, params, refs, momentum):
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
