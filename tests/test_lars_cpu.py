"""HIPLARS without a GPU: config and factory, the tensor-op path against the
fp64 reference of lars_ref.py, and state_dict round trips."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as R  # noqa: E402

from distribuuuu_amd import models, utils  # noqa: E402
from distribuuuu_amd.config import cfg  # noqa: E402
from distribuuuu_amd.ops import functional as DF  # noqa: E402
from distribuuuu_amd.ops.optim import HIPLARS, HIPSGD  # noqa: E402

CPU = torch.device("cpu")


def _lars(params, **kw):
    # fused=False: the tensor-op path also where a GPU and the extension exist
    return HIPLARS(params, fused=False, **kw)


# ---------------------------------------------------------------------------
# config and factory
# ---------------------------------------------------------------------------
def test_config_defaults_and_overrides():
    assert cfg.OPTIM.OPTIMIZER == "sgd"
    assert cfg.OPTIM.LARS_TRUST_COEF == 0.001
    assert cfg.OPTIM.LARS_EPS == 1e-8
    cfg.merge_from_list(["OPTIM.OPTIMIZER", "lars", "OPTIM.LARS_TRUST_COEF",
                         0.02, "OPTIM.LARS_EPS", 1e-6])
    assert cfg.OPTIM.OPTIMIZER == "lars"
    assert cfg.OPTIM.LARS_TRUST_COEF == 0.02
    assert cfg.OPTIM.LARS_EPS == 1e-6


def test_reference_presets_still_load():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in sorted(os.listdir(os.path.join(root, "config"))):
        cfg.merge_from_file(os.path.join(root, "config", name))
        assert cfg.OPTIM.OPTIMIZER == "sgd", name


def test_construct_optimizer_by_name():
    net = models.build_model("resnet18", num_classes=10)
    opt = utils.construct_optimizer(net)
    want = HIPSGD if torch.cuda.is_available() else torch.optim.SGD
    assert type(opt) is want
    assert "trust_coef" not in opt.param_groups[0]

    cfg.OPTIM.OPTIMIZER = "lars"
    cfg.OPTIM.LARS_TRUST_COEF = 0.02
    cfg.OPTIM.LARS_EPS = 1e-6
    cfg.OPTIM.FUSED_SGD = False
    opt = utils.construct_optimizer(net)
    assert type(opt) is HIPLARS and isinstance(opt, HIPSGD)
    assert not opt._fused
    g = opt.param_groups[0]
    assert (g["trust_coef"], g["eps"]) == (0.02, 1e-6)
    assert (g["lr"], g["momentum"], g["weight_decay"], g["dampening"],
            g["nesterov"]) == (cfg.OPTIM.BASE_LR, cfg.OPTIM.MOMENTUM,
                               cfg.OPTIM.WEIGHT_DECAY, cfg.OPTIM.DAMPENING,
                               cfg.OPTIM.NESTEROV)
    cfg.OPTIM.FUSED_SGD = True
    assert utils.construct_optimizer(net)._fused

    cfg.OPTIM.OPTIMIZER = "adam"
    with pytest.raises(ValueError, match="OPTIM.OPTIMIZER"):
        utils.construct_optimizer(net)


def test_constructor_rejects_negative_knobs():
    p = [torch.zeros(2, 2)]
    with pytest.raises(ValueError):
        HIPLARS(p, lr=0.1, trust_coef=-1.0)
    with pytest.raises(ValueError):
        HIPLARS(p, lr=0.1, eps=-1.0)


# ---------------------------------------------------------------------------
# tensor-op path against fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pdtype,gdtype", R.DTYPES, ids=R.DTYPE_IDS)
@pytest.mark.parametrize("name,kwargs", R.CONFIGS,
                         ids=[c[0] for c in R.CONFIGS])
def test_tensor_path_matches_fp64(name, kwargs, pdtype, gdtype):
    shapes = [R.adapted(s) for s in R.SHAPES] + [(7,)]  # (7,): not adapted
    params, refs = R.make_params(shapes, pdtype, CPU)
    opt = _lars(params, lr=R.LRS[0], trust_coef=R.TRUST, **kwargs)
    late = 1 if name == "dampening" else None
    ref = R.trajectory(opt, params, refs, gdtype, R.LRS, late=late)
    R.check(opt, ref, params, refs, kwargs["momentum"])
    q = opt.last_trust[0]
    assert q.dtype == torch.float32 and q.shape == (len(params),)
    assert q[-1].item() == 1.0
    assert all(v > 0 and v != 1.0 for v in q[:-1].tolist()), q
    # q against the formula in fp64, from the published norms
    sq = opt.last_sqnorms[0]
    assert sq.dtype == torch.float32 and sq.shape == (len(params), 2)
    wd = kwargs["weight_decay"]
    for i, p in enumerate(params[:-1]):
        want = R.trust_fp64(sq[i, 0], sq[i, 1], wd, R.TRUST, 1e-8)
        assert abs(q[i].item() - want) <= 8 * R.U * want, p.shape


def test_trust_is_one_where_lars_does_not_apply():
    torch.manual_seed(0)
    w = [torch.randn(33), torch.zeros(4, 5), torch.randn(4, 5),
         torch.randn(4, 5), torch.randn(6, 2)]
    g = [torch.randn(33), torch.randn(4, 5), torch.zeros(4, 5), None,
         torch.randn(6, 2)]
    before = [t.clone() for t in w]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2)
    sgd_w = [t.clone() for t in w]
    opt, sgd = _lars(w, trust_coef=R.TRUST, **kw), HIPSGD(sgd_w, **kw)
    for p, s, grad in zip(w, sgd_w, g):
        p.grad = grad
        s.grad = None if grad is None else grad.clone()
    opt.step()
    sgd.step()
    q = opt.last_trust[0].tolist()
    assert q[:4] == [1.0, 1.0, 1.0, 1.0] and 0 < q[4] < 1, q
    # 1-D, zero weight, zero grad: exactly HIPSGD's update
    for i in range(3):
        assert torch.equal(w[i], sgd_w[i]), i
    assert torch.equal(w[3], before[3]) and not opt.state.get(w[3])
    assert not torch.equal(w[4], sgd_w[4])
    assert opt.last_sqnorms[0][3].tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------
# state_dict
# ---------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, (list, tuple)):
        return all(_plain(x) for x in v)
    return v is None or isinstance(v, (bool, int, float, str))


def _toy(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) for s in [(12, 3), (5,), (4, 2, 3, 3)]]


def _grads(params, step):
    gen = torch.Generator().manual_seed(100 + step)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen)


KW = dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-3)


def test_state_dict_groups_are_plain_values():
    params = _toy()
    opt = _lars(params, trust_coef=0.05, eps=1e-6, **KW)
    _grads(params, 0)
    opt.step()
    sd = opt.state_dict()
    for group in sd["param_groups"]:
        bad = {k: type(v) for k, v in group.items() if not _plain(v)}
        assert not bad, bad
        assert group["trust_coef"] == 0.05 and group["eps"] == 1e-6
    for group in opt.param_groups:
        assert not [k for k in group if k.startswith("_hip")]


def test_save_load_resume_is_bit_identical():
    a = _toy()
    opt_a = _lars(a, trust_coef=0.05, **KW)
    for step in range(4):
        _grads(a, step)
        opt_a.step()

    b = _toy()
    opt_b = _lars(b, trust_coef=0.05, **KW)
    for step in range(2):
        _grads(b, step)
        opt_b.step()
    sd = opt_b.state_dict()
    c = [p.clone() for p in b]
    opt_c = _lars(c, trust_coef=0.05, **KW)
    gen = opt_c.generation
    opt_c.load_state_dict(sd)
    assert opt_c.generation == gen + 1
    for step in range(2, 4):
        _grads(c, step)
        opt_c.step()
    for pa, pc in zip(a, c):
        assert torch.equal(pa, pc)
        assert torch.equal(opt_a.state[pa]["momentum_buffer"],
                           opt_c.state[pc]["momentum_buffer"])
    assert torch.equal(opt_a.last_trust[0], opt_c.last_trust[0])


def test_torch_sgd_state_dict_loads_with_constructor_knobs():
    a = _toy()
    sgd = torch.optim.SGD(a, **KW)
    _grads(a, 0)
    sgd.step()
    sd = sgd.state_dict()
    assert "trust_coef" not in sd["param_groups"][0]

    b = [p.clone() for p in a]
    opt = _lars(b, trust_coef=0.05, eps=1e-6, **KW)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["trust_coef"], g["eps"]) == (0.05, 1e-6)
    refs = [p.double().clone() for p in b]
    mom = [sgd.state[p]["momentum_buffer"].double().clone() for p in a]
    _grads(b, 1)
    opt.step()
    q = opt.last_trust[0].double()
    assert q[1].item() == 1.0 and 0 < q[0].item() < 1
    # the loaded momentum is in use (no first-step seeding), q is applied
    for i, (p, r, m) in enumerate(zip(b, refs, mom)):
        ge = q[i] * (p.grad.double() + KW["weight_decay"] * r)
        m = KW["momentum"] * m + (1 - KW["dampening"]) * ge
        assert torch.allclose(p.double(), r - KW["lr"] * m, **R.TOL)


# ---------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------
def test_train_epoch_with_lars(tmp_path):
    from distribuuuu_amd import trainer
    from distribuuuu_amd.data import construct_train_loader
    import distribuuuu_amd.data as data_mod

    cfg.OUT_DIR = str(tmp_path)
    cfg.MODEL.DUMMY_INPUT = True
    cfg.MODEL.NUM_CLASSES = 10
    cfg.TRAIN.BATCH_SIZE = 4
    cfg.TRAIN.IM_SIZE = 32
    cfg.TRAIN.WORKERS = 0
    cfg.TRAIN.PRINT_FREQ = 2
    cfg.OPTIM.OPTIMIZER = "lars"
    orig = data_mod.DummyDataset
    data_mod.DummyDataset = lambda size=(3, 32, 32), length=1000: orig(size, 8)
    try:
        loader = construct_train_loader()
        assert len(loader) == 2
        torch.manual_seed(0)
        net = models.build_model("resnet18", num_classes=10)
        before = [p.detach().clone() for p in net.parameters()]
        opt = utils.construct_optimizer(net)
        assert type(opt) is HIPLARS
        trainer.train_epoch(loader, net, DF.cross_entropy, opt, 0, CPU,
                            torch.float32)
    finally:
        data_mod.DummyDataset = orig
    after = list(net.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    assert all(not torch.equal(a, b) for a, b in zip(after, before)
               if a.ndim > 1)
    q = opt.last_trust[0]
    assert q.shape == (len(after),)
    assert all((v == 1.0) == (p.ndim <= 1) for v, p in zip(q.tolist(), after))
