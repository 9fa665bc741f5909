"""HIPLARS's fused step (csrc/lars.hip) on the GPU.

1. squared norms of integer-valued data are exact (any dropped, doubled or
   misattributed element changes an integer below 2^24);
2. squared norms of random data against fp64 sums of the same stored values:
   relative error <= (n+1) * 2^-24, which holds for any order of n-1
   additions of once-rounded squares;
3. the trust ratio q against the formula in fp64, from the kernel's own
   published norms (<= 8 * 2^-24: two square roots, a multiply-add, an add, a
   multiply, a divide) and from fp64 norms (<= (2(n+1) + 8) * 2^-24);
4. a four-step trajectory against fp64 (lars_ref.py);
5. the paths agree: 1-D-only groups with HIPSGD, device rate with launch
   argument, fused with tensor ops, one run with the next;
6. layouts: two groups, grads at odd element offsets, a channels_last grad;
7. a captured resnet18 step against the eager loop, bit for bit.

Tests 2 and 3 print their worst error/bound ratio (pytest -s).
"""

import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = R.CHUNK
ADAPTED = [R.adapted(s) for s in R.SHAPES]
BIG = (257 * CHUNK + 3, 1)  # more chunks than the combine block has threads
DTYPES = pytest.mark.parametrize("pdtype,gdtype", R.DTYPES, ids=R.DTYPE_IDS)


def _lars(*a, **k):
    from distribuuuu_amd.ops.dispatch import hip_op_available, require_ext
    from distribuuuu_amd.ops.optim import HIPLARS

    assert require_ext() is not None, "HIP extension must be built"
    assert hip_op_available("lars_step") and hip_op_available("lars_step_dev")
    return HIPLARS(*a, **k)


def _signs(shape, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 2, shape, device="cuda", generator=gen) * 2.0 - 1.0


def _step_once(ws, gs, **kw):
    """One lr=0 step (the norms are taken before the update anyway)."""
    for w, g in zip(ws, gs):
        R.set_grad(w, g)
    kw.setdefault("momentum", 0.9)
    opt = _lars(ws, lr=0.0, **kw)
    opt.step()
    torch.cuda.synchronize()
    return opt


# ---------------------------------------------------------------------------
# 1. exact sums
# ---------------------------------------------------------------------------
@DTYPES
def test_sqnorms_of_signs_are_exact(pdtype, gdtype):
    shapes = ADAPTED + [BIG]
    ws = [_signs(s, i).to(pdtype) for i, s in enumerate(shapes)]
    gs = [(2.0 * _signs(s, 100 + i)).to(gdtype)
          for i, s in enumerate(ADAPTED)]
    big = _signs(BIG, 200)
    big[-5:] = 0
    gs.append(big.to(gdtype))
    opt = _step_once(ws, gs)
    got = opt.last_sqnorms[0].tolist()
    want = [[float(w.numel()), 4.0 * w.numel()] for w in ws[:-1]]
    want.append([float(ws[-1].numel()), float(ws[-1].numel() - 5)])
    assert got == want
    assert opt.last_sqnorms[0].dtype == torch.float32


@DTYPES
def test_sqnorms_of_marked_elements_are_exact(pdtype, gdtype):
    def marked(shape, dtype):
        t = torch.zeros(shape, device="cuda")
        flat, n = t.view(-1), t.numel()
        for idx, v in ((0, 1.0), (CHUNK - 1, 2.0), (CHUNK, 4.0), (n - 1, 8.0)):
            if idx < n:
                flat[idx] = v
        return t.to(dtype)

    ws = [marked(s, pdtype) for s in ADAPTED]
    gs = [marked(s, gdtype) for s in ADAPTED]
    opt = _step_once(ws, gs)
    want = [[w.double().square().sum().item(), g.double().square().sum().item()]
            for w, g in zip(ws, gs)]
    # a later mark overwrites an earlier one at the same index: n=1 keeps 8
    # alone, n=CHUNK has 8 at CHUNK-1, n=CHUNK+1 has 8 at CHUNK
    assert [x[0] for x in want] == [64.0, 65.0, 65.0, 65.0, 69.0, 85.0, 85.0]
    assert all(x[0] == x[1] for x in want)
    assert opt.last_sqnorms[0].tolist() == want


# ---------------------------------------------------------------------------
# 2-3. random data: norms and q
# ---------------------------------------------------------------------------
WD, EPS = 1e-2, 1e-8


def _random_step(pdtype, gdtype):
    ws, _ = R.make_params(ADAPTED, pdtype, "cuda", seed=3)
    gen = torch.Generator(device="cuda").manual_seed(4)
    gs = [torch.randn(w.shape, device="cuda", generator=gen).to(gdtype)
          for w in ws]
    opt = _step_once(ws, gs, trust_coef=R.TRUST, weight_decay=WD, eps=EPS)
    exact = [[w.double().square().sum().item(),
              g.double().square().sum().item()] for w, g in zip(ws, gs)]
    return opt, ws, exact


@DTYPES
def test_sqnorms_against_fp64(pdtype, gdtype):
    opt, ws, exact = _random_step(pdtype, gdtype)
    got = opt.last_sqnorms[0].double().tolist()
    worst = 0.0
    for w, g2, e2 in zip(ws, got, exact):
        bound = (w.numel() + 1) * R.U
        for a, b in zip(g2, e2):
            worst = max(worst, abs(a - b) / b / bound)
    print(f"lars sqnorm worst err/bound = {worst:.4f}")
    assert worst <= 1.0


@DTYPES
def test_trust_ratio_against_fp64(pdtype, gdtype):
    opt, ws, exact = _random_step(pdtype, gdtype)
    q = opt.last_trust[0].double().tolist()
    sq = opt.last_sqnorms[0].double().tolist()
    assert opt.last_trust[0].dtype == torch.float32
    worst_own = worst_e2e = 0.0
    for w, qi, own, ex in zip(ws, q, sq, exact):
        want = R.trust_fp64(own[0], own[1], WD, R.TRUST, EPS)
        worst_own = max(worst_own, abs(qi - want) / want / (8 * R.U))
        want = R.trust_fp64(ex[0], ex[1], WD, R.TRUST, EPS)
        bound = (2 * (w.numel() + 1) + 8) * R.U
        worst_e2e = max(worst_e2e, abs(qi - want) / want / bound)
    print(f"lars q worst err/bound: own norms {worst_own:.4f}, "
          f"fp64 norms {worst_e2e:.4f}")
    assert worst_own <= 1.0 and worst_e2e <= 1.0


def _assert_same_state(opt_a, pa, opt_b, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b), a.shape
        sa, sb = opt_a.state.get(a, {}), opt_b.state.get(b, {})
        assert sa.keys() == sb.keys()
        for k in sa:
            if torch.is_tensor(sa[k]):
                assert torch.equal(sa[k], sb[k]), (a.shape, k)


@DTYPES
def test_trust_is_one_where_lars_does_not_apply(pdtype, gdtype):
    from distribuuuu_amd.ops.optim import HIPSGD

    gen = torch.Generator(device="cuda").manual_seed(5)

    def rn(*s):
        return torch.randn(s, device="cuda", generator=gen)

    n = CHUNK + 1
    w = [rn(n), torch.zeros(n, 1, device="cuda"), rn(n, 1), rn(n, 1), rn(n, 1)]
    g = [rn(n), rn(n, 1), torch.zeros(n, 1, device="cuda"), None, rn(n, 1)]
    w = [t.to(pdtype) for t in w]
    g = [None if t is None else t.to(gdtype) for t in g]
    before = [t.clone() for t in w]
    sgd_w = [t.clone() for t in w]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2, nesterov=True)
    opt, sgd = _lars(w, trust_coef=R.TRUST, **kw), HIPSGD(sgd_w, **kw)
    for p, s, grad in zip(w, sgd_w, g):
        R.set_grad(p, grad)
        R.set_grad(s, None if grad is None else grad.clone())
    opt.step()
    sgd.step()
    q = opt.last_trust[0].tolist()
    assert q[:4] == [1.0, 1.0, 1.0, 1.0] and 0 < q[4] < 1, q
    # 1-D, zero weight, zero grad: exactly HIPSGD's update
    _assert_same_state(opt, w[:3], sgd, sgd_w[:3])
    assert torch.equal(w[3], before[3]) and not opt.state.get(w[3])
    assert not torch.equal(w[4], sgd_w[4])
    sq = opt.last_sqnorms[0]
    assert sq[1, 0].item() == 0 and sq[2, 1].item() == 0
    assert sq[3].tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------
# 4. trajectory
# ---------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name,kwargs", R.CONFIGS,
                         ids=[c[0] for c in R.CONFIGS])
def test_fused_lars_matches_fp64(name, kwargs, pdtype, gdtype):
    shapes = ADAPTED + [(255,)]  # the last one is not adapted
    params, refs = R.make_params(shapes, pdtype, "cuda")
    opt = _lars(params, lr=R.LRS[0], trust_coef=R.TRUST, **kwargs)
    # under dampening, a parameter whose first step comes at step 3
    late = 2 if name == "dampening" else None
    ref = R.trajectory(opt, params, refs, gdtype, R.LRS, late=late)
    R.check(opt, ref, params, refs, kwargs["momentum"])
    q = opt.last_trust[0].tolist()
    assert q[-1] == 1.0 and all(v > 0 and v != 1.0 for v in q[:-1]), q


# ---------------------------------------------------------------------------
# 5. the paths agree
# ---------------------------------------------------------------------------
@DTYPES
def test_one_dim_group_is_bit_identical_to_hipsgd(pdtype, gdtype):
    from distribuuuu_amd.ops.optim import HIPSGD

    shapes = [s for s in R.SHAPES if len(s) == 1]
    pa, _ = R.make_params(shapes, pdtype, "cuda", seed=6)
    pb = [p.clone() for p in pa]
    kw = dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=5e-5)
    lars, sgd = _lars(pa, trust_coef=R.TRUST, **kw), HIPSGD(pb, **kw)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for lr in R.LRS[1:]:
        for a, b in zip(pa, pb):
            g = torch.randn(a.shape, device="cuda", generator=gen).to(gdtype)
            R.set_grad(a, g)
            R.set_grad(b, g.clone())
        for o in (lars, sgd):
            o.param_groups[0]["lr"] = lr
        lars.step()
        sgd.step()
        _assert_same_state(lars, pa, sgd, pb)
    assert lars.last_trust[0].tolist() == [1.0] * len(pa)


def _two_runs(pdtype, gdtype, make_a, make_b, steps=R.LRS, before_b=None):
    shapes = ADAPTED + [(255,)]
    pa, _ = R.make_params(shapes, pdtype, "cuda", seed=8)
    pb = [p.clone() for p in pa]
    a, b = make_a(pa), make_b(pb)
    if before_b is not None:
        before_b(b)
    gen = torch.Generator(device="cuda").manual_seed(9)
    for lr in steps:
        for x, y in zip(pa, pb):
            g = torch.randn(x.shape, device="cuda", generator=gen).to(gdtype)
            R.set_grad(x, g)
            R.set_grad(y, g.clone())
        for o in (a, b):
            o.param_groups[0]["lr"] = lr
        a.step()
        b.step()
    return a, pa, b, pb


KW5 = dict(lr=0.1, momentum=0.9, weight_decay=5e-5, nesterov=True,
           trust_coef=R.TRUST)


@DTYPES
def test_lars_step_dev_is_bit_identical_to_lars_step(pdtype, gdtype):
    def dev(o):
        o.enable_device_lr()
        assert o.device_lr_blocker() is None

    a, pa, b, pb = _two_runs(pdtype, gdtype, lambda p: _lars(p, **KW5),
                             lambda p: _lars(p, **KW5), before_b=dev)
    assert b._lr_dev[0].item() == pytest.approx(R.LRS[-1])
    _assert_same_state(a, pa, b, pb)
    assert torch.equal(a.last_trust[0], b.last_trust[0])
    assert torch.equal(a.last_sqnorms[0], b.last_sqnorms[0])


@DTYPES
def test_two_runs_are_bit_identical(pdtype, gdtype):
    from distribuuuu_amd import ops

    assert not ops.is_deterministic()
    a, pa, b, pb = _two_runs(pdtype, gdtype, lambda p: _lars(p, **KW5),
                             lambda p: _lars(p, **KW5))
    _assert_same_state(a, pa, b, pb)
    assert torch.equal(a.last_trust[0], b.last_trust[0])
    assert torch.equal(a.last_sqnorms[0], b.last_sqnorms[0])


@DTYPES
def test_fused_and_tensor_paths_agree(pdtype, gdtype):
    a, pa, b, pb = _two_runs(pdtype, gdtype, lambda p: _lars(p, **KW5),
                             lambda p: _lars(p, fused=False, **KW5))
    assert "_hip_table" in a.param_groups[0]
    assert "_hip_table" not in b.param_groups[0]
    for x, y in zip(pa, pb):
        for k in ("momentum_buffer", "master"):
            if k in a.state[x]:
                assert torch.allclose(a.state[x][k], b.state[y][k],
                                      **R.TOL), (x.shape, k)
        if x.dtype == torch.float32:
            assert torch.allclose(x, y, **R.TOL), x.shape
    assert torch.allclose(a.last_trust[0], b.last_trust[0], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------
# 6. layouts
# ---------------------------------------------------------------------------
@DTYPES
def test_two_groups_with_their_own_knobs(pdtype, gdtype):
    params, refs = R.make_params(ADAPTED, pdtype, "cuda", seed=10)
    groups = [dict(params=params[:4], weight_decay=1e-2, trust_coef=0.1),
              dict(params=params[4:], weight_decay=0.0, trust_coef=0.02)]
    opt = _lars(groups, lr=R.LRS[0], momentum=0.9, nesterov=True,
                trust_coef=0.5, eps=1e-6)
    ref = R.trajectory(opt, params, refs, gdtype, R.LRS)
    R.check(opt, ref, params, refs, 0.9)
    for gi, grp in enumerate(opt.param_groups):
        assert grp["eps"] == 1e-6
        q = opt.last_trust[gi].double().tolist()
        sq = opt.last_sqnorms[gi].double().tolist()
        assert len(q) == len(grp["params"])
        for qi, s in zip(q, sq):
            want = R.trust_fp64(s[0], s[1], grp["weight_decay"],
                                grp["trust_coef"], 1e-6)
            assert abs(qi - want) <= 8 * R.U * want


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_grad_views_at_odd_element_offsets(dtype):
    """Grads that are views into a flat buffer at element offsets 1 and 3
    (not 16-byte aligned): exact norms, and the same bits as with aligned
    copies of the same grads, since the summation order does not depend on
    alignment."""
    shapes = [(CHUNK, 1), (2 * CHUNK + 7, 1)]
    pa = [_signs(s, 20 + i).to(dtype) for i, s in enumerate(shapes)]
    pb = [p.clone() for p in pa]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=5e-5, trust_coef=R.TRUST)
    a, b = _lars(pa, **kw), _lars(pb, **kw)
    total = sum(p.numel() for p in pa) + 8
    gen = torch.Generator(device="cuda").manual_seed(22)
    for step in range(2):
        buf = torch.zeros(total, dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        off = 1
        for x, y in zip(pa, pb):
            n = x.numel()
            view = buf[off:off + n].view_as(x)
            if step == 0:
                view.copy_(2.0 * _signs(x.shape, 30 + off))
            else:
                view.copy_(torch.randn(x.shape, device="cuda", generator=gen))
            assert view.data_ptr() % 16 != 0
            x.grad = view
            y.grad = view.clone()
            off += n + 2  # the second view starts at element offset 3 mod 4
        assert (pa[1].grad.data_ptr() - buf.data_ptr()) \
            // buf.element_size() % 4 == 3
        a.step()
        b.step()
        if step == 0:
            assert a.last_sqnorms[0].tolist() == [
                [float(p.numel()), 4.0 * p.numel()] for p in pa]
        _assert_same_state(a, pa, b, pb)
        assert torch.equal(a.last_sqnorms[0], b.last_sqnorms[0])
        assert torch.equal(a.last_trust[0], b.last_trust[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_channels_last_grad_takes_stride_aware_path(dtype):
    from distribuuuu_amd.ops.optim import HIPSGD

    shapes = [(16, 8, 3, 3), (CHUNK + 1, 1)]
    params, refs = R.make_params(shapes, dtype, "cuda", seed=12)

    def layout(g):
        if g.dim() == 4:
            g = g.contiguous(memory_format=torch.channels_last)
            assert g.stride() != params[0].stride()
        return g

    opt = _lars(params, lr=R.LRS[0], momentum=0.9, nesterov=True,
                weight_decay=5e-5, trust_coef=R.TRUST)
    HIPSGD._warned_layout = False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ref = R.trajectory(opt, params, refs, dtype, R.LRS, layout=layout)
    assert sum("not laid out like" in str(w.message) for w in caught) == 1
    assert [p for p, _ in opt.param_groups[0]["_hip_table"][2]] == [params[0]]
    R.check(opt, ref, params, refs, 0.9)
    q = opt.last_trust[0].double().tolist()
    sq = opt.last_sqnorms[0].double().tolist()
    # the kernel's q (params[1]) holds 8 * 2^-24; the tensor-op q (params[0])
    # goes through torch's device sqrt and divide, taken as within 2 ulp
    # (4 * 2^-24) each, plus a multiply, a multiply-add and an add:
    # 3*4 + 3 = 15, rounded to 16
    for qi, s, k in zip(q, sq, (16, 8)):
        want = R.trust_fp64(s[0], s[1], 5e-5, R.TRUST, 1e-8)
        assert qi != 1.0 and abs(qi - want) <= k * R.U * want
    assert opt.device_lr_blocker() is not None


# ---------------------------------------------------------------------------
# 7. captured step
# ---------------------------------------------------------------------------
def test_captured_lars_step_matches_eager(tmp_path):
    from distribuuuu_amd import models, ops, utils
    from distribuuuu_amd.config import cfg
    from distribuuuu_amd.graph_step import GraphedTrainStep
    from distribuuuu_amd.ops import functional as DF
    from distribuuuu_amd.trainer import _prepare_batch

    cudnn = (torch.backends.cudnn.deterministic,
             torch.backends.cudnn.benchmark)
    was_det = ops.is_deterministic()
    cfg.RNG_SEED = 3
    cfg.CUDNN.DETERMINISTIC = True
    cfg.OUT_DIR = str(tmp_path)
    cfg.TRAIN.DTYPE = "bfloat16"
    cfg.TRAIN.CHANNELS_LAST = True
    cfg.OPTIM.OPTIMIZER = "lars"
    cfg.OPTIM.LARS_TRUST_COEF = 0.02
    cfg.OPTIM.BASE_LR = 0.5
    gen = torch.Generator().manual_seed(21)
    batches = [(torch.randn(8, 3, 32, 32, generator=gen).cuda(),
                torch.randint(0, 16, (8,), generator=gen).cuda())
               for _ in range(5)]
    lrs = [0.5, 0.5, 0.5, 0.1, 0.1]  # changes before the fourth step
    dev = torch.device("cuda")

    def build():
        from distribuuuu_amd.ops.optim import HIPLARS

        utils.setup_seed()
        assert ops.is_deterministic()
        m = models.build_model("resnet18", num_classes=16).to(dev)
        m = m.to(torch.bfloat16)
        for mod in m.modules():
            if hasattr(mod, "running_mean"):
                mod.float()
        m = m.to(memory_format=torch.channels_last).train()
        opt = utils.construct_optimizer(m)
        assert type(opt) is HIPLARS and opt._fused
        return m, opt

    def snapshot(m, opt):
        snap = {f"model.{k}": v.detach().clone()
                for k, v in m.state_dict().items()}
        for i, p in enumerate(m.parameters()):
            for k, v in opt.state[p].items():
                if torch.is_tensor(v):
                    snap[f"opt.{i}.{k}"] = v.detach().clone()
        return snap

    try:
        m, opt = build()
        trusts_eager = []
        for (x, t), lr in zip(batches, lrs):
            utils.set_lr(opt, lr)
            x, t = _prepare_batch(x, t, dev, torch.bfloat16)
            loss = DF.cross_entropy(m(x).float(), t)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            trusts_eager.append(opt.last_trust[0].clone())
        eager = snapshot(m, opt)

        m, opt = build()
        runner = GraphedTrainStep(m, DF.cross_entropy, opt, 5, warmup=2,
                                  dtype=torch.bfloat16)
        trusts = []
        for (x, t), lr in zip(batches, lrs):
            utils.set_lr(opt, lr)
            runner(x, t)
            torch.cuda.synchronize()
            trusts.append(opt.last_trust[0].clone())
        graphed = snapshot(m, opt)
        stats = dict(runner.stats)
        runner._release()
    finally:
        ops.set_deterministic(was_det)
        (torch.backends.cudnn.deterministic,
         torch.backends.cudnn.benchmark) = cudnn

    assert stats["captures"] == 1 and stats["replays"] == 3, stats
    assert stats["eager_steps"] == 2 and stats["fallback_reason"] is None
    assert eager.keys() == graphed.keys()
    assert any(k.endswith("momentum_buffer") for k in eager)
    assert any(k.endswith("master") for k in eager)
    bad = [k for k in eager if not torch.equal(eager[k], graphed[k])]
    assert not bad, f"{len(bad)} of {len(eager)} tensors differ: {bad[:5]}"
    # the replays wrote q where last_trust points, and it moved
    for i in range(5):
        assert torch.equal(trusts[i], trusts_eager[i]), i
    assert not torch.equal(trusts[2], trusts[3])
    assert not torch.equal(trusts[3], trusts[4])
    ndims = [p.ndim for p in m.parameters()]
    assert all((v == 1.0) == (d <= 1)
               for v, d in zip(trusts[4].tolist(), ndims))
