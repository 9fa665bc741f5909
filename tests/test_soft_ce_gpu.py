"""ce_soft_fwd / ce_soft_bwd (label smoothing + batch-reversal mixing) against
an fp64 reference built from the definition

    q[n, j]  = (1-eps) * (lam*[j==a] + (1-lam)*[j==b]) + eps/K
    loss     = mean_n(-sum_j q[n, j] * log_softmax(x[n])[j])
    dx[n, j] = gl/N * (softmax(x[n])[j] - q[n, j])

with a = target[n], b = target[N-1-n] and lam the fp32 value the kernel reads.
The bounds are the ones the suite holds ce_fwd / ce_bwd to
(tests/test_pool_loss_gpu.py): 1e-5 relative, or 4x the error that ATen's own
fp32 F.cross_entropy(logits, q) makes on the same inputs, measured here; each
gradient row sums to zero within K * 2^-23 * gl/N (or 4x ATen's worst row).

Measured on MI355X over the cases below (worst error / bound): loss 0.028,
gradient 0.19, row sum 0.44 (`pytest -s` prints them per case).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GRID_CAP = 2048 * 256  # grid_1d: work items covered by one grid-stride trip
GL = 0.37
CE_REL = 1e-5
ATEN_MULT = 4.0
PAIRS = [(0.1, None), (0.0, 0.3), (0.1, 0.3), (0.1, 0.0), (0.5, 0.5)]
PAIR_IDS = ["eps.1", "lam.3", "eps.1-lam.3", "eps.1-lam0", "eps.5-lam.5"]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


@pytest.fixture(autouse=True)
def _mode_off_after():
    from distribuuuu_amd import ops

    was = ops.is_deterministic()
    yield
    ops.set_deterministic(was)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ce_case(n, k, s, seed):
    """As _ce_case of tests/test_pool_loss_gpu.py."""
    logits = torch.randn(n, k, device="cuda", generator=_gen(seed)) * s
    logits[0] += 90.0           # overflows exp() without max-subtraction
    logits[n - 1] -= 90.0       # (n == 1: the row ends up unshifted)
    target = torch.randint(0, k, (n,), device="cuda", generator=_gen(seed + 1))
    target[0] = 0
    target[n - 1] = k - 1
    if n > 2:
        target[1] = k - 1
    if n > 3:
        target[2] = 0
    return logits, target


def _lam_tensor(lam):
    if lam is None:
        return None
    return torch.tensor([lam], dtype=torch.float32, device="cuda")


def _q64(target, k, eps, lam_t):
    lam = 1.0 if lam_t is None else lam_t.double().item()  # the fp32 value
    a = F.one_hot(target, k).double()
    b = F.one_hot(target.flip(0), k).double()
    return (1.0 - eps) * (lam * a + (1.0 - lam) * b) + eps / k


def _reference(logits, q):
    ls = F.log_softmax(logits.double(), dim=1)
    n = logits.shape[0]
    loss = -(q * ls).sum(dim=1).mean()
    grad = (ls.exp() - q) * (GL / n)
    return loss, grad


def _aten_errors(logits, q, ref_loss, ref_grad):
    lr = logits.detach().clone().requires_grad_(True)
    loss = F.cross_entropy(lr, q.float())
    loss.backward(torch.tensor(GL, device="cuda"))
    return ((loss.double() - ref_loss).abs().item(),
            (lr.grad.double() - ref_grad).abs().max().item(),
            lr.grad.double().sum(dim=1).abs().max().item())


def _soft_check(n, k, s, eps, lam, seed):
    e = _ext()
    logits, target = _ce_case(n, k, s, seed)
    lam_t = _lam_tensor(lam)
    q = _q64(target, k, eps, lam_t)
    ref_loss, ref_grad = _reference(logits, q)
    a_loss, a_grad, a_row = _aten_errors(logits, q, ref_loss, ref_grad)
    tol_loss = max(CE_REL * ref_loss.abs().item(), ATEN_MULT * a_loss)
    tol_grad = torch.maximum(CE_REL * ref_grad.abs(),
                             torch.full_like(ref_grad, ATEN_MULT * a_grad))
    row_bound = max(k * 2.0 ** -23 * GL / n, ATEN_MULT * a_row)
    gl = torch.tensor(GL, device="cuda")

    loss, lse = e.ce_soft_fwd(logits, target, lam_t, eps)
    gx = e.ce_soft_bwd(logits, target, lse, gl, lam_t, eps)
    assert loss.shape == () and lse.shape == (n, 2) and gx.shape == (n, k)
    assert torch.isfinite(loss) and torch.isfinite(gx).all()
    err_loss = (loss.double() - ref_loss).abs().item()
    err = (gx.double() - ref_grad).abs()
    exact = torch.where(err > 0, float("inf"), 0.0)  # where the tolerance is 0
    err_grad = torch.where(tol_grad > 0, err / tol_grad.clamp_min(1e-300),
                           exact).max().item()
    rowsum = gx.double().sum(dim=1).abs().max().item()
    # a loss of exactly 0 (one class dominating at scale 30) has tolerance 0
    r_loss = err_loss / tol_loss if tol_loss > 0 else float(err_loss > 0)
    print(f"soft_ce n={n} k={k} s={s} eps={eps} lam={lam}: loss err/tol "
          f"{r_loss:.3g} (aten {a_loss:.3g}); grad err/tol "
          f"{err_grad:.3g} (aten abs {a_grad:.3g}); row sum/bound "
          f"{rowsum / row_bound:.3g} (aten {a_row:.3g})")
    assert err_loss <= tol_loss
    assert err_grad <= 1.0
    assert rowsum <= row_bound
    return logits, target, lam_t, loss, lse, gx


@pytest.mark.parametrize("eps,lam", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("s", [1, 30], ids=["s1", "s30"])
@pytest.mark.parametrize("k", [2, 10, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_soft_cross_entropy_vs_fp64(n, k, s, eps, lam):
    _soft_check(n, k, s, eps, lam, seed=100 + k + n)


def test_soft_cross_entropy_second_grid_stride_trip():
    assert 600 * 1000 > GRID_CAP
    _soft_check(600, 1000, 1, 0.1, 0.3, seed=300)


@pytest.mark.parametrize("deterministic", [False, True],
                         ids=["atomic", "deterministic"])
@pytest.mark.parametrize("n,k,s", [(1, 2, 1), (3, 257, 30), (64, 1000, 1),
                                   (600, 1000, 1)])
def test_plain_arguments_equal_hard_kernels_bitwise(n, k, s, deterministic):
    """eps = 0 and no lam: the SOFT bodies compute the hard loss; lse and gx
    to the bit, and the loss too where its row sum is ordered."""
    from distribuuuu_amd import ops

    e = _ext()
    ops.set_deterministic(deterministic)
    logits, target = _ce_case(n, k, s, seed=400 + k + n)
    gl = torch.tensor(GL, device="cuda")
    loss0, lse0 = e.ce_fwd(logits, target)
    gx0 = e.ce_bwd(logits, target, lse0, gl)
    loss1, lse1 = e.ce_soft_fwd(logits, target, None, 0.0)
    gx1 = e.ce_soft_bwd(logits, target, lse1, gl, None, 0.0)
    assert torch.equal(lse0, lse1)
    assert torch.equal(gx0, gx1)
    if deterministic or n == 1:
        assert torch.equal(loss0, loss1)
    else:
        assert torch.allclose(loss0, loss1, rtol=1e-5)


@pytest.mark.parametrize("n,k,s", [(3, 257, 30), (64, 1000, 1), (64, 10, 30)])
def test_smoothing_alone_matches_torch_label_smoothing(n, k, s):
    e = _ext()
    logits, target = _ce_case(n, k, s, seed=500 + k + n)
    ref = F.cross_entropy(logits.double(), target, label_smoothing=0.1)
    aten = F.cross_entropy(logits, target, label_smoothing=0.1)
    a_loss = (aten.double() - ref).abs().item()
    tol = max(CE_REL * ref.abs().item(), ATEN_MULT * a_loss)
    loss, _ = e.ce_soft_fwd(logits, target, None, 0.1)
    err = (loss.double() - ref).abs().item()
    print(f"smoothing n={n} k={k} s={s}: err/tol {err / tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("n,k,s", [(3, 257, 30), (64, 1000, 1), (64, 10, 30)])
def test_soft_cross_entropy_deterministic_mode(n, k, s):
    from distribuuuu_amd import ops

    e = _ext()
    ops.set_deterministic(True)
    logits, target, lam_t, loss, lse, gx = _soft_check(
        n, k, s, 0.1, 0.3, seed=200 + k + n)
    gl = torch.tensor(GL, device="cuda")
    loss2, lse2 = e.ce_soft_fwd(logits, target, lam_t, 0.1)
    gx2 = e.ce_soft_bwd(logits, target, lse2, gl, lam_t, 0.1)
    assert torch.equal(loss, loss2) and torch.equal(lse, lse2)
    assert torch.equal(gx, gx2)


def test_autograd_function_uses_the_soft_kernels():
    from distribuuuu_amd import ops
    from distribuuuu_amd.ops import functional as DF

    e = _ext()
    ops.set_deterministic(True)
    logits, target = _ce_case(8, 16, 1, seed=600)
    lam_t = _lam_tensor(0.3)
    x = logits.clone().requires_grad_(True)
    loss = DF.cross_entropy(x, target, label_smoothing=0.1, lam=lam_t)
    (loss * GL).backward()
    want, lse = e.ce_soft_fwd(logits, target, lam_t, 0.1)
    assert torch.equal(loss.detach(), want)
    gl = torch.tensor(GL, device="cuda")
    assert torch.equal(x.grad, e.ce_soft_bwd(logits, target, lse, gl, lam_t,
                                             0.1))
    # positional use stays on the hard kernels
    assert torch.equal(DF.cross_entropy(logits, target),
                       e.ce_fwd(logits, target)[0])


def test_captured_loss_follows_lambda():
    """lam is read from memory: a replay after lam.fill_ computes the loss
    and gradient of the new value, to the bit in deterministic mode."""
    from distribuuuu_amd import ops

    e = _ext()
    ops.set_deterministic(True)
    logits, target = _ce_case(64, 257, 1, seed=700)
    lam_t = _lam_tensor(0.3)
    gl = torch.tensor(GL, device="cuda")
    ptr = lam_t.data_ptr()

    def eager():
        loss, lse = e.ce_soft_fwd(logits, target, lam_t, 0.1)
        return loss, lse, e.ce_soft_bwd(logits, target, lse, gl, lam_t, 0.1)

    at_old = [t.clone() for t in eager()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = eager()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, at_old):
        assert torch.equal(got, want)
    lam_t.fill_(0.8)
    assert lam_t.data_ptr() == ptr
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    at_new = eager()
    torch.cuda.synchronize()
    for got, want in zip(replayed, at_new):
        assert torch.equal(got, want)
    assert not torch.equal(replayed[0], at_old[0])
    assert not torch.equal(replayed[2], at_old[2])
    assert torch.equal(replayed[1], at_old[1])  # (max, log-sum) know no lam


def test_bad_arguments_raise_before_launch():
    e = _ext()
    logits, target = _ce_case(4, 10, 1, seed=800)
    gl = torch.tensor(GL, device="cuda")
    _, lse = e.ce_soft_fwd(logits, target, None, 0.1)
    ok = _lam_tensor(0.5)
    bad_lams = [torch.tensor([0.5], dtype=torch.float64, device="cuda"),
                torch.tensor([0.5], dtype=torch.bfloat16, device="cuda"),
                torch.tensor([0.5, 0.5], dtype=torch.float32, device="cuda"),
                torch.empty(0, dtype=torch.float32, device="cuda"),
                torch.tensor([0.5], dtype=torch.float32)]
    for lam in bad_lams:
        with pytest.raises(RuntimeError, match="lam"):
            e.ce_soft_fwd(logits, target, lam, 0.1)
        with pytest.raises(RuntimeError, match="lam"):
            e.ce_soft_bwd(logits, target, lse, gl, lam, 0.1)
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="smoothing"):
            e.ce_soft_fwd(logits, target, ok, eps)
        with pytest.raises(RuntimeError, match="smoothing"):
            e.ce_soft_bwd(logits, target, lse, gl, ok, eps)
    with pytest.raises(RuntimeError, match="fp32"):
        e.ce_soft_fwd(logits.to(torch.bfloat16), target, ok, 0.1)
    with pytest.raises(RuntimeError, match="targets"):
        e.ce_soft_fwd(logits, target[:3], ok, 0.1)
    with pytest.raises(RuntimeError, match="targets"):
        e.ce_soft_fwd(logits, target.int(), ok, 0.1)
    with pytest.raises(RuntimeError, match="lse"):
        e.ce_soft_bwd(logits, target, lse[:3], gl, ok, 0.1)
    torch.cuda.synchronize()
