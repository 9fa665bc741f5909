"""Pooling, loss, top-k and plain elementwise kernels against fp64 references
(or, where the operation is exact, bit-for-bit against ATen), at the shapes
where they take another path: odd extents, dropped tail rows, overlapping
windows, padded borders, ties, channel counts off the pack width, a second
channel block, logits that overflow without max-subtraction, and more than
2048 x 256 work items (second trip of the grid-stride loops).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GRID_CAP = 2048 * 256  # grid_1d: work items covered by one grid-stride trip


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _tol(dtype):
    return dict(atol=3e-2, rtol=3e-2) if dtype == torch.bfloat16 else dict(
        atol=1e-4, rtol=1e-4)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------
def _maxpool_check(x, k, s, p, seed):
    """Forward bit-equal to ATen in the same dtype. Backward against fp64
    autograd on the CPU (first maximum in window scan order wins a tie, the
    rule the saved window-local index encodes). gy holds multiples of 1/8 in
    [-1, 1], so the up-to-9-term sums are exact in fp32 AND in bf16: the
    comparison is exact, which is inside the 1 ulp the sums would need."""
    e = _ext()
    y, idx = e.maxpool_fwd(x, k, s, p)
    ref = F.max_pool2d(x, k, s, p)
    assert y.shape == ref.shape
    assert torch.equal(y, ref)
    gy = _cl((torch.randint(-8, 9, y.shape, device="cuda",
                            generator=_gen(seed)) / 8.0).to(x.dtype))
    gx = e.maxpool_bwd(gy, idx, x.shape[2], x.shape[3], k, s, p)
    xr = x.double().cpu().contiguous().requires_grad_(True)
    F.max_pool2d(xr, k, s, p).backward(gy.double().cpu().contiguous())
    want = xr.grad.to(x.dtype)
    assert torch.equal(want.double(), xr.grad)  # exactly representable
    assert torch.equal(gx.cpu(), want)


@pytest.mark.parametrize("dtype,c", [(torch.bfloat16, 8), (torch.bfloat16, 40),
                                     (torch.float32, 4), (torch.float32, 12)],
                         ids=["bf16-c8", "bf16-c40", "fp32-c4", "fp32-c12"])
@pytest.mark.parametrize("hw", [(15, 13), (7, 7)], ids=["15x13", "7x7"])
@pytest.mark.parametrize("ksp", [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0)],
                         ids=["k3s2p1", "k2s2p0", "k3s1p1", "k3s2p0"])
@pytest.mark.parametrize("kind", ["negative", "ties"])
def test_maxpool_vs_aten_and_fp64(kind, ksp, hw, dtype, c):
    shape = (3, c, hw[0], hw[1])
    if kind == "negative":
        # all-negative: a zero (instead of -inf) padding value would win
        x = torch.randn(shape, device="cuda", generator=_gen(1)) - 5.0
        x = x.clamp_max(-0.0625)
    else:
        x = torch.randint(-1, 3, shape, device="cuda",
                          generator=_gen(2)).float()
    _maxpool_check(_cl(x.to(dtype)), *ksp, seed=3)


@pytest.mark.parametrize("ksp", [(3, 2, 1), (3, 1, 1)],
                         ids=["k3s2p1", "k3s1p1"])
def test_maxpool_second_grid_stride_trip(ksp):
    """540,800 input packs. With stride 2 (the stem pool) the forward has a
    quarter of that and the specialised backward has a 2-D grid, so only
    stride 1 takes the second trip, in the forward and the generic backward."""
    n, c, h, w = 4, 64, 130, 130
    assert n * h * w * (c // 8) > GRID_CAP
    x = _cl(torch.randn(n, c, h, w, device="cuda",
                        generator=_gen(4)).to(torch.bfloat16))
    _maxpool_check(x, *ksp, seed=5)


# ---------------------------------------------------------------------------
# global average pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c", [(torch.bfloat16, 8),
                                     (torch.bfloat16, 264),   # 2nd c-block
                                     (torch.bfloat16, 20),    # scalar path
                                     (torch.float32, 4),
                                     (torch.float32, 6)],     # scalar path
                         ids=["bf16-c8", "bf16-c264", "bf16-c20", "fp32-c4",
                              "fp32-c6"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (3, 11), (7, 7), (14, 14)],
                         ids=["hw1", "hw7", "hw33", "hw49", "hw196"])
def test_gap_vs_fp64(hw, dtype, c):
    e = _ext()
    h, w = hw
    x = _cl((torch.randn(3, c, h, w, device="cuda", generator=_gen(6))
             + 0.5).to(dtype))
    y = e.gap_fwd(x)
    ref = x.double().mean(dim=(2, 3), keepdim=True)
    assert y.shape == ref.shape
    assert torch.allclose(y.double(), ref, **_tol(dtype))
    gy = torch.randn(3, c, 1, 1, device="cuda", generator=_gen(7)).to(dtype)
    gx = e.gap_bwd(gy.contiguous(), h, w)
    assert gx.is_contiguous(memory_format=torch.channels_last)
    ref_gx = gy.double().expand(3, c, h, w) / (h * w)
    assert torch.allclose(gx.double(), ref_gx, **_tol(dtype))


def test_gap_bwd_second_grid_stride_trip():
    e = _ext()
    n, c, h, w = 3, 264, 28, 28
    assert n * c * h * w > GRID_CAP
    gy = torch.randn(n, c, 1, 1, device="cuda",
                     generator=_gen(8)).to(torch.bfloat16)
    gx = e.gap_bwd(gy, h, w)
    ref = gy.double().expand(n, c, h, w) / (h * w)
    assert torch.allclose(gx.double(), ref, **_tol(torch.bfloat16))


# ---------------------------------------------------------------------------
# average pool (no padding)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [8, 20])
@pytest.mark.parametrize("hw", [(7, 9), (8, 8)], ids=["7x9", "8x8"])
@pytest.mark.parametrize("ks", [(2, 2), (3, 2), (3, 1)],
                         ids=["k2s2", "k3s2", "k3s1"])
def test_avgpool_vs_fp64(ks, hw, c, dtype):
    e = _ext()
    k, s = ks
    h, w = hw
    x = _cl((torch.randn(3, c, h, w, device="cuda", generator=_gen(9))
             + 0.5).to(dtype))
    y = e.avgpool_fwd(x, k, s)
    xr = x.double().detach().requires_grad_(True)
    ref = F.avg_pool2d(xr, k, s)
    assert y.shape == ref.shape
    assert torch.allclose(y.double(), ref, **_tol(dtype))
    gy = _cl(torch.randn(y.shape, device="cuda",
                         generator=_gen(10)).to(dtype))
    gx = e.avgpool_bwd(gy, k, s, h, w)
    ref.backward(gy.double())
    assert torch.allclose(gx.double(), xr.grad, **_tol(dtype))


def test_avgpool_second_grid_stride_trip():
    e = _ext()
    n, c, h, w = 4, 64, 66, 66
    assert n * c * 64 * 64 > GRID_CAP  # outputs of k3 s1; inputs are more
    x = _cl(torch.randn(n, c, h, w, device="cuda",
                        generator=_gen(11)).to(torch.bfloat16))
    y = e.avgpool_fwd(x, 3, 1)
    xr = x.double().detach().requires_grad_(True)
    ref = F.avg_pool2d(xr, 3, 1)
    assert torch.allclose(y.double(), ref, **_tol(torch.bfloat16))
    gy = _cl(torch.randn(y.shape, device="cuda",
                         generator=_gen(12)).to(torch.bfloat16))
    gx = e.avgpool_bwd(gy, 3, 1, h, w)
    ref.backward(gy.double())
    assert torch.allclose(gx.double(), xr.grad, **_tol(torch.bfloat16))


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
GL = 0.37
CE_REL = 1e-5      # the bound the suite already held the kernel to
# The kernel may also use 4x the error ATen's own fp32 cross_entropy makes on
# the same inputs, measured in the test itself. Measured on MI355X over the
# cases below, ATen vs fp64: loss relative error at most 2.3e-7, grad absolute
# error at most 1.6e-7 (in units of gl/N) -- so CE_REL is the larger of the
# two for the loss everywhere, and 4x ATen matters only for gradient entries
# below 1e-2 of a row's largest. The kernel: loss within 0.055 of its
# tolerance (5.5e-7 relative), gradients within 0.25, row sums within 0.51 of
# K * 2^-23 * gl / N.
ATEN_MULT = 4.0


def _ce_case(n, k, s, seed):
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


def _ce_reference(logits, target):
    ld = logits.double()
    ls = F.log_softmax(ld, dim=1)
    n = logits.shape[0]
    loss = -ls[torch.arange(n, device="cuda"), target].mean()
    grad = ls.exp()
    grad[torch.arange(n, device="cuda"), target] -= 1.0
    return loss, grad * (GL / n)


def _aten_errors(logits, target, ref_loss, ref_grad):
    lr = logits.detach().clone().requires_grad_(True)
    loss = F.cross_entropy(lr, target)
    loss.backward(torch.tensor(GL, device="cuda"))
    return ((loss.double() - ref_loss).abs().item(),
            (lr.grad.double() - ref_grad).abs().max().item())


def _ce_check(n, k, s, seed, deterministic=False):
    e = _ext()
    logits, target = _ce_case(n, k, s, seed)
    ref_loss, ref_grad = _ce_reference(logits, target)
    a_loss, a_grad = _aten_errors(logits, target, ref_loss, ref_grad)
    tol_loss = max(CE_REL * ref_loss.abs().item(), ATEN_MULT * a_loss)
    tol_grad = torch.maximum(CE_REL * ref_grad.abs(),
                             torch.full_like(ref_grad, ATEN_MULT * a_grad))
    gl = torch.tensor(GL, device="cuda")

    loss, lse = e.ce_fwd(logits, target)
    gx = e.ce_bwd(logits, target, lse, gl)
    assert torch.isfinite(loss) and torch.isfinite(gx).all()
    err_loss = (loss.double() - ref_loss).abs().item()
    err_grad = ((gx.double() - ref_grad).abs() / tol_grad).max().item()
    rowsum = gx.double().sum(dim=1).abs().max().item()
    row_bound = k * 2.0 ** -23 * GL / n
    print(f"ce n={n} k={k} s={s}: loss err {err_loss:.3g} (tol "
          f"{tol_loss:.3g}, aten {a_loss:.3g}, rel "
          f"{err_loss / max(ref_loss.abs().item(), 1e-300):.3g}); grad err/tol "
          f"{err_grad:.3g} (aten abs {a_grad:.3g}); row sum {rowsum:.3g} "
          f"(bound {row_bound:.3g})")
    assert err_loss <= tol_loss
    assert err_grad <= 1.0
    assert rowsum <= row_bound
    if deterministic:
        loss2, lse2 = e.ce_fwd(logits, target)
        assert torch.equal(loss, loss2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("s", [1, 30], ids=["s1", "s30"])
@pytest.mark.parametrize("k", [2, 10, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_cross_entropy_vs_fp64(n, k, s):
    _ce_check(n, k, s, seed=100 + k + n)


@pytest.mark.parametrize("n,k,s", [(3, 257, 30), (64, 1000, 1), (64, 10, 30)])
def test_cross_entropy_deterministic_mode(n, k, s):
    from distribuuuu_amd import ops

    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        _ce_check(n, k, s, seed=200 + k + n, deterministic=True)
    finally:
        ops.set_deterministic(was)


def test_cross_entropy_second_grid_stride_trip():
    assert 600 * 1000 > GRID_CAP
    _ce_check(600, 1000, 1, seed=300)


# ---------------------------------------------------------------------------
# top-k accuracy
# ---------------------------------------------------------------------------
def _rank_rule(logits, target, topk):
    """#(v > tv) + #(v == tv and j < tj), in plain Python."""
    rows = logits.float().cpu().tolist()
    c1 = ck = 0
    for row, tj in zip(rows, target.cpu().tolist()):
        tv = row[tj]
        rank = sum(1 for j, v in enumerate(row)
                   if v > tv or (v == tv and j < tj))
        c1 += rank == 0
        ck += rank < topk
    return c1, ck


def _topk_check(logits, target, topk):
    e = _ext()
    c1, ck = e.topk_acc(logits, target, topk)
    w1, wk = _rank_rule(logits, target, topk)
    assert (c1.item(), ck.item()) == (w1, wk)
    return w1, wk


def test_topk_small_k_idle_lanes():
    logits = torch.randn(5, 10, device="cuda", generator=_gen(20))
    target = torch.randint(0, 10, (5,), device="cuda", generator=_gen(21))
    _topk_check(logits, target, 5)


def test_topk_all_rows_correct_when_k_equals_classes():
    logits = torch.randn(7, 5, device="cuda", generator=_gen(22))
    target = torch.randint(0, 5, (7,), device="cuda", generator=_gen(23))
    _, wk = _topk_check(logits, target, 5)
    assert wk == 7


def test_topk_constant_rows_tie_break_by_index():
    logits = torch.full((9, 12), 0.25, device="cuda")
    target = torch.tensor([0, 1, 4, 5, 11, 0, 3, 4, 5], device="cuda")
    w1, wk = _topk_check(logits, target, 5)
    assert (w1, wk) == (2, 6)  # rank == target index on a constant row


def test_topk_partial_last_block_with_ties():
    # 130 rows = 32 full blocks of 4 rows + 2; values on a coarse grid -> ties
    logits = torch.randint(-3, 4, (130, 100), device="cuda",
                           generator=_gen(24)).float()
    target = torch.randint(0, 100, (130,), device="cuda", generator=_gen(25))
    _topk_check(logits, target, 5)


def test_topk_bf16_logits():
    logits = torch.randn(33, 100, device="cuda",
                         generator=_gen(26)).to(torch.bfloat16)
    target = torch.randint(0, 100, (33,), device="cuda", generator=_gen(27))
    _topk_check(logits, target, 5)


# ---------------------------------------------------------------------------
# elementwise: second grid-stride trip, exact against ATen
# ---------------------------------------------------------------------------
BIG = (8, 64, 130, 130)


def _big(seed):
    x = _cl(torch.randn(BIG, device="cuda",
                        generator=_gen(seed)).to(torch.bfloat16))
    assert x.numel() // 8 > GRID_CAP
    return x


def test_relu_fwd_bwd_second_grid_stride_trip():
    e = _ext()
    x, gy = _big(30), _big(31)
    y = e.relu_fwd(x)
    assert torch.equal(y, F.relu(x))
    gx = e.relu_bwd(gy, y)
    assert torch.equal(gx, torch.where(x > 0, gy, torch.zeros_like(gy)))


def test_add_relu_second_grid_stride_trip():
    e = _ext()
    a, b = _big(32), _big(33)
    y = e.add_relu_fwd(a, b)
    # the kernel adds in fp32 and rounds once, as ATen's bf16 add does
    assert torch.equal(y, F.relu(a + b))


def test_dropout_second_grid_stride_trip():
    e = _ext()
    x = _big(34)
    assert (x != 0).all()
    p = 0.3
    y = e.dropout_fwd(x, p, 4242)
    kept = y != 0
    assert abs(kept.float().mean().item() - (1 - p)) < 0.01
    # both halves of the storage (first and second trip) keep at that rate
    flat = kept.permute(0, 2, 3, 1).reshape(-1)
    half = flat.numel() // 2
    for part in (flat[:half], flat[half:]):
        assert abs(part.float().mean().item() - (1 - p)) < 0.01
    inv_keep = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32))
    want = (x.float() * inv_keep.item()).to(torch.bfloat16)
    assert torch.equal(y, torch.where(kept, want, torch.zeros_like(want)))
    assert torch.equal(e.dropout_fwd(x, p, 4242), y)
    assert not torch.equal(e.dropout_fwd(x, p, 4243), y)
