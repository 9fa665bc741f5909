"""batch_mix (mixup / CutMix against the reversed batch) on the GPU.

CutMix and mixup at lam 0 / 1 are pure copies: torch.equal. Mixup otherwise
against fp64 from the stored inputs and the fp32 lam. With a = x[n],
b = x[N-1-n]: the kernel forms lam*a + (1-lam)*b in fp32 (1-lam rounded once,
two products and a sum, or one product and an fma: at most 4 roundings of
2^-24 relative on terms no larger than |lam*a| + |(1-lam)*b|), so

    fp32: |err| <= B32 = 4 * 2^-24 * (|lam*a| + |(1-lam)*b|)
    bf16: |err| <= B32 + 2^-8 * (|ref| + B32)   (one rounding to 8 bits)

Shapes: 3*7*5 = 105 elements per sample and 5- or 15-element rows force the
scalar path; (8, 16, 16) and 224 x 224 take 16-byte packs; the 224 case has
more than one chunk per sample and a box edge inside a pack.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(n, c, h, w) for n in (1, 2, 3, 5)
          for (c, h, w) in ((3, 4, 6), (3, 7, 5), (8, 16, 16))]
SHAPES.append((8, 3, 224, 224))
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
LAYOUTS = [pytest.param(False, id="nchw"), pytest.param(True, id="nhwc")]
DTYPES = [pytest.param(torch.float32, id="fp32"),
          pytest.param(torch.bfloat16, id="bf16")]


def _ext():
    from distribuuuu_amd.ops.dispatch import require_ext

    e = require_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _x(shape, dtype, cl):
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda", generator=g).to(dtype)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def _same_layout(out, x):
    return out.dtype == x.dtype and out.shape == x.shape and \
        out.stride() == x.stride() and out.data_ptr() != x.data_ptr()


def _boxes(h, w):
    return {"empty": (2, 2, 1, 1),
            "empty-cols": (0, h, 3, 3),
            "whole": (0, h, 0, w),
            "last-pixel": (h - 1, h, w - 1, w),
            "interior-odd": (1, h - 1, 1, w - 2),
            "full-width-rows": (1, 3, 0, w)}


@pytest.mark.parametrize("cl", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cutmix_is_exact(shape, dtype, cl):
    e = _ext()
    x = _x(shape, dtype, cl)
    keep = x.clone()
    h, w = shape[2], shape[3]
    for name, (y0, y1, x0, x1) in _boxes(h, w).items():
        out = e.batch_mix(x, 1, 1.0, y0, y1, x0, x1)
        inside = torch.zeros(1, 1, h, w, dtype=torch.bool, device="cuda")
        inside[:, :, y0:y1, x0:x1] = True
        assert _same_layout(out, x), name
        assert torch.equal(out, torch.where(inside, x.flip(0), x)), name
    assert torch.equal(x, keep)


@pytest.mark.parametrize("cl", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_mixup_vs_fp64(shape, dtype, cl):
    e = _ext()
    x = _x(shape, dtype, cl)
    keep = x.clone()
    one = e.batch_mix(x, 0, 1.0, 0, 0, 0, 0)
    assert _same_layout(one, x) and torch.equal(one, x)
    zero = e.batch_mix(x, 0, 0.0, 0, 0, 0, 0)
    assert _same_layout(zero, x) and torch.equal(zero, x.flip(0))
    a, b = x.double(), x.flip(0).double()
    for lam in (0.3, 0.9371):
        out = e.batch_mix(x, 0, lam, 0, 0, 0, 0)
        assert _same_layout(out, x)
        l32 = torch.tensor(lam, dtype=torch.float32).double().item()
        ref = l32 * a + (1.0 - l32) * b
        b32 = 4 * 2.0 ** -24 * ((l32 * a).abs() + ((1.0 - l32) * b).abs())
        bound = b32 if dtype == torch.float32 else \
            b32 + 2.0 ** -8 * (ref.abs() + b32)
        err = (out.double() - ref).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print(f"mixup {shape} {dtype} cl={cl} lam={lam}: max err/bound "
              f"{ratio:.3f}")
        assert (err <= bound).all(), ratio
    assert torch.equal(x, keep)


def test_signed_zero_and_nonfinite_survive_the_copy_modes():
    """lam 1 / 0 and CutMix never do arithmetic: -0.0, inf and NaN come
    through as their own bit patterns."""
    e = _ext()
    x = _x((3, 3, 4, 6), torch.float32, False)
    flat = x.view(-1)
    flat[0], flat[5], flat[17], flat[40] = -0.0, float("inf"), float("nan"), \
        -float("inf")
    bits = x.view(torch.int32)
    assert torch.equal(e.batch_mix(x, 0, 1.0, 0, 0, 0, 0).view(torch.int32),
                       bits)
    assert torch.equal(e.batch_mix(x, 0, 0.0, 0, 0, 0, 0).view(torch.int32),
                       x.flip(0).view(torch.int32))


def test_functional_batch_mix_dispatch_and_dense_copy():
    from distribuuuu_amd.ops import functional as DF

    e = _ext()
    x = _x((4, 8, 16, 16), torch.bfloat16, True)
    assert torch.equal(DF.batch_mix(x, 0.3), e.batch_mix(x, 0, 0.3, 0, 0, 0, 0))
    box = (3, 9, 5, 12)
    assert torch.equal(DF.batch_mix(x, 0.5, box), e.batch_mix(x, 1, 1.0, *box))
    view = x[:, :, ::2]  # not dense: made dense in its own (NHWC) format
    out = DF.batch_mix(view, 0.3)
    dense = view.contiguous(memory_format=torch.channels_last)
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out, e.batch_mix(dense, 0, 0.3, 0, 0, 0, 0))


def test_bad_arguments_raise_before_launch():
    e = _ext()
    x = _x((2, 3, 4, 6), torch.float32, False)
    for box in ((0, 5, 0, 6), (0, 4, 0, 7), (-1, 4, 0, 6), (3, 2, 0, 6),
                (0, 4, 5, 4)):
        with pytest.raises(RuntimeError, match="box"):
            e.batch_mix(x, 1, 1.0, *box)
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(RuntimeError, match="lam"):
            e.batch_mix(x, 0, lam, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="mode"):
        e.batch_mix(x, 2, 0.5, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dense"):
        e.batch_mix(x[:, :, :, ::2], 0, 0.5, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="N, C, H, W"):
        e.batch_mix(x[0], 0, 0.5, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="dtype"):
        e.batch_mix(x.half(), 0, 0.5, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        e.batch_mix(x.cpu(), 0, 0.5, 0, 0, 0, 0)
    torch.cuda.synchronize()
