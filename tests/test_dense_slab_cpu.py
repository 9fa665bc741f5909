"""Dense-block slab route (models/densenet.py, ops/dense.py) without a GPU:
the route predicate, and the concat path staying what it was."""

import pytest
import torch

from distribuuuu_amd.models.densenet import _DenseBlock, densenet121, densenet161
from distribuuuu_amd.parallel.syncbn import convert_sync_batchnorm


@pytest.mark.parametrize("factory,im", [(densenet121, 224), (densenet161, 224)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_route_true_for_the_zoo_on_meta(factory, im, dtype):
    with torch.device("meta"):
        net = factory()
    side, blocks = im // 4, [m for m in net.modules() if isinstance(m, _DenseBlock)]
    assert len(blocks) == 4
    for block in blocks:
        c0 = next(iter(block.values())).norm1.num_features
        x = torch.empty(2, c0, side, side, device="meta", dtype=dtype)
        assert block.slab_route(x)
        side //= 2


def test_route_false_outside_the_gate(monkeypatch):
    x = torch.empty(2, 16, 8, 8, device="meta", dtype=torch.bfloat16)
    assert _DenseBlock(2, 16, 4, 8, 0.0).slab_route(x)
    assert not _DenseBlock(2, 16, 4, 8, 0.0).slab_route(
        torch.empty(2, 16, 8, 8, dtype=torch.bfloat16))  # CPU tensor
    assert not _DenseBlock(2, 16, 4, 8, 0.0, memory_efficient=True).slab_route(x)
    assert not _DenseBlock(2, 16, 4, 12, 0.0).slab_route(x)  # g % 8 != 0
    assert not _DenseBlock(2, 16, 4, 8, 0.0).slab_route(x.half())
    assert not convert_sync_batchnorm(_DenseBlock(2, 16, 4, 8, 0.0)).slab_route(x)
    # fp32 packs are 4 wide
    assert _DenseBlock(2, 16, 4, 12, 0.0).slab_route(x.float())
    monkeypatch.setenv("DISTRIBUUUU_DENSE_SLAB", "0")
    assert not _DenseBlock(2, 16, 4, 8, 0.0).slab_route(x)


def test_cpu_block_is_the_concat_composition():
    torch.manual_seed(2)
    block = _DenseBlock(3, 16, 4, 8, 0.0)
    x = torch.randn(2, 16, 6, 5)
    feats = [x]
    for layer in block.values():
        cat = torch.cat(feats, 1)
        mid = layer.conv1(layer.norm1(cat))
        feats.append(layer.conv2(layer.norm2(mid)))
    want = torch.cat(feats, 1)
    for m in block.modules():  # the loop above already updated running stats
        if hasattr(m, "running_mean"):
            m.running_mean.zero_()
            m.running_var.fill_(1.0)
    got = block(x)
    assert torch.equal(got, want)
    assert not hasattr(got, "_bn_partials")
