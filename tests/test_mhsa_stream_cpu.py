"""Host side of the streaming MHSA route: the range predicate at its edges
and the trainer's fmap_size-aware factory call."""

import pytest

from distribuuuu_amd import models, trainer
from distribuuuu_amd.ops.attention import (hip_mhsa_stream_supported,
                                           hip_mhsa_supported)


@pytest.mark.parametrize("h,w,want", [(16, 16, False), (17, 16, True),
                                      (32, 32, True), (33, 8, False),
                                      (17, 3, False)])
def test_stream_range_edges(h, w, want):
    assert hip_mhsa_stream_supported(h, w, 128) is want
    # the two ranges never overlap
    assert not (want and hip_mhsa_supported(h, w, 128))


def test_stream_range_head_dims():
    assert all(hip_mhsa_stream_supported(24, 24, d) for d in (32, 64, 96, 128))
    assert not any(hip_mhsa_stream_supported(24, 24, d) for d in (16, 48, 160))


@pytest.fixture
def stub_arch(monkeypatch):
    calls = []

    def stubnet(num_classes=1000, fmap_size=(14, 14)):
        calls.append((num_classes, fmap_size))
        return "net"

    monkeypatch.setattr(models, "stubnet", stubnet, raising=False)
    return calls


@pytest.mark.parametrize("im_size,fmap", [(224, (14, 14)), (384, (24, 24))])
def test_trainer_passes_fmap_size(stub_arch, im_size, fmap):
    assert trainer.build_arch("stubnet", im_size, 10) == "net"
    assert stub_arch == [(10, fmap)]


def test_trainer_rejects_im_size_off_stride(stub_arch):
    with pytest.raises(ValueError, match="multiple of 16, got 230"):
        trainer.build_arch("stubnet", 230, 10)
    assert not stub_arch


def test_trainer_leaves_other_archs_alone(monkeypatch):
    monkeypatch.setattr(models, "plainnet", lambda num_classes=1000: num_classes,
                        raising=False)
    assert trainer.build_arch("plainnet", 230, 7) == 7
