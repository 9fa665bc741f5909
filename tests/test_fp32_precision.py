"""The fp32 precision switch (docs/ARCHITECTURE.md "fp32 split-bf16 conv"):
the Python-side API, the config key and the environment variable. No GPU
needed: the switch keeps a Python copy of the flag without the extension."""

import os
import subprocess
import sys

import pytest

from distribuuuu_amd import ops
from distribuuuu_amd.config import cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _highest():
    ops.set_fp32_precision("highest")
    yield
    ops.set_fp32_precision("highest")


def test_set_get_round_trip():
    e = ops.ext()  # None on a box without the built extension
    assert ops.get_fp32_precision() == "highest"
    for mode in ("high", "highest", "high"):
        ops.set_fp32_precision(mode)
        assert ops.get_fp32_precision() == mode
        if e is not None:
            assert e.get_fp32_precision() == mode
            assert e.fp32_conv_route(64, 64, "fwd") == (
                "split" if mode == "high" else "exact")


@pytest.mark.parametrize("mode", ["medium", "HIGH", "", None])
def test_other_modes_raise(mode):
    ops.set_fp32_precision("high")
    with pytest.raises(ValueError):
        ops.set_fp32_precision(mode)
    assert ops.get_fp32_precision() == "high"  # a refused call changes nothing


def test_config_key():
    assert cfg.TRAIN.FP32_PRECISION == "highest"


@pytest.mark.parametrize("value,mode", [(None, "highest"), ("high", "high"),
                                        ("High", "highest")])
def test_environment_variable(value, mode):
    """What a new interpreter reports on import: exactly "high" is on."""
    env = {k: v for k, v in os.environ.items()
           if k != "DISTRIBUUUU_FP32_PRECISION"}
    if value is not None:
        env["DISTRIBUUUU_FP32_PRECISION"] = value
    out = subprocess.run(
        [sys.executable, "-c",
         "from distribuuuu_amd import ops; print(ops.get_fp32_precision())"],
        cwd=REPO, env=env, check=True, capture_output=True, text=True)
    assert out.stdout.strip().splitlines()[-1] == mode


def test_setup_seed_applies_the_config_key(tmp_path):
    from distribuuuu_amd import utils

    import torch

    saved = cfg.clone()
    det = ops.is_deterministic()
    cudnn = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    try:
        cfg.defrost()
        cfg.OUT_DIR = str(tmp_path)
        cfg.RNG_SEED = None
        cfg.TRAIN.FP32_PRECISION = "high"
        utils.setup_seed(0)
        assert ops.get_fp32_precision() == "high"
    finally:
        cfg.defrost()
        cfg.merge_from_other_cfg(saved)
        ops.set_deterministic(det)
        (torch.backends.cudnn.deterministic,
         torch.backends.cudnn.benchmark) = cudnn
