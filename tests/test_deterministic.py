"""Deterministic-mode switch (docs/DETERMINISM.md): the Python-side API and
its wiring into ``setup_seed``. No GPU needed — the switch keeps a Python copy
of the flag when the HIP extension is absent."""

import os
import subprocess
import sys

import pytest

from distribuuuu_amd import ops, utils
from distribuuuu_amd.config import cfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _flag_off(monkeypatch):
    """Every test starts and ends with the mode off, whatever the shell set."""
    monkeypatch.delenv("DISTRIBUUUU_DETERMINISTIC", raising=False)
    ops.set_deterministic(False)
    yield
    ops.set_deterministic(False)


@pytest.fixture
def seed_cfg(tmp_path):
    """A defrosted cfg with OUT_DIR in a temp dir; restored afterwards."""
    import torch

    saved = cfg.clone()
    cudnn = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    rng = torch.get_rng_state()
    cfg.defrost()
    cfg.OUT_DIR = str(tmp_path)
    yield cfg
    cfg.defrost()
    cfg.merge_from_other_cfg(saved)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = cudnn
    torch.set_rng_state(rng)


def _fresh_process_flag(env_value):
    """ops.is_deterministic() as a new interpreter reports it on import."""
    env = {k: v for k, v in os.environ.items()
           if k != "DISTRIBUUUU_DETERMINISTIC"}
    if env_value is not None:
        env["DISTRIBUUUU_DETERMINISTIC"] = env_value
    out = subprocess.run(
        [sys.executable, "-c",
         "from distribuuuu_amd import ops; print(ops.is_deterministic())"],
        cwd=REPO, env=env, check=True, capture_output=True, text=True)
    return out.stdout.strip().splitlines()[-1]


def test_default_is_off():
    assert ops.is_deterministic() is False
    assert _fresh_process_flag(None) == "False"
    assert _fresh_process_flag("0") == "False"


def test_environment_variable_turns_it_on():
    assert _fresh_process_flag("1") == "True"


@pytest.mark.parametrize("value", ["10", "1 "])
def test_environment_variable_only_exact_one(value):
    """One rule with and without the built extension: only "1" is on."""
    assert _fresh_process_flag(value) == "False"


def test_set_round_trips():
    e = ops.ext()  # None on a box without the built extension
    for flag in (True, False, 1):  # truthy values are accepted
        ops.set_deterministic(flag)
        assert ops.is_deterministic() is bool(flag)
        if e is not None:
            assert e.is_deterministic() is bool(flag)


def test_setup_seed_config_switch_on(seed_cfg):
    seed_cfg.CUDNN.DETERMINISTIC = True
    utils.setup_seed()
    assert ops.is_deterministic() is True


def test_setup_seed_default_config_switches_off(seed_cfg):
    assert seed_cfg.CUDNN.DETERMINISTIC is False  # the default
    ops.set_deterministic(True)
    utils.setup_seed()
    assert ops.is_deterministic() is False


def test_rng_seed_alone_keeps_fast_kernels(seed_cfg):
    seed_cfg.RNG_SEED = 1
    utils.setup_seed()
    assert ops.is_deterministic() is False


def test_rng_seed_with_config_switch(seed_cfg):
    seed_cfg.RNG_SEED = 1
    seed_cfg.CUDNN.DETERMINISTIC = True
    utils.setup_seed()
    assert ops.is_deterministic() is True
