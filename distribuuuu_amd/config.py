"""Global config system.

API-parity with the reference's yacs-based config (`/root/reference/distribuuuu/config.py:7-100`):
a global frozen ``cfg`` singleton with MODEL/TRAIN/TEST/CUDNN/OPTIM groups, ``--cfg`` YAML merge,
positional ``KEY VALUE`` overrides, ``dump_cfg``/``reset_cfg``/``load_cfg_fom_args``. The schema
key names are identical so the reference's 7 YAML presets load unmodified.

Implementation is our own (yacs is not a dependency): a small attribute-dict ``CfgNode`` with
freeze/merge/dump semantics. MIOPEN is accepted as an alias group for CUDNN-style flags.
"""

import argparse
import copy
import os

import yaml


class CfgNode(dict):
    """Attribute-style nested dict with freeze / merge semantics (yacs-compatible surface)."""

    IMMUTABLE = "__immutable__"

    def __init__(self, init_dict=None):
        init_dict = init_dict or {}
        super().__init__()
        object.__setattr__(self, CfgNode.IMMUTABLE, False)
        for k, v in init_dict.items():
            self[k] = CfgNode(v) if isinstance(v, dict) else v

    # -- attribute access -------------------------------------------------
    def __getattr__(self, name):
        if name in self:
            return self[name]
        raise AttributeError(f"Config key not found: {name}")

    def __setattr__(self, name, value):
        if object.__getattribute__(self, CfgNode.IMMUTABLE):
            raise AttributeError(f"Attempted to set {name} on an immutable CfgNode")
        self[name] = value

    # -- mutability --------------------------------------------------------
    def freeze(self):
        self._set_immutable(True)

    def defrost(self):
        self._set_immutable(False)

    def is_frozen(self):
        return object.__getattribute__(self, CfgNode.IMMUTABLE)

    def _set_immutable(self, flag):
        object.__setattr__(self, CfgNode.IMMUTABLE, flag)
        for v in self.values():
            if isinstance(v, CfgNode):
                v._set_immutable(flag)

    # -- merge -------------------------------------------------------------
    def clone(self):
        node = CfgNode()
        for k, v in self.items():
            node[k] = v.clone() if isinstance(v, CfgNode) else copy.deepcopy(v)
        return node

    def merge_from_other_cfg(self, other):
        self._merge_dict(dict(other))

    def _merge_dict(self, d, prefix=""):
        was_frozen = self.is_frozen()
        if was_frozen:
            self._set_immutable(False)
        try:
            for k, v in d.items():
                full = f"{prefix}{k}"
                if k not in self:
                    raise KeyError(f"Non-existent config key: {full}")
                cur = self[k]
                if isinstance(cur, CfgNode):
                    if not isinstance(v, dict):
                        raise TypeError(f"Cannot merge non-dict into group {full}")
                    cur._merge_dict(v, prefix=full + ".")
                else:
                    self[k] = _coerce(v, cur, full)
        finally:
            if was_frozen:
                self._set_immutable(True)

    def merge_from_file(self, cfg_file):
        with open(cfg_file, "r") as f:
            d = yaml.safe_load(f) or {}
        self._merge_dict(d)

    def merge_from_list(self, opts):
        if not opts:
            return
        if len(opts) % 2 != 0:
            raise ValueError(f"Override list has odd length: {opts}")
        for key, value in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = getattr(node, p)
            leaf = parts[-1]
            if leaf not in node:
                raise KeyError(f"Non-existent config key: {key}")
            cur = node[leaf]
            if isinstance(value, str):
                try:
                    value = yaml.safe_load(value)
                except yaml.YAMLError:
                    pass
            was_frozen = self.is_frozen()
            if was_frozen:
                self._set_immutable(False)
            node[leaf] = _coerce(value, cur, key)
            if was_frozen:
                self._set_immutable(True)

    # -- dump --------------------------------------------------------------
    def to_dict(self):
        return {
            k: (v.to_dict() if isinstance(v, CfgNode) else v) for k, v in self.items()
        }

    def dump(self, stream=None, **kwargs):
        kwargs.setdefault("default_flow_style", False)
        kwargs.setdefault("sort_keys", True)
        return yaml.safe_dump(self.to_dict(), stream, **kwargs)


def _coerce(value, reference, key):
    """Validate/coerce an incoming value against the default's type."""
    if reference is None or value is None:
        return value
    if isinstance(reference, bool):
        if isinstance(value, bool):
            return value
        raise TypeError(f"Expected bool for {key}, got {type(value).__name__}")
    if isinstance(reference, float) and isinstance(value, int):
        return float(value)
    # YAML 1.1 does not parse "1e-5" as a float; accept numeric strings
    if isinstance(value, str) and isinstance(reference, (int, float)):
        try:
            num = float(value)
            return int(num) if isinstance(reference, int) else num
        except ValueError:
            pass
    if isinstance(reference, (list, tuple)) and isinstance(value, (list, tuple)):
        return list(value)
    if type(value) is type(reference):
        return value
    raise TypeError(
        f"Type mismatch for {key}: expected {type(reference).__name__}, "
        f"got {type(value).__name__} ({value!r})"
    )


# ---------------------------------------------------------------------------
# Schema — key names identical to /root/reference/distribuuuu/config.py:10-63
# so the shipped YAML presets load unmodified.
# ---------------------------------------------------------------------------
_C = CfgNode()
cfg = _C

_C.MODEL = CfgNode()
_C.MODEL.ARCH = "resnet18"
_C.MODEL.NUM_CLASSES = 1000
_C.MODEL.PRETRAINED = False
_C.MODEL.SYNCBN = False
_C.MODEL.WEIGHTS = None
_C.MODEL.DUMMY_INPUT = False

_C.TRAIN = CfgNode()
_C.TRAIN.BATCH_SIZE = 32
_C.TRAIN.IM_SIZE = 224
_C.TRAIN.DATASET = "./data/ILSVRC/"
_C.TRAIN.SPLIT = "train"
_C.TRAIN.AUTO_RESUME = True
_C.TRAIN.LOAD_OPT = True
_C.TRAIN.WORKERS = 4
_C.TRAIN.PIN_MEMORY = True
_C.TRAIN.PRINT_FREQ = 30
_C.TRAIN.TOPK = 5
# MI355X-native additions (defaults preserve reference behavior)
_C.TRAIN.DTYPE = "float32"          # "float32" | "bfloat16" (bf16 compute, fp32 master)
_C.TRAIN.CHANNELS_LAST = False       # NHWC end-to-end
_C.TRAIN.BUCKET_CAP_MB = 8           # DDP gradient bucket size, tuned for 7-link xGMI
_C.TRAIN.COMPILE_GRAPH = False       # capture the train step in a hipGraph
# soft-target training (mixing.SoftTargetCriterion); all at default = the
# plain hard-target loss and no batch mixing
_C.TRAIN.LABEL_SMOOTH = 0.0          # label smoothing eps in [0, 1)
_C.TRAIN.MIXUP_ALPHA = 0.0           # mixup: lam ~ Beta(alpha, alpha); 0 = off
_C.TRAIN.CUTMIX_ALPHA = 0.0          # CutMix box from Beta(alpha, alpha); 0 = off
_C.TRAIN.MIX_PROB = 1.0              # probability that a batch is mixed at all
_C.TRAIN.MIX_SWITCH_PROB = 0.5       # CutMix (vs mixup) when both alphas are set

_C.TEST = CfgNode()
_C.TEST.DATASET = "./data/ILSVRC/"
_C.TEST.SPLIT = "val"
_C.TEST.BATCH_SIZE = 200
_C.TEST.IM_SIZE = 256
_C.TEST.PRINT_FREQ = 10

# Kept under its reference name so preset YAMLs load; on ROCm these map to
# MIOpen/rocBLAS benchmark & determinism toggles (torch.backends.cudnn on ROCm
# drives MIOpen).
_C.CUDNN = CfgNode()
_C.CUDNN.BENCHMARK = True
_C.CUDNN.DETERMINISTIC = False

_C.OPTIM = CfgNode()
_C.OPTIM.MAX_EPOCH = 100
_C.OPTIM.LR_POLICY = "cos"           # {'cos', 'steps'}
_C.OPTIM.BASE_LR = 0.2
_C.OPTIM.MIN_LR = 0.0
_C.OPTIM.STEPS = []
_C.OPTIM.LR_MULT = 0.1
_C.OPTIM.MOMENTUM = 0.9
_C.OPTIM.DAMPENING = 0.0
_C.OPTIM.NESTEROV = True
_C.OPTIM.WARMUP_FACTOR = 0.1
_C.OPTIM.WARMUP_EPOCHS = 5
_C.OPTIM.WEIGHT_DECAY = 5e-5
_C.OPTIM.FUSED_SGD = True            # fused multi-tensor HIP SGD step on GPU
_C.OPTIM.OPTIMIZER = "sgd"           # "sgd" | "lars" (layer-wise adaptive rate)
_C.OPTIM.LARS_TRUST_COEF = 0.001     # LARS trust coefficient
_C.OPTIM.LARS_EPS = 1e-8             # added to the LARS ratio's denominator

_C.OUT_DIR = "./exp"
_C.CFG_DEST = "config.yaml"
_C.RNG_SEED = None

_CFG_DEFAULT = _C.clone()
_CFG_DEFAULT.freeze()


def merge_from_file(cfg_file):
    """Merge a YAML preset into the global cfg (reference config.py:69-72)."""
    _C.merge_from_file(cfg_file)


def dump_cfg():
    """Dump the config to OUT_DIR/CFG_DEST (reference config.py:75-79)."""
    os.makedirs(_C.OUT_DIR, exist_ok=True)
    cfg_file = os.path.join(_C.OUT_DIR, _C.CFG_DEST)
    with open(cfg_file, "w") as f:
        _C.dump(stream=f)


def reset_cfg():
    """Reset config to the default state (reference config.py:82-84)."""
    was_frozen = _C.is_frozen()
    if was_frozen:
        _C.defrost()
    for k in list(_C.keys()):
        default = _CFG_DEFAULT[k]
        _C[k] = default.clone() if isinstance(default, CfgNode) else copy.deepcopy(default)
    if was_frozen:
        _C.freeze()


def load_cfg_fom_args(description="Config file options.", argv=None):
    """Load config from CLI args: --cfg file + positional KEY VALUE overrides
    (reference config.py:87-100; --local_rank accepted and ignored for legacy launchers)."""
    parser = argparse.ArgumentParser(description=description)
    parser.add_argument("--cfg", dest="cfg_file", default=None, type=str,
                        help="Config file location")
    parser.add_argument("--local_rank", default=None,
                        help="LOCAL_RANK for legacy torch.distributed.launch")
    parser.add_argument("opts", default=None, nargs=argparse.REMAINDER,
                        help="See distribuuuu_amd/config.py for all options")
    args = parser.parse_args(argv)
    if args.cfg_file is not None:
        merge_from_file(args.cfg_file)
    if args.opts:
        _C.merge_from_list(args.opts)
