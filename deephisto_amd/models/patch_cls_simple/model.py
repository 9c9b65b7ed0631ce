"""`get_model(n_classes)` -- drop-in for models/patch_cls_simple/model.py:5-11.

The reference returns torchvision's ResNet-18 with `fc` swapped for `nn.Linear(512, n_classes)`.  `ResNet18HIP` has the same
`state_dict` keys/shapes (so `best_model.pth` files interchange, examples/predict_full_patched.py:116-126) and runs entirely in
the hand-written HIP kernels of libdeephisto_hip.so: eval forwards on the `dh_resnet18` inference handle (float32 or bf16 MFMA),
training on the float32 engine (`dh_resnet18_train_*`) or, in bf16, on the `dh_train2` engine.  The handle protocol, the autograd
bridge and the fused `train_step` are shared with ResNet-50 in engine.py.

Pretrained ImageNet weights (`ResNet18_Weights.DEFAULT` in the reference) are a download and unobtainable offline: parameters get
torchvision's random initialisation; load a checkpoint with `load_state_dict` for real use.
"""
from __future__ import annotations

import ctypes as C

import torch.nn as nn

from ..._lib import DH_DTYPE_BF16, DH_DTYPE_F32, lib
from .ddp import allreduce_mean_  # noqa: F401  (re-exported)
from .engine import ResNetHIP, _F32Trainer, _Train2Trainer, ce_loss  # noqa: F401  (ce_loss re-exported)
from .resnet_bf16 import ResNet50HIP

_STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))


class _BlockParams(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, 0, bias=False),
                                            nn.BatchNorm2d(cout))


def _stages():
    cin = 64
    for c, s in _STAGES:
        yield [_BlockParams(cin, c, s), _BlockParams(c, c, 1)]
        cin = c


class ResNet18HIP(ResNetHIP):
    """ResNet-18 patch classifier; eval forward = dh_resnet18_forward (gfx950 MFMA kernels)."""

    ABI = "dh_resnet18"

    def __init__(self, n_classes: int, compute_dtype: str = "f32"):
        if compute_dtype not in ("f32", "bf16"):
            raise ValueError("compute_dtype must be 'f32' or 'bf16'")
        super().__init__(n_classes, compute_dtype, _stages(), 512)

    @property
    def MAX_TILES(self) -> int:
        """Tiles per forward_tiles launch: 4 096 in bf16 (the library's maximum), 1 024 in float32 (32-bit offsets of the conv
        tables)."""
        return 4096 if self.compute_dtype == "bf16" else 1024

    def _create_handle(self, h):
        return lib().dh_resnet18_create(C.byref(h), self.n_classes, DH_DTYPE_BF16 if self.compute_dtype == "bf16" else DH_DTYPE_F32)

    def _new_trainer(self):
        # bf16: bf16 activations / MFMA with f32 masters on the dh_train2 engine
        return _F32Trainer(self) if self.compute_dtype == "f32" else _Train2Trainer(self, "resnet18")

    def _forward_eval(self, x):
        return self.forward_infer(x)

    def _bf16_engine(self):
        """The bf16 trainer (a model built with compute_dtype="bf16")."""
        if self.compute_dtype != "bf16":
            raise RuntimeError("the bf16 training engine needs compute_dtype='bf16'")
        return self._engine

    def set_compute_dtype(self, compute_dtype: str):
        """Switch the inference handles and the training engine to another compute dtype.  The parameters are kept; the Adam
        moments (and step count) start afresh on the new engine."""
        if compute_dtype != self.compute_dtype:
            self.pull_parameters()
            self._release()
            self.compute_dtype = compute_dtype
            self._engine = self._new_trainer()
        return self


def get_model(n_classes: int, compute_dtype: str = "f32", arch: str = "resnet18") -> nn.Module:
    """Same call as the reference's `get_model(n_classes)` (model.py:5).  `arch="resnet50"` selects the ResNet-50
    backbone of BASELINE.json configs[4] (bf16 engine, whatever `compute_dtype` says)."""
    if arch == "resnet18":
        return ResNet18HIP(n_classes, compute_dtype)
    if arch == "resnet50":
        return ResNet50HIP(n_classes)
    raise ValueError(f"unknown architecture {arch!r} (resnet18, resnet50)")


ARCHS = ("resnet18", "resnet50")


def detect_arch(state_dict) -> str:
    """Backbone of a checkpoint from its keys: a bottleneck's third convolution (`layer1.0.conv3.weight`) means ResNet-50."""
    return "resnet50" if "layer1.0.conv3.weight" in state_dict else "resnet18"


def resolve_arch(arch, state_dict=None) -> str:
    """`arch` None / "auto": read it from `state_dict` (ResNet-18 without one, as the reference); an explicit arch must match the
    checkpoint's keys."""
    if arch not in (None, "auto") and arch not in ARCHS:
        raise ValueError(f"unknown architecture {arch!r} (auto, {', '.join(ARCHS)})")
    found = detect_arch(state_dict) if state_dict is not None else None
    if arch in (None, "auto"):
        return found or "resnet18"
    if found is not None and found != arch:
        raise ValueError(f"--arch {arch} does not match the checkpoint, whose keys are those of a {found} "
                         f"({'has' if found == 'resnet50' else 'lacks'} layer1.0.conv3.weight)")
    return arch
