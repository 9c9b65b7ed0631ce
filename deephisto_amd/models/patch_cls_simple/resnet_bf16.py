"""ResNet-50 patch classifier (BASELINE.json configs[4]) on the bf16 engine.

`get_model(n_classes, arch="resnet50")` returns `ResNet50HIP`: an `nn.Module` with torchvision's ResNet-50 `state_dict` layout
(Bottleneck x [3,4,6,3], `fc = Linear(2048, n_classes)`) whose forward, backward and optimizer step run in the bf16 engine of
libdeephisto_hip.so (`dh_train2_*`: bf16 activations, bf16 MFMA with f32 accumulation for forward, dgrad and wgrad; f32 master
weights, gradients and Adam).  The factory is models/patch_cls_simple/model.py:5-11 with a ResNet-50 backbone.  Whole-slide
prediction (`forward_tiles`, `lane_handles`) runs on the inference handle `dh_resnet50_*`, which folds eval BN into the weights;
`forward` in eval mode keeps the training engine's eval route.  The shared handle protocol lives in engine.py.
"""
from __future__ import annotations

import ctypes as C

import torch.nn as nn

from ..._lib import lib
from .engine import ResNetHIP, _Train2Trainer


class _BottleneckParams(nn.Module):
    def __init__(self, cin, width, stride):
        super().__init__()
        cout = 4 * width
        self.conv1 = nn.Conv2d(cin, width, 1, 1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, 0, bias=False), nn.BatchNorm2d(cout))


_R50_STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))


def _stages():
    cin = 64
    for w, n, s in _R50_STAGES:
        yield [_BottleneckParams(cin, w, s)] + [_BottleneckParams(4 * w, w, 1) for _ in range(n - 1)]
        cin = 4 * w


class ResNet50HIP(ResNetHIP):
    """ResNet-50 patch classifier on the bf16 engine."""

    ABI = "dh_resnet50"
    MAX_TILES = 1024   # DH_RESNET50_MAX_TILES: tiles per dh_resnet50_forward_tiles call

    def __init__(self, n_classes: int):
        super().__init__(n_classes, "bf16", _stages(), 2048)

    def _create_handle(self, h):
        return lib().dh_resnet50_create(C.byref(h), self.n_classes)

    def _new_trainer(self):
        return _Train2Trainer(self, "resnet50")

    def _forward_eval(self, x):
        # the training engine's eval route: BN from the running statistics, not folded (forward_infer / forward_tiles fold it)
        return self._engine.forward(self._input(x), False)
