#!/usr/bin/env python3
"""Diagnostic: phase cycles of the fused bf16 stem per strip step (stamped instantiation), strip width forced to 15 and to 16 in turn.
Tooling only."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from deephisto_amd._lib import check, lib
from deephisto_amd.models.patch_cls_simple.model import get_model
from deephisto_amd import tiles
B, P = 3968, 256
dev = torch.device("cuda:0")
m = get_model(5, "bf16").to(dev).eval()
slide = tiles.synth_slide(16384, 16384, 0, dev)
o = torch.zeros((B, 2), dtype=torch.int32, device=dev)
o[:, 0] = torch.arange(B, device=dev, dtype=torch.int32) % 63 * 256
o[:, 1] = torch.arange(B, device=dev, dtype=torch.int32) // 63 % 63 * 256
m.forward_tiles(slide, o, P); torch.cuda.synchronize()
for width in (15, 16, 15, 16):
    check(lib().dh_debug_stem_strip_width(width), "width")
    m.forward_tiles(slide, o, P); torch.cuda.synchronize()
    check(lib().dh_debug_stamps(1, None), "stamps on")
    for _ in range(3):
        m.forward_tiles(slide, o, P)
    out = np.zeros(64, np.uint64)
    check(lib().dh_debug_stamps(0, out.ctypes.data), "stamps read")
    v = out[56:64].astype(np.float64)
    strips = B * (5 if width == 15 else 4) * 3
    steps = strips * 16
    tot = v[:6].sum()
    print(f"width {width}: wgs {int(v[6])}  cycles/wg {tot / v[6]:9.0f}  cycles per strip-step (wg cycles / steps): " +
          "  ".join(f"{n} {a / steps:7.1f}" for n, a in zip(["prefetch", "mfma", "bn+pack", "pool+stores", "stage", "barrier"], v[:6])) +
          f"  total {tot / steps:7.1f}", flush=True)
check(lib().dh_debug_stem_strip_width(0), "width")
