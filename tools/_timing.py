"""What the *_time.py tools share: event and wall timing, the JSON-lines rows and the whole-slide case they time.  Importing it
puts the repository root on sys.path (the tools run as scripts), so it comes before any `deephisto_amd` import."""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def median_ms(fn, reps):
    """(median, min) in ms of `reps` calls of `fn`, each between two HIP events, after 3 warm-up calls."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def best_of(fn, reps):
    """Least wall time in s of `reps` synchronised calls of `fn`, after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


class Rows:
    """The measurements of one run: `emit` prints a row as JSON and keeps it, `write` saves them as JSON lines."""

    def __init__(self, **common):
        self.common, self.rows = common, []   # `common`: keys that lead every row

    def emit(self, **kw):
        self.rows.append({**self.common, **kw})
        print(json.dumps(self.rows[-1]), flush=True)

    def write(self, path, mode="w"):
        if path:
            Path(path).parent.mkdir(parents=True, exist_ok=True)
            with open(path, mode) as f:
                f.write("".join(json.dumps(r) + "\n" for r in self.rows))


def whole_slide_case(dev, side=50000, arch="resnet18", dtype="bf16", patch=224, stride=112, batch=64):
    """(slide, sampler, model): the closed-form `side`^2 slide in HBM, its dense sampler and a seeded model in eval mode."""
    import torch

    from deephisto_amd import tiles
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    slide = tiles.synth_slide(side, side, 0, dev)
    smp = FullImageDenseSampler(slide, layer=1, patch_size=patch, batch_size=batch, stride=stride, device=dev)
    torch.manual_seed(0)
    return slide, smp, get_model(5, dtype, arch=arch).to(dev).eval()
