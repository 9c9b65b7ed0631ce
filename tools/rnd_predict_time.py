"""Time the random sampler's branch at the reference's geometry (FullImageRndSampler, device index logic).

50 000^2 synthetic slide in HBM, patch 224, batch 64, dense_level 2, speedup 16 (3 125^2 coverage cells).  Reports
batches / tiles to full coverage, sampler-only patches/s (origins on the device, no forward), predict_random_patched
end to end in bf16 and f32, host ms per batch (planning + step + counter read-back) and the span of HIP events around
one batch on the map's stream (`gpu_ms_per_batch_span`: planning included, the step is queued after it; not kernel-only
time), and the NumPy index logic's cost per batch over its first 5 batches.  One JSON line per measurement.

    python tools/rnd_predict_time.py [--side 50000] [--seed 0] [--out profiles/rnd_predict_time.json]
"""
from __future__ import annotations

import argparse
import time


def main():
    import numpy as np
    import torch
    from _timing import Rows

    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import predict_random_patched
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    side, P, B, dl, d = args.side, args.patch, args.batch, 2, 16
    slide = tiles.synth_slide(side, side, 0, dev)
    torch.cuda.synchronize()
    rows = Rows(side=side, patch=P, batch=B, dense_level=dl, speedup=d)

    def mk(logic):
        return FullImageRndSampler(slide, layer=1, patch_size=P, batch_size=B, dense_level=dl, speedup=d, index_logic=logic)

    # sampler only: origins stay on the device; per-batch host time (planning + step + counters) and GPU time
    np.random.seed(args.seed)
    smp = mk("device")
    ev = []
    t0 = time.perf_counter()
    n = 0
    host_plan = 0.0
    gen = smp._device_origin_batches(host_origins=False)
    while True:
        th = time.perf_counter()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            next(gen)
        except StopIteration:
            break
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        if n % 16 == 0:
            ev.append((e0, e1))
        host_plan += time.perf_counter() - th
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gpu_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    rows.emit(what="sampler_only", batches=n, tiles=n * B, filled=smp._filled_ratio[-1], seconds=round(dt, 3),
              patches_per_s=round(n * B / dt), host_ms_per_batch=round(1e3 * host_plan / n, 4),
              gpu_ms_per_batch_span=round(gpu_ms, 4), stats=repr(smp.planner.stats))
    n_batches = n

    # end to end
    for dtype in ("bf16", "f32"):
        torch.manual_seed(0)
        model = get_model(5, dtype).to(dev).eval()
        np.random.seed(args.seed)
        predict_random_patched(mk("device"), model, 5, d)          # warm-up (kernels, workspaces)
        torch.cuda.synchronize()
        np.random.seed(args.seed)
        timing = {}
        t0 = time.perf_counter()
        predict_random_patched(mk("device"), model, 5, d, timing=timing)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows.emit(what=f"predict_random_patched_{dtype}", batches=timing["n_batches"], tiles=timing["n_tiles"], seconds=round(dt, 3),
                  patches_per_s=round(timing["n_tiles"] / dt), host_loop_s=round(timing["host_s"], 3))
        assert timing["n_batches"] == n_batches
        del model
        torch.cuda.empty_cache()

    # the NumPy index logic, first 5 batches
    np.random.seed(args.seed)
    smp = mk("numpy")
    it = smp._numpy_origin_batches()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        next(it)
        t.append(time.perf_counter() - t0)
    rows.emit(what="numpy_index_logic_first5", ms_per_batch=[round(1e3 * x, 1) for x in t],
              patches_per_s=round(5 * B / sum(t), 1))
    rows.write(args.out)


if __name__ == "__main__":
    main()
