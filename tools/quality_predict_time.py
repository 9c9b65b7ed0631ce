"""Cost of the tile quality filter on a 50 000^2 slide at 224 / 112.

The closed-form slide in HBM with a fixed, seeded pattern of 1 000^2 blocks worked over by torch ops: a quarter of them
box-blurred 5 x 5, 15 % painted flat blue (20, 60, 200), 5 % painted flat (10, 10, 10).  The closed-form slide is hash noise
(sharpness about 16 000, about 42 % of its pixels pass the ink rule), so the filter here is QualityFilter(min_sharpness=4000,
max_ink_fraction=0.6): thresholds for this picture, not for a scan.  Three modes:

  --mode time     the quality step alone (sums, flags, compaction with its one read-back, and the download of the sums and
                  reasons for the report: what predict_full_patched runs), one warm-up then `--reps` timed runs (best, wall);
                  whole-slide predict_full_patched with bf16 ResNet-18 unfiltered (`quality=None`, which is the parent's code
                  path untouched) and filtered, timed the same way; the step's share of the unfiltered prediction against
                  the 3 % budget of a scoring step;
  --mode kernels  only the quality step, `--reps` times: run it under `rocprofv3 --kernel-trace --stats` for kernel times;
  --mode merge    reads that run's kernel_stats.csv (`--stats`) and appends per-kernel ms and achieved GB/s (bytes the kernel
                  loads, and the slide's bytes once) against the 6.29 TB/s measured copy rate to `--out`.

    python tools/quality_predict_time.py --mode time [--side 50000] [--reps 2] --out profiles/quality_predict_time.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o quality -- python tools/quality_predict_time.py --mode kernels
    python tools/quality_predict_time.py --mode merge --stats OUT/.../quality_kernel_stats.csv --out profiles/quality_predict_time.json
"""
from __future__ import annotations

import argparse
import csv
import json
from pathlib import Path

COPY_RATE = 6.29e12   # bytes/s, the float4 copy rate measured on the MI355X (6.3 TB/s)
P, S, D = 224, 112, 16
BLOCK = 1000
BAND = 16             # csrc/quality.hip kBand
MIN_SHARPNESS, MAX_INK = 4000, 0.6


def painted_slide(side: int, dev):
    import torch
    import torch.nn.functional as F

    from deephisto_amd import tiles
    slide = tiles.synth_slide(side, side, 0, dev)
    g = torch.Generator().manual_seed(1234)
    nb = -(-side // BLOCK)
    kind = torch.rand((nb, nb), generator=g)
    blue = torch.tensor((20, 60, 200), dtype=torch.uint8, device=dev)
    for by in range(nb):
        for bx in range(nb):
            blk = slide[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK]
            k = float(kind[by, bx])
            if k < 0.25:
                f = blk.permute(2, 0, 1).float()[None]
                f = F.avg_pool2d(F.pad(f, (2, 2, 2, 2), mode="replicate"), 5, stride=1)
                blk.copy_(f[0].round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0))
            elif k < 0.40:
                blk[:] = blue
            elif k < 0.45:
                blk[:] = 10
    torch.cuda.synchronize(dev)
    return slide


def step(slide, smp, filt, dev):
    import torch

    from deephisto_amd import quality
    o = smp.origins[:smp.n_tiles]
    _, _, info = quality.score_quality(slide, torch.from_numpy(o).to(dev), P, -1, filt, o)
    return info


def main():
    import torch
    from _timing import Rows, best_of

    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    from deephisto_amd.quality import QualityFilter, sharpness_summary

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "kernels", "merge"], default="time")
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = Rows()

    if args.mode == "merge":
        side = args.side
        n_tiles = None
        if args.out and Path(args.out).exists():
            for ln in Path(args.out).read_text().splitlines():
                r = json.loads(ln)
                n_tiles = r.get("n_tiles", n_tiles)
        n_tiles = n_tiles or 198916
        # what quality_stats_kernel loads: per tile and band of 16 rows, (rows + 2) x (P + 2) pixels of 3 bytes; then 8 bytes of
        # origin in and 32 bytes of sums out per tile.  Most of it comes from L2: neighbouring tiles overlap by half
        loaded = n_tiles * (sum((min(BAND, P - b) + 2) * (P + 2) * 3 for b in range(0, P, BAND)) + 40)
        need = {"quality_stats_kernel": loaded, "quality_flags_kernel": 37 * n_tiles, "tissue_select_kernel": 24 * n_tiles}
        total_ms = 0.0
        with open(args.stats) as f:
            for r in csv.DictReader(f):
                name = next((k for k in need if k in r["Name"]), None)
                if name is None:
                    continue
                ms = float(r["AverageNs"]) / 1e6
                total_ms += ms
                gbs = need[name] / (ms / 1e3) / 1e9
                row = dict(kernel=name, calls=int(r["Calls"]), avg_ms=round(ms, 4), bytes_loaded=need[name], gb_per_s=round(gbs, 1),
                           fraction_of_copy_rate=round(gbs * 1e9 / COPY_RATE, 3))
                if name == "quality_stats_kernel":
                    once = 3 * side * side
                    row.update(slide_bytes=once, slide_once_gb_per_s=round(once / (ms / 1e3) / 1e9, 1),
                               slide_once_fraction_of_copy_rate=round(once / (ms / 1e3) / COPY_RATE, 3))
                rows.emit(**row)
        rows.emit(kernel="all kernels of the quality step", avg_ms=round(total_ms, 4))
        rows.write(args.out, "a")
        return

    dev = torch.device("cuda:0")
    slide = painted_slide(args.side, dev)
    smp = FullImageDenseSampler(slide, layer=1, patch_size=P, batch_size=64, stride=S, device=dev)
    filt = QualityFilter(min_sharpness=MIN_SHARPNESS, max_ink_fraction=MAX_INK)
    if args.mode == "kernels":
        for _ in range(args.reps + 1):
            step(slide, smp, filt, dev)
        torch.cuda.synchronize()
        return
    info: dict = {}
    step_s = best_of(lambda: info.update(step(slide, smp, filt, dev)), args.reps)
    kept_frac = info["n_kept"] / info["n_tiles"]
    rows.emit(step="quality (sums, flags, compaction, read-back; wall)", side=args.side, patch=P, stride=S, n_tiles=info["n_tiles"],
              n_kept=info["n_kept"], kept_fraction=round(kept_frac, 4), rejected_blur=info["rejected_blur"],
              rejected_ink=info["rejected_ink"], min_sharpness=MIN_SHARPNESS, max_ink_pixels=info["max_ink_pixels"],
              sharpness=sharpness_summary(info["stats"]), seconds=round(step_s, 5))
    torch.manual_seed(0)
    model = get_model(5, "bf16", arch="resnet18").to(dev).eval()
    full_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=D), args.reps)
    filt_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=D, quality=filt), args.reps)
    rows.emit(arch="resnet18", dtype="bf16", side=args.side, patch=P, stride=S, n_tiles=info["n_tiles"], n_kept=info["n_kept"],
              kept_fraction=round(kept_frac, 4), unfiltered_s=round(full_s, 4), filtered_s=round(filt_s, 4),
              ratio=round(filt_s / full_s, 4), quality_step_s=round(step_s, 5),
              step_fraction_of_unfiltered=round(step_s / full_s, 4), step_within_3pct=step_s <= 0.03 * full_s)
    rows.write(args.out)


if __name__ == "__main__":
    main()
