"""Cost and benefit of the tissue filter on a 50 000^2 slide at 224 / 112.

The closed-form slide in HBM with a fixed, seeded glass pattern painted over it by torch ops: white (255) blocks of 1 000^2 pixels
over about half the area and a low-chroma grey band (chroma 4) that Otsu's threshold must reject.  Three modes:

  --mode time     whole-slide predict_full_patched with bf16 ResNet-18 and ResNet-50, unmasked and with TissueFilter("otsu"),
                  one warm-up then `--reps` timed runs (best); the scoring step alone (histogram, Otsu, counts, compaction,
                  fill) timed the same way; kept fraction, masked / unmasked ratio and the two bounds of the issue;
  --mode kernels  only the scoring step, `--reps` times: run it under `rocprofv3 --kernel-trace --stats` for kernel times;
  --mode merge    reads that run's kernel_stats.csv (`--stats`) and appends per-kernel ms and achieved GB/s (bytes the
                  algorithm must move, over kernel time) against the 6.29 TB/s measured copy rate to `--out`.

    python tools/tissue_predict_time.py --mode time [--side 50000] [--reps 2] --out profiles/tissue_predict_time.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o tissue -- python tools/tissue_predict_time.py --mode kernels
    python tools/tissue_predict_time.py --mode merge --stats OUT/.../tissue_kernel_stats.csv --out profiles/tissue_predict_time.json
"""
from __future__ import annotations

import argparse
import csv
import json
from pathlib import Path

COPY_RATE = 6.29e12   # bytes/s, the float4 copy rate measured on the MI355X (6.3 TB/s)
P, S, D = 224, 112, 16
BLOCK = 1000
GREY = (200, 196, 198)


def painted_slide(side: int, dev):
    import torch

    from deephisto_amd import tiles
    slide = tiles.synth_slide(side, side, 0, dev)
    g = torch.Generator().manual_seed(1234)
    nb = -(-side // BLOCK)
    glass = torch.rand((nb, nb), generator=g) < 0.5
    for by in range(nb):
        for bx in range(nb):
            if glass[by, bx]:
                slide[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK] = 255
    band = side * 45 // 100
    slide[band:band + side // 20] = torch.tensor(GREY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    return slide


def score(slide, smp, filt, dev):
    import torch

    from deephisto_amd import tissue
    o = smp.origins[:smp.n_tiles]
    idx, yx, info = tissue.score_tiles(slide, torch.from_numpy(o).to(dev), P, filt, o)
    cmap = torch.zeros((smp.h // D, smp.w // D), dtype=torch.int64, device=dev)
    tissue.fill_uncovered(cmap, yx, P, D, smp.h, smp.w, filt.fill_class)
    return info


def main():
    import torch
    from _timing import Rows, best_of

    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    from deephisto_amd.tissue import TissueFilter

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
        npix = side * side
        n_tiles = None
        if args.out and Path(args.out).exists():
            for ln in Path(args.out).read_text().splitlines():
                r = json.loads(ln)
                n_tiles = r.get("n_tiles", n_tiles)
        n_tiles = n_tiles or 198916
        # bytes each pass must move at least: the slide (3 B/pixel) per slide pass; the bitmap (1 bit/pixel) written once and
        # read at least once; 4 B count + 8 B origin per tile (read, and written again for the kept ones); the uint8 coverage map
        # (the fill pass writes only the uncovered cells of the int64 class map, a count this step does not know)
        cells = (side // D) ** 2
        need = {"tissue_hist_kernel": 3 * npix, "tissue_bitmap_kernel": 3 * npix + npix // 8,
                "tissue_count_kernel": npix // 8 + 12 * n_tiles, "tissue_select_kernel": 24 * n_tiles,
                "cover_mark_kernel": 8 * n_tiles + cells, "cover_fill_kernel": cells}
        total_ms = 0.0
        with open(args.stats) as f:
            for r in csv.DictReader(f):
                name = next((k for k in need if k in r["Name"]), None)
                if name is None:
                    continue
                ms = float(r["AverageNs"]) / 1e6
                total_ms += ms
                gbs = need[name] / (ms / 1e3) / 1e9
                rows.emit(kernel=name, calls=int(r["Calls"]), avg_ms=round(ms, 4), bytes_needed=need[name], gb_per_s=round(gbs, 1),
                          fraction_of_copy_rate=round(gbs * 1e9 / COPY_RATE, 3))
        rows.emit(kernel="all scoring passes", avg_ms=round(total_ms, 4))
        rows.write(args.out, "a")
        return

    dev = torch.device("cuda:0")
    slide = painted_slide(args.side, dev)
    smp = FullImageDenseSampler(slide, layer=1, patch_size=P, batch_size=64, stride=S, device=dev)
    filt = TissueFilter("otsu")
    if args.mode == "kernels":
        for _ in range(args.reps + 1):
            score(slide, smp, filt, dev)
        torch.cuda.synchronize()
        return
    info: dict = {}
    score_s = best_of(lambda: info.update(score(slide, smp, filt, dev)), args.reps)
    kept_frac = info["n_kept"] / info["n_tiles"]
    rows.emit(step="scoring (histogram, Otsu, counts, compaction, fill; wall)", side=args.side, patch=P, stride=S,
              n_tiles=info["n_tiles"], n_kept=info["n_kept"], kept_fraction=round(kept_frac, 4), threshold=info["threshold"],
              min_pixels=info["min_pixels"], seconds=round(score_s, 5))
    for arch, dtype in (("resnet18", "bf16"), ("resnet50", "bf16")):
        torch.manual_seed(0)
        model = get_model(5, dtype, arch=arch).to(dev).eval()
        full_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=D), args.reps)
        masked_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=D, tissue=filt), args.reps)
        bound = kept_frac * full_s + score_s + 0.05 * full_s
        rows.emit(arch=arch, dtype=dtype, side=args.side, patch=P, stride=S, n_tiles=info["n_tiles"], n_kept=info["n_kept"],
                  kept_fraction=round(kept_frac, 4), unmasked_s=round(full_s, 4), masked_s=round(masked_s, 4),
                  ratio=round(masked_s / full_s, 4), scoring_s=round(score_s, 5),
                  scoring_fraction_of_unmasked=round(score_s / full_s, 4), scoring_within_3pct=score_s <= 0.03 * full_s,
                  masked_bound_s=round(bound, 4), masked_within_bound=masked_s <= bound)
        del model
    rows.write(args.out)


if __name__ == "__main__":
    main()
