"""Cost of the distance maps of a whole-slide class map on canvases of 3125 x 3125 cells (a 50 000^2
layer, d = 16) and 12 500 x 12 500 cells (d = 4).

Masks at each size: `blobs`, the boundaries of the discs of tests/test_regions_host.py's `blob_map` (one tile of them repeated);
`corner`, a single feature cell in the bottom right corner (every row of the row pass scans to its far end); `full`.  Timed with
HIP events around the whole call (median and least of `--reps` runs after 3 warm-up calls, and the spread between them):

  class_mask    dh_class_mask, the boundary mode, on the blob map (the call waits for its status word);
  transform     dh_distance_transform with the index map, per mask (`transform_d2_only`: nearest = NULL); the split between the
                column and the row pass is read off a `rocprofv3 --kernel-trace --stats` run of this tool (--reps 5 --no-scipy);
  margin_bands  distance.margin_bands([-500, 0, 500]) end to end on the blob map: two masks, two transforms, the comparisons;
  tolerant      distance.tolerant_score(tolerance 32 px) end to end against the blob map shifted by (2, -3) cells;
  scipy         wall time of scipy.ndimage.distance_transform_edt(..., return_indices=True) on the same mask on the host, once,
                if scipy is installed.

The device results are compared before anything is timed: `corner` and `full` with their closed forms, `blobs` with scipy's
squared distances (when installed).

    python tools/distance_time.py [--reps 25] [--sides 3125 12500] --out profiles/distance_time.json
"""
from __future__ import annotations

import argparse
import sys
import time


def main():
    import numpy as np
    import torch
    from _timing import REPO, Rows, median_ms
    sys.path.insert(0, str(REPO / "tests"))
    from test_distance_host import tiled_blob_map

    from deephisto_amd import distance

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--sides", type=int, nargs="+", default=[3125, 12500])
    ap.add_argument("--no-scipy", action="store_true", help="leave out the host run of scipy")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = Rows()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if args.no_scipy:
        ndimage = None

    for side in args.sides:
        d = 50000 // side
        pred_np = tiled_blob_map((side, side), 8, tile=(625, 625))
        pred = torch.from_numpy(pred_np).to(dev)
        truth = torch.roll(pred, (2, -3), (0, 1)).to(torch.int32).contiguous()
        blobs = distance.class_mask(pred, range(5), mode="boundary")
        corner = torch.zeros((side, side), dtype=torch.uint8, device=dev)
        corner[side - 1, side - 1] = 1
        masks = dict(blobs=blobs, corner=corner, full=torch.ones((side, side), dtype=torch.uint8, device=dev))

        # the results first
        r = (side - 1 - torch.arange(side, device=dev, dtype=torch.int32)) ** 2
        d2, near = distance.distance_transform(corner, return_nearest=True)
        assert torch.equal(d2, r[:, None] + r[None, :]) and bool((near == side * side - 1).all()), "corner: not the closed form"
        d2, near = distance.distance_transform(masks["full"], return_nearest=True)
        assert not bool(d2.any()) and torch.equal(near.flatten(), torch.arange(side * side, device=dev, dtype=torch.int32))
        del d2, near, r
        scipy_s = {}
        if ndimage is not None:
            for name, m in masks.items():
                host = m.cpu().numpy() == 0
                t0 = time.perf_counter()
                iy, ix = ndimage.distance_transform_edt(host, return_distances=False, return_indices=True)
                scipy_s[name] = time.perf_counter() - t0
                if name == "blobs":
                    y, x = np.mgrid[0:side, 0:side]
                    want = (iy.astype(np.int64) - y) ** 2 + (ix.astype(np.int64) - x) ** 2
                    assert np.array_equal(distance.distance_transform(m).cpu().numpy(), want), "blobs: not scipy's squared distances"
                    del y, x, want
                del iy, ix, host

        common = dict(side=side, cells=side * side, downscale=d, reps=args.reps)

        def emit(way, fn, **extra):
            med, best = median_ms(fn, args.reps)
            rows.emit(way=way, **common, **extra, median_ms=round(med, 4), min_ms=round(best, 4), spread=round(med / best - 1, 4))
            return med

        emit("class_mask", lambda: distance.class_mask(pred, range(5), mode="boundary"), mask="blobs")
        med = {}
        for name, m in masks.items():
            features = int(m.sum())
            med[name] = emit("transform", lambda m=m: distance.distance_transform(m, return_nearest=True), mask=name, features=features,
                             scipy_wall_s=None if name not in scipy_s else round(scipy_s[name], 3))
            emit("transform_d2_only", lambda m=m: distance.distance_transform(m), mask=name, features=features)
        rows.emit(way="corner_over_blobs", **common, ratio=round(med["corner"] / med["blobs"], 2))
        emit("margin_bands", lambda: distance.margin_bands(pred, [1, 3], [-500, 0, 500], d), mask="blobs")
        labels = ["a", "b", "c", "d", "e"]
        emit("tolerant_score", lambda: distance.tolerant_score(pred, truth, labels, 32, d), mask="blobs")
        del pred, truth, blobs, corner, masks
        torch.cuda.empty_cache()
    rows.write(args.out)


if __name__ == "__main__":
    main()
