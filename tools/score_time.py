"""Cost of scoring a whole-slide class map against its annotation on a 50 000^2 layer, d = 16.

Input: the 3125 x 3125 canvas and `scoring.synthetic_annotation(side, side, 200, 1000, seed=11)`: 200 rings of 1 000 vertices.
Timed with HIP events around the whole call (median of `--reps` runs after 3 warm-up calls, fresh output tensors every run):

  rasterize        scoring.rasterize_rings with the ring data and bin lists already on the device (the kept plan);
  rasterize_cold   the first call: bounding boxes, bin lists, upload, kernel (wall time, once);
  confusion        scoring.confusion with the outcome map: histogram kernel, 33 KB read-back, the wait for the status;
  accumulate       tiles.accumulate_logits of the 256 / 256 grid's logits: what the class map itself costs (the yardstick);
  numpy            wall time of the NumPy restatement (tests/test_score_host.py) on the same input, once: the CPU baseline.

The device results are compared with the restatement's before anything is timed.  `--whole` adds the wall time of
predict_full_patched (bf16 ResNet-18, 224 / 112, synthetic slide) and of score_prediction on its map.

    python tools/score_time.py [--side 50000] [--reps 25] [--whole] --out profiles/score_time.json
"""
from __future__ import annotations

import argparse
import sys
import time

D, N_CLS = 16, 5
LABELS = ["AT", "BG", "LP", "MM", "TUM"]


def main():
    import numpy as np
    import torch
    from _timing import REPO, Rows, median_ms, whole_slide_case
    sys.path.insert(0, str(REPO / "tests"))
    from test_score_host import confusion_np, rasterize_np

    from deephisto_amd import scoring, tiles
    from deephisto_amd.anno.utils import AnnoDescription

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rings", type=int, default=200)
    ap.add_argument("--vertices", type=int, default=1000)
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda:0")
    side, rows = args.side, Rows()
    dh = side // D
    cells = dh * dh

    dsc = AnnoDescription.with_known_colors({lb: (0, 0, 0) for lb in LABELS})
    records = scoring.synthetic_annotation(side, side, args.rings, args.vertices, LABELS, seed=11)
    xy, start, cls, info = scoring.annotation_rings(records, dsc, 1, side, side)
    common = dict(side=side, downscale=D, cells=cells, rings=int(info["n_rings"]), vertices=int(len(xy)))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    truth = scoring.rasterize_rings(xy, start, cls, N_CLS, dh, dh, D, dev)
    torch.cuda.synchronize()
    cold = time.perf_counter() - t0
    t0 = time.perf_counter()
    truth_np = rasterize_np(xy, start, cls, N_CLS, dh, dh, D)
    np_raster = time.perf_counter() - t0
    assert np.array_equal(truth.cpu().numpy(), truth_np), "the device label map differs from the restatement"

    # a class map of patches: the truth, with a seeded fifth of the 16 x 16-cell blocks replaced by another class and some left out
    g = torch.Generator(device="cpu").manual_seed(3)
    blocks = torch.randint(-1, N_CLS, ((dh + 15) // 16, (dh + 15) // 16), generator=g)
    keep = torch.rand(blocks.shape, generator=g) < 0.8
    coarse = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)[:dh, :dh]
    keep = keep.repeat_interleave(16, 0).repeat_interleave(16, 1)[:dh, :dh]
    pred_host = torch.where(keep & (torch.from_numpy(truth_np) >= 0), torch.from_numpy(truth_np).long(), coarse.long())
    pred = pred_host.to(dev).contiguous()
    t0 = time.perf_counter()
    counts_np, outcome_np = confusion_np(pred_host.numpy(), truth_np, N_CLS)
    np_conf = time.perf_counter() - t0
    counts, outcome = scoring.confusion(pred, truth, N_CLS, return_outcome=True)
    assert np.array_equal(counts.numpy(), counts_np) and np.array_equal(outcome.cpu().numpy(), outcome_np)

    o, n_unique = tiles.tile_grid(side, side, 256, 256, 64)
    logits = torch.randn((len(o), N_CLS), generator=torch.Generator(device=dev).manual_seed(256), device=dev) * 3
    ways = {
        "rasterize": lambda: scoring.rasterize_rings(xy, start, cls, N_CLS, dh, dh, D, dev),
        "confusion": lambda: scoring.confusion(pred, truth, N_CLS, return_outcome=True),
        "confusion_no_outcome": lambda: scoring.confusion(pred, truth, N_CLS),
        "accumulate": lambda: tiles.accumulate_logits(logits, o, 256, D, side, side),
    }
    ms = {k: median_ms(fn, args.reps) for k, fn in ways.items()}
    for k, (med, best) in ms.items():
        rows.emit(way=k, **common, reps=args.reps, median_ms=round(med, 4), min_ms=round(best, 4),
                  ratio_to_accumulate=round(med / ms["accumulate"][0], 3))
    rows.emit(way="rasterize_cold", **common, wall_ms=round(cold * 1e3, 2))
    rows.emit(way="numpy", **common, rasterize_wall_s=round(np_raster, 3), confusion_wall_s=round(np_conf, 3),
              labelled_fraction=round(float((truth_np >= 0).mean()), 4))
    if args.whole:
        from deephisto_amd.examples.predict_full_patched import predict_full_patched
        del logits
        _slide, smp, model = whole_slide_case(dev, side)
        wall = {}
        for k in range(3):   # the first round is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cmap = predict_full_patched(smp, model, 5, downscale=D)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            scoring.score_prediction(cmap, records, dsc, 1, side, side, D)
            t2 = time.perf_counter()
            wall = dict(predict_s=t1 - t0, score_s=t2 - t1)
        t0 = time.perf_counter()
        scoring.annotation_rings(records, dsc, 1, side, side)
        parse_s = time.perf_counter() - t0
        rows.emit(step="predict_full_patched + score_prediction wall", arch="resnet18", dtype="bf16", side=side, patch=224, stride=112,
                  predict_s=round(wall["predict_s"], 4), score_s=round(wall["score_s"], 4), of_which_parsing_s=round(parse_s, 4),
                  device_part_ms=round(ms["rasterize"][0] + ms["confusion"][0], 4),
                  device_part_of_predict=round((ms["rasterize"][0] + ms["confusion"][0]) / 1e3 / wall["predict_s"], 5))
    rows.write(args.out)


if __name__ == "__main__":
    main()
