"""Cost of the probability finish on a 50 000^2 slide's logits, d = 16.

For 256 / 256 (38 464 rows) and 224 / 112 (198 976 rows, 198 916 unique) seeded logits in HBM are finished three ways, each
timed with HIP events around the whole call (warm plan cache, median of `--reps` runs, fresh output tensors every run):

  parent   tiles.accumulate_logits: ordered logit sums + argmax, what the class map costs (the yardstick);
  fused    tiles.accumulate_probabilities: softmax rows + sums/counts with the finish in the same pass (the default);
  unfused  tiles.accumulate_probabilities(finish=False).finish(): softmax rows + sums/counts, then dh_finish_mean.

Bytes per cell the algorithm must move at 5 classes (zero-filling of fresh tensors left out on every side): parent 40 (canvas
read + write) + 28 (argmax) = 68; unfused 48 (sums + counts read + write) + 24 + 32 (finish) = 104; fused 48 + 12 (map and
confidence writes) = 60.  The achieved rate is those bytes over the measured time.  `--whole` adds the wall time of
predict_full_patched (bf16 ResNet-18, 224 / 112, synthetic slide) with and without return_proba.

    python tools/proba_time.py [--side 50000] [--reps 25] [--whole] --out profiles/proba_time.json
"""
from __future__ import annotations

import argparse
import time

D, N_CLS = 16, 5
BYTES_PER_CELL = {"parent": 68, "fused": 60, "unfused": 104}


def main():
    import torch
    from _timing import Rows, median_ms, whole_slide_case

    from deephisto_amd import tiles

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda:0")
    side, rows = args.side, Rows()
    cells = (side // D) ** 2

    for P, S in ((256, 256), (224, 112)):
        o, n_unique = tiles.tile_grid(side, side, P, S, 64)
        logits = torch.randn((len(o), N_CLS), generator=torch.Generator(device=dev).manual_seed(P), device=dev) * 3
        ways = {
            "parent": lambda: tiles.accumulate_logits(logits, o, P, D, side, side),
            "fused": lambda: tiles.accumulate_probabilities(logits, o, P, D, side, side),
            "unfused": lambda: tiles.accumulate_probabilities(logits, o, P, D, side, side, finish=False).finish(),
        }
        ms = {k: median_ms(fn, args.reps) for k, fn in ways.items()}
        a, b = ways["fused"](), ways["unfused"]()
        assert torch.equal(a.proba, b.proba) and torch.equal(a.class_map, b.class_map) and torch.equal(a.count, b.count)
        for k, (med, best) in ms.items():
            rows.emit(way=k, side=side, patch=P, stride=S, downscale=D, rows=len(o), unique_rows=n_unique, cells=cells, reps=args.reps,
                      median_ms=round(med, 4), min_ms=round(best, 4), ratio_to_parent=round(med / ms["parent"][0], 3),
                      bytes_per_cell=BYTES_PER_CELL[k], gb_per_s=round(BYTES_PER_CELL[k] * cells / (med / 1e3) / 1e9, 1))
        del logits
    if args.whole:
        from deephisto_amd.examples.predict_full_patched import predict_full_patched
        _slide, smp, model = whole_slide_case(dev, side)
        wall = {}
        for flag in (False, True, False, True):   # alternated; the first pair is the warm-up
            t0 = time.perf_counter()
            predict_full_patched(smp, model, 5, downscale=D, return_proba=flag)
            torch.cuda.synchronize()
            wall[flag] = time.perf_counter() - t0
        rows.emit(step="predict_full_patched wall", arch="resnet18", dtype="bf16", side=side, patch=224, stride=112,
                  without_proba_s=round(wall[False], 4), with_proba_s=round(wall[True], 4),
                  difference_ms=round((wall[True] - wall[False]) * 1e3, 2))
    rows.write(args.out)


if __name__ == "__main__":
    main()
