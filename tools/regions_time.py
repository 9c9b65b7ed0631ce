"""Cost of the regions of a whole-slide class map on a 3125 x 3125 canvas (a 50 000^2 layer, d = 16).

Inputs: `prediction`, the class map predict_full_patched gives for the 50 000^2 synthetic slide (bf16 ResNet-18, 224 / 112;
left out with --no-whole), and `patch14`, the seeded patch-like map of tests/test_regions_host.py (a coarse noise grid of five
classes and -1, upsampled by 14).  Timed with HIP events around the whole call (median of `--reps` runs after 3 warm-up calls):

  label        regions.label_components: seven kernels, K read back;
  table        dh_region_stats with the confidence map (device part; the table stays on the device);
  clean_round  regions.clean_map(min_cells, rounds=1): label + table + dh_clean_small_regions;
  budget       what section 4.10 holds against 3 % of the whole-slide prediction: clean_round, then label and table of the
               cleaned map;
  accumulate   tiles.accumulate_logits of the 256 / 256 grid's logits (the yardstick of sections 4.8 and 4.9);
  numpy        wall time of the NumPy restatement on the same input, once (and of scipy.ndimage.label per class, if installed);
  trace        wall time of regions.trace_polygons over every region of the cleaned map (host, NumPy), once.

The device results are compared with the restatement's before anything is timed.

    python tools/regions_time.py [--reps 25] [--min_cells 9] [--no-whole] --out profiles/regions_time.json
"""
from __future__ import annotations

import argparse
import sys
import time

D, N_CLS, SIDE = 16, 5, 50000


def main():
    import numpy as np
    import torch
    from _timing import REPO, Rows, median_ms, whole_slide_case
    sys.path.insert(0, str(REPO / "tests"))
    from test_regions_host import canvas, clean_round_np, label_np, table_np

    from deephisto_amd import regions, tiles

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--min_cells", type=int, default=9)
    ap.add_argument("--no-whole", action="store_true", help="leave out the 50 000^2 prediction (a profiling run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dh = SIDE // D
    rows = Rows()

    maps, predict_s = {}, None
    if not args.no_whole:
        from deephisto_amd.examples.predict_full_patched import predict_full_patched
        slide, smp, model = whole_slide_case(dev, SIDE)
        for _ in range(3):   # the first round is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cmap, proba = predict_full_patched(smp, model, 5, downscale=D, return_proba=True)
            torch.cuda.synchronize()
            with_proba_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            cmap = predict_full_patched(smp, model, 5, downscale=D)
            torch.cuda.synchronize()
            predict_s = time.perf_counter() - t0
        maps["prediction"] = (cmap, proba.confidence)
        rows.emit(step="predict_full_patched wall", arch="resnet18", dtype="bf16", side=SIDE, patch=224, stride=112,
                  predict_s=round(predict_s, 4), with_proba_s=round(with_proba_s, 4))
        del slide, smp, model, proba
    m14, _ = canvas("patch14", (dh, dh))
    conf14 = torch.rand((dh, dh), generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    maps["patch14"] = (torch.from_numpy(m14).to(dev), conf14)

    o, _ = tiles.tile_grid(SIDE, SIDE, 256, 256, 64)
    logits = torch.randn((len(o), N_CLS), generator=torch.Generator(device=dev).manual_seed(256), device=dev) * 3
    acc_ms = median_ms(lambda: tiles.accumulate_logits(logits, o, 256, D, SIDE, SIDE), args.reps)
    rows.emit(way="accumulate", cells=dh * dh, reps=args.reps, median_ms=round(acc_ms[0], 4), min_ms=round(acc_ms[1], 4))

    for name, (pred, conf) in maps.items():
        m = pred.cpu().numpy()
        t0 = time.perf_counter()
        lab_np, k_np = label_np(m)
        np_label = time.perf_counter() - t0
        t0 = time.perf_counter()
        tab_np = table_np(m, lab_np, k_np, conf.cpu().numpy())
        np_table = time.perf_counter() - t0
        t0 = time.perf_counter()
        clean_ref, changed_ref = clean_round_np(m, args.min_cells)
        np_clean = time.perf_counter() - t0
        scipy_s = None
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            k_sp = sum(ndimage.label(m == c)[1] for c in range(N_CLS))
            scipy_s = time.perf_counter() - t0
            assert k_sp == k_np
        except ImportError:
            pass
        labels, k = regions.label_components(pred, N_CLS)
        assert k == k_np and np.array_equal(labels.cpu().numpy(), lab_np), "the device label map differs from the restatement"
        table = regions.region_table(pred, labels, k, conf)
        assert np.array_equal(table.area, tab_np["area"]) and np.array_equal(table.conf_q, tab_np["conf_q"])
        cleaned, changed = regions.clean_map(pred, args.min_cells, 1, N_CLS)
        assert changed == changed_ref and np.array_equal(cleaned.cpu().numpy(), clean_ref)
        labels_c, k_c = regions.label_components(cleaned, N_CLS)

        def budget():
            c, _ = regions.clean_map(pred, args.min_cells, 1, N_CLS)
            lb, kk = regions.label_components(c, N_CLS)
            regions._table_dev(c, lb, kk, conf)

        ways = {
            "label": lambda: regions.label_components(pred, N_CLS),
            "table": lambda: regions._table_dev(pred, labels, k, conf),
            "clean_round": lambda: regions.clean_map(pred, args.min_cells, 1, N_CLS),
            "budget": budget,
        }
        common = dict(map=name, cells=int(m.size), regions=k, regions_after_cleanup=k_c, min_cells=args.min_cells, changed=changed)
        ms = {w: median_ms(fn, args.reps) for w, fn in ways.items()}
        for w, (med, best) in ms.items():
            extra = {}
            if w == "budget" and predict_s:
                extra = dict(share_of_predict=round(med / 1e3 / predict_s, 5), limit=0.03, within=bool(med / 1e3 / predict_s < 0.03))
            rows.emit(way=w, **common, reps=args.reps, median_ms=round(med, 4), min_ms=round(best, 4),
                      ratio_to_accumulate=round(med / acc_ms[0], 2), **extra)
        rows.emit(way="numpy", **common, label_wall_s=round(np_label, 3), table_wall_s=round(np_table, 3), clean_round_wall_s=round(np_clean, 3),
                  scipy_label_per_class_wall_s=None if scipy_s is None else round(scipy_s, 3))
        if k_c > 300000:   # a speckled map: the per-ring Python loop takes minutes; not a case a user traces
            rows.emit(way="trace", **common, wall_s=None, note="not measured: more than 300 000 regions")
            continue
        host = labels_c.cpu().numpy()
        t0 = time.perf_counter()
        polys = regions.trace_polygons(host, range(1, k_c + 1), D, 1)
        trace_s = time.perf_counter() - t0
        rows.emit(way="trace", **common, wall_s=round(trace_s, 3), rings=sum(1 + len(h) for _, h in polys.values()),
                  vertices=int(sum(len(o_) + sum(len(x) for x in h) for o_, h in polys.values())))
    rows.write(args.out)


if __name__ == "__main__":
    main()
