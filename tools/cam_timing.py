"""Cost of the fine maps on the 50 000^2 synthetic slide at 224 / 112 / d = 16.

  --mode slide       whole-slide `predict_fine_patched` beside `predict_full_patched` (the parent's code path, untouched) for bf16
                     ResNet-18 and ResNet-50: one warm-up each, then `--reps` rounds that alternate the two (wall time around a
                     device synchronise; min and all values).  One process: no exchange runs; `exchange_bytes` is what the one
                     all-gather of the rows would move.
  --mode head        one full launch of `cam_tiles` (with logits) and of `forward_tiles` per engine, `--reps` times each, for a
                     kernel trace (`rocprofv3 --kernel-trace --stats -- python tools/cam_timing.py --mode head`): the trace gives
                     cam_head_kernel's time; the row printed here gives the bytes one launch must read and write, and the time that
                     takes at the 6.3 TB/s copy rate the other sections use.  Event times of the two entries are printed too, but
                     their difference is far below their spread: the trace is the measurement.
  --mode accumulate  `accumulate_cam` on the slide's tile list beside (1) `accumulate_logits` on the same tiles (one row per tile: the
                     parent's map) and (2) `accumulate_logits` over `expand_positions` with patch 32, the route it replaces: median
                     of `--reps` event-timed calls after 3 warm-ups, each route in a loop of its own (the bin plan is cached per
                     origin list, so alternating routes would time the host's plan builds), and the wall time of each route's
                     first call, which includes building and uploading its bin plan.

    python tools/cam_timing.py --mode slide [--side 50000] [--reps 3] --out profiles/cam_time.json
    python tools/cam_timing.py --mode accumulate [--reps 10] --out profiles/cam_time.json --append
"""
from __future__ import annotations

import argparse
import time

P, S, DOWN = 224, 112, 16
COPY_RATE = 6.3e12   # bytes per second: the HBM copy rate DESIGN.md measures kernels against


def slide_mode(args, rows):
    import torch
    from _timing import whole_slide_case
    from embeddings_timing import alternate

    from deephisto_amd.cam import predict_fine_patched
    from deephisto_amd.predict import predict_full_patched

    dev = torch.device("cuda:0")
    for arch in ("resnet18", "resnet50"):
        slide, smp, model = whole_slide_case(dev, args.side, arch, "bf16", P, S)
        t = alternate({
            "predict": lambda: predict_full_patched(smp, model, 5, downscale=DOWN),
            "fine": lambda: predict_fine_patched(smp, model, 5, downscale=DOWN),
            "fine_proba": lambda: predict_fine_patched(smp, model, 5, downscale=DOWN, return_proba=True),
        }, args.reps)
        best = {k: min(v) for k, v in t.items()}
        row_bytes = 4 * (P // 32) ** 2 * 5
        rows.emit(mode="slide", arch=arch, dtype="bf16", side=args.side, patch=P, stride=S, downscale=DOWN, n_tiles=smp.n_tiles,
                  row_bytes=row_bytes, exchange_bytes=row_bytes * smp.n_tiles, predict_s=round(best["predict"], 4),
                  fine_s=round(best["fine"], 4), fine_proba_s=round(best["fine_proba"], 4),
                  fine_over_predict=round(best["fine"] / best["predict"], 4),
                  all_s={k: [round(x, 4) for x in v] for k, v in t.items()})
        del slide, smp, model
        torch.cuda.empty_cache()


def head_mode(args, rows):
    import torch
    from _timing import median_ms, whole_slide_case

    dev = torch.device("cuda:0")
    for arch in ("resnet18", "resnet50"):
        slide, smp, model = whole_slide_case(dev, 8000, arch, "bf16", P, S)
        n = min(model.default_micro_batch(), smp.n_tiles)
        o = torch.from_numpy(smp.origins[:n]).to(dev)
        C, HW = model.feature_width, (P // 32) ** 2
        fwd_ms, _ = median_ms(lambda: model.forward_tiles(slide, o, P), args.reps)
        cam_ms, _ = median_ms(lambda: model.cam_tiles(slide, o, P, return_logits=True), args.reps)
        need = n * HW * (2 * C + 4 * 5) + 4 * 5 * (C + 1)      # the bf16 activation once, the rows once, fc once
        rows.emit(mode="head", arch=arch, n=n, C=C, HW=HW, n_cls=5, bytes_needed=need, us_at_copy_rate=round(need / COPY_RATE * 1e6, 2),
                  forward_tiles_ms=round(fwd_ms, 4), cam_tiles_ms=round(cam_ms, 4))
        del slide, smp, model
        torch.cuda.empty_cache()


def accumulate_mode(args, rows):
    import torch
    from _timing import median_ms

    from deephisto_amd import tiles

    dev = torch.device("cuda:0")
    side, n_cls, s = args.side, 5, P // 32
    o, n = tiles.tile_grid(side, side, P, S, 1)
    o = o[:n]
    g = torch.Generator(device=dev).manual_seed(0)
    cam = torch.randn((n, s, s, n_cls), generator=g, device=dev, dtype=torch.float32)
    logits = cam.mean(dim=(1, 2)).contiguous()
    expanded = tiles.expand_positions(o, P)
    flat = cam.view(-1, n_cls)

    def first(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    routes = {"accumulate_logits_tiles": lambda: tiles.accumulate_logits(logits, o, P, DOWN, side, side),
              "accumulate_cam": lambda: tiles.accumulate_cam(cam, o, P, DOWN, side, side),
              "accumulate_logits_expanded": lambda: tiles.accumulate_logits(flat, expanded, 32, DOWN, side, side)}
    out = {}
    for name, fn in routes.items():
        first_s = first(fn)
        med, best = median_ms(fn, args.reps)
        out[name] = dict(first_call_s=round(first_s, 4), median_ms=round(med, 4), min_ms=round(best, 4))
    same = torch.equal(routes["accumulate_cam"]()[0], routes["accumulate_logits_expanded"]()[0])
    rows.emit(mode="accumulate", side=side, patch=P, stride=S, downscale=DOWN, n_cls=n_cls, n_tiles=int(n), n_expanded=int(len(expanded)),
              canvas_bytes=4 * n_cls * (side // DOWN) ** 2, rows_bytes=4 * n_cls * s * s * int(n), bit_identical=bool(same), **out,
              cam_over_tiles=round(out["accumulate_cam"]["median_ms"] / out["accumulate_logits_tiles"]["median_ms"], 3),
              cam_over_expanded=round(out["accumulate_cam"]["median_ms"] / out["accumulate_logits_expanded"]["median_ms"], 3))


def main():
    from _timing import Rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["slide", "head", "accumulate"], default="slide")
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    rows = Rows()
    {"slide": slide_mode, "head": head_mode, "accumulate": accumulate_mode}[args.mode](args, rows)
    rows.write(args.out, "a" if args.append else "w")


if __name__ == "__main__":
    main()
