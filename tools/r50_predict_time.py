"""Time whole-slide prediction with a ResNet-50 (dh_resnet50 inference engine) against the callback route it replaces.

Closed-form slide in HBM (default 12 000^2); predict_full_patched with a ResNet-50 (bf16, BN folded) at the reference's geometry
(patch 224, stride 112) and at 256 / 256, device-resident, one warm-up run then `--reps` timed runs.  The old route --
ImagePredictorPatched + batch_predictor, which for a ResNet-50 builds a float32 NCHW copy of every 64-tile batch and runs the
training engine's eval forward -- is timed on a `--cb_side`^2 slice of the same slide at 224 / 112.  Per run: tiles, seconds,
patches/s and the whole-model fraction of the 2.5 PF dense bf16 MFMA peak (algorithmic FLOPs = 2 x MACs of every convolution and
the fc, counted from the topology).  One JSON line per measurement.

    python tools/r50_predict_time.py [--side 12000] [--cb_side 2048] [--reps 3] [--skip_callback] [--out profiles/r50_predict_time.json]
"""
from __future__ import annotations

import argparse
import time

PEAK_BF16 = 2.5e15


def resnet50_macs(P: int, n_cls: int = 5) -> int:
    h = P // 2
    macs = 7 * 7 * 3 * 64 * h * h
    h //= 2
    cin = 64
    for width, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            ho = h // s
            macs += cin * width * h * h + 9 * width * width * ho * ho + width * 4 * width * ho * ho
            if b == 0:
                macs += cin * 4 * width * ho * ho
            cin, h = 4 * width, ho
    return macs + 2048 * n_cls


def main():
    import numpy as np
    import torch
    from _timing import Rows, best_of, whole_slide_case

    from deephisto_amd.examples.predict_full_patched import ImagePredictorPatched, batch_predictor, predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=12000)
    ap.add_argument("--cb_side", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip_callback", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    slide, _smp, model = whole_slide_case(dev, args.side, arch="resnet50")
    torch.cuda.synchronize()
    rows = Rows()

    for P, S in ((224, 112), (256, 256)):
        smp = FullImageDenseSampler(slide, layer=1, patch_size=P, batch_size=64, stride=S, device=dev)
        best = best_of(lambda: predict_full_patched(smp, model, 5, downscale=16), args.reps)   # warm-up: handles, workspaces, kernels
        n = len(smp.origins)
        pps = n / best
        rows.emit(route="predict_full_patched", arch="resnet50", side=args.side, patch=P, stride=S, tiles=n, seconds=round(best, 4),
                  patches_per_s=round(pps, 1), gflop_per_tile=round(2 * resnet50_macs(P) / 1e9, 3),
                  fraction_of_bf16_peak=round(pps * 2 * resnet50_macs(P) / PEAK_BF16, 4))
    if not args.skip_callback:
        P, S, s = 224, 112, args.cb_side
        sub = slide[:s, :s].contiguous()
        smp = FullImageDenseSampler(sub, layer=1, patch_size=P, batch_size=64, stride=S, device=dev)

        def run():
            return ImagePredictorPatched((s, s), smp.generator(), lambda p: batch_predictor(p, model, dev), 5, layer=1,
                                         downscale=16).process()

        run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = len(smp.origins)
        rows.emit(route="ImagePredictorPatched+batch_predictor (training-engine eval)", arch="resnet50", side=s, patch=P, stride=S, tiles=n,
                  seconds=round(dt, 4), patches_per_s=round(n / dt, 1), fraction_of_bf16_peak=round(n / dt * 2 * resnet50_macs(P) / PEAK_BF16, 4))
        smp2 = FullImageDenseSampler(sub, layer=1, patch_size=P, batch_size=64, stride=S, device=dev)
        fast = predict_full_patched(smp2, model, 5, downscale=16).cpu().numpy()
        rows.emit(route="agreement on the slice", class_map_agreement=float((fast == np.asarray(pred)).mean()))
    rows.write(args.out)


if __name__ == "__main__":
    main()
