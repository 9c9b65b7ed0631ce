"""Cost of the rotated and rescaled gather against the plain flipped gather and the stain-jitter gather
at the training shape.

One resident slide (a 2 048^2 synthetic H&E tile, tests/helpers/stain_ref.py, repeated to `--side`^2), one batch of `--batch`
seeded origins (some hang over the border, as the region samplers allow), patch 224, NCHW, both flips on, angles uniform in
+-180 degrees, s uniform in [0.8, 1.25].  Per dtype four gathers alternate in one process: `gather_tiles_aug` and
`gather_tiles_stain_aug` (whose kernels the rotated gather leaves as they were) and `gather_tiles_affine_aug` without and with the
stain rows; each is timed with HIP events around `--calls` back-to-back calls (a single call is tens of microseconds), median of
`--reps` such windows after 3 warm-up windows, in two alternating rounds.  The rotated batches are compared with the NumPy
restatement on their first tiles before anything is timed.  `of_step`: a gather's time over one bf16 ResNet-18 training step at
`--steps-per-s`.

    python tools/geom_aug_time.py [--side 8192] [--batch 64] [--reps 20] [--calls 50] --out profiles/geom_aug_time.json
"""
from __future__ import annotations

import argparse
import sys


def main():
    import numpy as np
    import torch
    from _timing import REPO, Rows, median_ms
    sys.path.insert(0, str(REPO / "tests" / "helpers"))
    import geom_aug_ref as G
    import stain_ref as R

    from deephisto_amd import geom_aug as GA
    from deephisto_amd import stain as S
    from deephisto_amd import tiles
    from deephisto_amd._lib import DH_LAYOUT_NCHW

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps-per-s", type=float, nargs=2, default=(384.0, 412.0))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda:0")
    P, B, side, rows = args.patch, args.batch, args.side, Rows()
    tile_host = R.synth_he(2048, 2048, 1, glass=0.05)
    n = -(-side // 2048)
    slide = torch.from_numpy(tile_host).to(dev).repeat(n, n, 1)[:side, :side].contiguous()
    rng = np.random.default_rng(0)
    yx = rng.integers(-P // 4, side - 3 * P // 4, (B, 2)).astype(np.int32)
    fit = S.StainNormalizer().fit(slide)
    params = S.jitter_params(fit.HE, *S.StainAugmenter(0.2, 0.05, seed=0).draw(B))
    affine = GA.GeometricAugmenter(180.0, (0.8, 1.25), seed=0).rows(B)
    o_dev, p_dev, a_dev = torch.from_numpy(yx).to(dev), torch.from_numpy(params).to(dev), torch.from_numpy(affine).to(dev)

    host = np.tile(tile_host, (n, n, 1))[:side, :side]
    for p_d, p_h in ((None, None), (p_dev[:4], params[:4])):
        got = tiles.gather_tiles_affine_aug(slide, o_dev[:4], P, DH_LAYOUT_NCHW, torch.float32, a_dev[:4], True, True, params_dev=p_d)
        want = G.gather(host, yx[:4], P, affine[:4], True, True, nchw=True, params=p_h)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "the rotated gather differs from the restatement"
    del host

    for name, dtype, esz in (("bf16", torch.bfloat16, 2), ("f32", torch.float32, 4)):
        def repeat(fn):
            def window():
                for _ in range(args.calls):
                    fn()
            return window

        fns = {"plain": repeat(lambda: tiles.gather_tiles_aug(slide, o_dev, P, DH_LAYOUT_NCHW, dtype, True, True)),
               "jitter": repeat(lambda: tiles.gather_tiles_stain_aug(slide, o_dev, P, DH_LAYOUT_NCHW, dtype, p_dev, True, True)),
               "affine": repeat(lambda: tiles.gather_tiles_affine_aug(slide, o_dev, P, DH_LAYOUT_NCHW, dtype, a_dev, True, True)),
               "affine_jitter": repeat(lambda: tiles.gather_tiles_affine_aug(slide, o_dev, P, DH_LAYOUT_NCHW, dtype, a_dev, True, True,
                                                                             params_dev=p_dev))}
        t = {k: [] for k in fns}
        for _ in range(2):   # two alternating rounds: the spread between them is the noise to read a difference against
            for k, fn in fns.items():
                med, best = median_ms(fn, args.reps)
                t[k].append((med / args.calls, best / args.calls))
        out_bytes, px = B * P * P * 3 * esz, B * P * P
        row = dict(dtype=name, batch=B, patch=P, layout="nchw", side=side, reps=args.reps, calls_per_window=args.calls,
                   out_mbytes=round(out_bytes / 1e6, 3), plain_read_mbytes=round(px * 3 / 1e6, 3), affine_read_mbytes=round(px * 12 / 1e6, 3))
        for k in t:
            med = min(m for m, _ in t[k])
            row.update({f"{k}_us": round(med * 1e3, 2), f"{k}_us_rounds": [round(m * 1e3, 2) for m, _ in t[k]],
                        f"{k}_min_us": round(min(b for _, b in t[k]) * 1e3, 2)})
        row["affine_over_plain"] = round(row["affine_us"] / row["plain_us"], 3)
        row["affine_jitter_over_jitter"] = round(row["affine_jitter_us"] / row["jitter_us"], 3)
        row["affine_jitter_over_plain"] = round(row["affine_jitter_us"] / row["plain_us"], 3)
        row["jitter_over_plain"] = round(row["jitter_us"] / row["plain_us"], 3)
        row["bytes_over_plain"] = round((px * 12 + out_bytes) / (px * 3 + out_bytes), 3)   # what the four-tap read alone explains
        for k in ("plain", "affine", "affine_jitter"):
            row[f"{k}_of_step"] = [round(row[f"{k}_us"] * 1e-6 * s, 4) for s in args.steps_per_s]
        rows.emit(**row)
    rows.write(args.out)


if __name__ == "__main__":
    main()
