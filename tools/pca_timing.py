"""Cost of the PCA layer: dh_embed_scatter, dh_embed_project and a whole fit.

  --mode kernels  at n = 38 416 and 198 916, D = 512 and 2048: median of `--reps` event-timed calls after 3 warm-ups, beside a
                  `dst.copy_(src)` of the feature matrix in the same run.  The scatter beside the float32 expression
                  `(x - m).T @ (x - m)` (hipBLAS; `over_torch` is the multiple the fixed order costs) with its rate in FMAs of one
                  triangle per second; the projection at K = 3 and 64 beside `(x - m) @ comp.T` and, at K = 64, beside
                  dh_embed_scores on the same rows.
  --mode slide    on the embeddings of the 50 000^2 synthetic slide at 224 / 112 (bf16 ResNet-18: D = 512; ResNet-50: D = 2048): a
                  whole `PCA(64).fit` (wall time around a device synchronise, the least of `--reps`) with its scatter and
                  eigen-solve parts, `transform` and `colour_map`, beside `predict_full_patched` on the same slide.

    python tools/pca_timing.py --mode kernels [--reps 20] --out profiles/pca_time.json
    python tools/pca_timing.py --mode slide [--side 50000] [--archs resnet18 resnet50] --out profiles/pca_time.json --append
"""
from __future__ import annotations

import argparse

P, S, DOWN = 224, 112, 16


def kernels_mode(args, rows):
    import torch
    from _timing import median_ms

    from deephisto_amd.embeddings import prototype_scores
    from deephisto_amd.pca import centred_scatter, project

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for n in args.ns:
        for D in args.ds:
            x = torch.rand((n, D), generator=g, device=dev, dtype=torch.float32) + 1.0      # a common mean, small detail
            y = torch.empty_like(x)
            copy_ms, _ = median_ms(lambda: y.copy_(x), args.reps)
            rows.emit(mode="kernels", what="copy", n=n, D=D, ms=round(copy_ms, 4), copy_rate_gb_s=round(8.0 * n * D / (copy_ms / 1e3) / 1e9, 1))
            del y
            m = x.mean(0).contiguous()
            ms, best = median_ms(lambda: centred_scatter(x, m), args.reps)

            def blas():
                t = x - m
                return t.T @ t

            tms, _ = median_ms(blas, args.reps)
            rows.emit(mode="kernels", what="scatter", n=n, D=D, ms=round(ms, 4), min_ms=round(best, 4), torch_ms=round(tms, 4),
                      over_torch=round(ms / tms, 3), triangle_tfma_per_s=round(n * D * (D + 64) / 2 / (ms / 1e3) / 1e12, 2),
                      over_copy=round(ms / copy_ms, 2))
            for K in (3, 64):
                c = torch.rand((K, D), generator=g, device=dev, dtype=torch.float32) - 0.5
                out = torch.zeros((n, 64), dtype=torch.float32, device=dev)
                ms, best = median_ms(lambda: project(x, m, c, out=out), args.reps)
                tms, _ = median_ms(lambda: (x - m) @ c.T, args.reps)
                row = dict(mode="kernels", what="project", n=n, D=D, K=K, ms=round(ms, 4), min_ms=round(best, 4), torch_ms=round(tms, 4),
                           over_torch=round(ms / tms, 3), over_copy=round(ms / copy_ms, 2))
                if K == 64:
                    sms, _ = median_ms(lambda: prototype_scores(x, c), args.reps)
                    row.update(scores_ms=round(sms, 4), over_scores=round(ms / sms, 3), tfma_per_s=round(n * D * K / (ms / 1e3) / 1e12, 2))
                rows.emit(**row)
            del x
            torch.cuda.empty_cache()


def slide_mode(args, rows):
    import torch
    from _timing import best_of, whole_slide_case

    from deephisto_amd.embeddings import extract_embeddings
    from deephisto_amd.pca import PCA
    from deephisto_amd.predict import predict_full_patched

    dev = torch.device("cuda:0")
    for arch in args.archs:
        slide, smp, model = whole_slide_case(dev, args.side, arch, "bf16", P, S)
        predict_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=DOWN), args.reps)
        emb = extract_embeddings(smp, model)
        del slide, smp, model
        torch.cuda.empty_cache()
        pca = PCA(64).fit(emb)
        fit_s = best_of(lambda: PCA(64).fit(emb), args.reps)
        timings = PCA(64).fit(emb).timings_
        rows.emit(mode="slide", arch=arch, side=args.side, patch=P, stride=S, n=len(emb), D=emb.width, K=64, predict_s=round(predict_s, 4),
                  fit_s=round(fit_s, 4), scatter_part_ms=round(timings["scatter_ms"], 2), eigen_ms=round(timings["eigen_ms"], 2),
                  transform_s=round(best_of(lambda: pca.transform(emb, width=64), args.reps), 5),
                  colour_map_s=round(best_of(lambda: pca.colour_map(emb, DOWN), args.reps), 4),
                  explained_first3=[round(float(v), 4) for v in pca.explained_variance_ratio_[:3]])
        del emb
        torch.cuda.empty_cache()


def main():
    from _timing import Rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "slide"], default="kernels")
    ap.add_argument("--ns", type=int, nargs="+", default=[38416, 198916])
    ap.add_argument("--ds", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--archs", nargs="+", default=["resnet18", "resnet50"])
    ap.add_argument("--reps", type=int, default=None, help="default 20 (kernels) or 3 (slide)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    args.reps = args.reps or (20 if args.mode == "kernels" else 3)
    rows = Rows()
    (kernels_mode if args.mode == "kernels" else slide_mode)(args, rows)
    rows.write(args.out, "a" if args.append else "w")


if __name__ == "__main__":
    main()
