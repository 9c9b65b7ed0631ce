"""Cost of the clustering layer: dh_embed_assign, one Lloyd iteration, the seeding and a whole fit.

  --mode kernels  dh_embed_assign at n = 38 416 and 198 916, D = 512 and 2048, K = 1, 5 and 64 beside `torch.cdist(x, c).argmin(1)`
                  on the same card: median of `--reps` event-timed calls after 3 warm-ups; the bytes the algorithm needs (the
                  matrix once, the centres, 8 bytes per row out) over that time as a fraction of the copy rate measured in the same
                  run (`dst.copy_(src)` of the feature matrix: bytes read + written over its time); element pairs per second (one
                  pair = a subtract and a fused multiply-add).  `tile64_ms` is the 32 x 64 tile launched for the same rows (K = 17
                  with the centres padded by copies of centre 0: that tile's work does not depend on K), what K <= 16 would cost
                  without the one-row-per-lane instantiation.
  --mode slide    on the embeddings of the 50 000^2 synthetic slide at 224 / 112 (bf16 ResNet-18: D = 512; ResNet-50: D = 2048):
                  one Lloyd iteration (class sums + centres + assignment), the K seeding calls and a whole `KMeans.fit`, for
                  K = 5 and 64, beside `predict_full_patched` on the same slide (wall time around a device synchronise, the least
                  of `--reps`).

    python tools/cluster_timing.py --mode kernels [--reps 20] --out profiles/cluster_time.json
    python tools/cluster_timing.py --mode slide [--side 50000] [--archs resnet18 resnet50] --out profiles/cluster_time.json --append
"""
from __future__ import annotations

import argparse

P, S, DOWN = 224, 112, 16


def kernels_mode(args, rows):
    import torch
    from _timing import median_ms

    from deephisto_amd.clustering import nearest_centres

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for n in (38416, 198916):
        for D in (512, 2048):
            x = torch.rand((n, D), generator=g, device=dev, dtype=torch.float32)
            y = torch.empty_like(x)
            copy_ms, _ = median_ms(lambda: y.copy_(x), args.reps)
            copy_rate = 8.0 * n * D / (copy_ms / 1e3)      # bytes read + written per second
            rows.emit(mode="kernels", what="copy", n=n, D=D, ms=round(copy_ms, 4), copy_rate_gb_s=round(copy_rate / 1e9, 1))
            del y
            lab = torch.empty(n, dtype=torch.int32, device=dev)
            dst = torch.empty(n, dtype=torch.float32, device=dev)
            for K in (1, 5, 64):
                c = torch.rand((K, D), generator=g, device=dev, dtype=torch.float32)
                ms, best = median_ms(lambda: nearest_centres(x, c, lab, dst), args.reps)
                tms, _ = median_ms(lambda: torch.cdist(x, c).argmin(1), args.reps)
                need = 4.0 * (n * D + K * D) + 8.0 * n
                row = dict(mode="kernels", what="assign", n=n, D=D, K=K, ms=round(ms, 4), min_ms=round(best, 4), torch_cdist_ms=round(tms, 4),
                           over_torch=round(ms / tms, 3), gpairs_per_s=round(n * D * K / (ms / 1e3) / 1e9, 1),
                           fraction_of_copy_rate=round(need / (ms / 1e3) / copy_rate, 3))
                if K <= 16:
                    wide = torch.cat([c, c[:1].expand(17 - K, D)]).contiguous()
                    l2, d2 = nearest_centres(x, wide)
                    nearest_centres(x, c, lab, dst)
                    assert torch.equal(l2, lab) and torch.equal(d2, dst), "the two instantiations agree bit for bit"
                    wms, _ = median_ms(lambda: nearest_centres(x, wide, lab, dst), args.reps)
                    row.update(tile64_ms=round(wms, 4), over_tile64=round(ms / wms, 3))
                rows.emit(**row)
            del x
            torch.cuda.empty_cache()


def slide_mode(args, rows):
    import torch
    from _timing import best_of, whole_slide_case

    from deephisto_amd.clustering import KMeans, nearest_centres
    from deephisto_amd.embeddings import class_sums, extract_embeddings, normalize_rows
    from deephisto_amd.predict import predict_full_patched

    dev = torch.device("cuda:0")
    for arch in args.archs:
        slide, smp, model = whole_slide_case(dev, args.side, arch, "bf16", P, S)
        predict_s = best_of(lambda: predict_full_patched(smp, model, 5, downscale=DOWN), args.reps)
        emb = extract_embeddings(smp, model)
        del slide, smp, model
        torch.cuda.empty_cache()
        x = normalize_rows(emb.features)
        n, D = int(x.shape[0]), int(x.shape[1])
        for K in (5, 64):
            km = KMeans(K, seed=0).fit(emb)
            centres, lab = km.centres_, km.labels_
            out_l, out_d = torch.empty_like(lab), torch.empty(n, dtype=torch.float32, device=dev)

            def iteration():
                sums, counts = class_sums(x, lab, K)
                counts.cpu()
                nearest_centres(x, sums / counts.clamp(min=1).to(torch.float32)[:, None], out_l, out_d)
                return int((out_l != lab).sum())

            def seeding():
                for j in range(K):
                    nearest_centres(x, centres[j:j + 1], out_l, out_d, k0=j, merge=j > 0)
                    out_d.cpu()

            rows.emit(mode="slide", arch=arch, side=args.side, patch=P, stride=S, n=n, D=D, K=K, predict_s=round(predict_s, 4),
                      iteration_s=round(best_of(iteration, args.reps), 5), seeding_s=round(best_of(seeding, args.reps), 5),
                      fit_s=round(best_of(lambda: KMeans(K, seed=0).fit(emb), args.reps), 4), fit_iterations=km.n_iter_,
                      converged=km.converged_, inertia=km.inertia_, sizes=km.counts_.tolist())
        del emb, x
        torch.cuda.empty_cache()


def main():
    from _timing import Rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "slide"], default="kernels")
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
