"""Cost of the tile embeddings on the 50 000^2 synthetic slide at 224 / 112, and of the three embed kernels.

  --mode slide    whole-slide `extract_embeddings` against `predict_full_patched` (the parent's code path, untouched) for bf16
                  ResNet-18 and ResNet-50, plain and with TissueFilter("otsu") on the slide with its right half set to glass: one
                  warm-up each, then `--reps` rounds that alternate the two (wall time around a device synchronise; min and all
                  values).  The difference is the cost of storing the pooled vectors (and, with `return_logits`, nothing else: the
                  logits are written either way).  One process: no exchange runs; `exchange_bytes` is what one all-gather of the
                  rows would move.
  --mode kernels  dh_embed_normalize / dh_embed_scores / dh_embed_class_sums at n = 38 416 and 198 916, D = 512 and 2048, K = 5 and
                  64, beside the torch expressions on the same card (`F.normalize`, `scale * (x @ p.T)`, `index_add_`): median of
                  `--reps` event-timed calls after 3 warm-ups; bytes the algorithm needs over that time as a fraction of the copy
                  rate measured in the same run (`dst.copy_(src)` of the feature matrix: bytes read + written over its time).

    python tools/embeddings_timing.py --mode slide [--side 50000] [--reps 3] --out profiles/embeddings_time.json
    python tools/embeddings_timing.py --mode kernels [--reps 20] --out profiles/embeddings_time.json --append
"""
from __future__ import annotations

import argparse
import time

P, S, DOWN = 224, 112, 16


def alternate(fns, reps):
    """{name: [seconds]}: one warm-up of every fn, then `reps` rounds running them in turn, each synchronised."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append(time.perf_counter() - t0)
    return out


def slide_mode(args, rows):
    import torch
    from _timing import whole_slide_case

    from deephisto_amd.embeddings import extract_embeddings
    from deephisto_amd.predict import predict_full_patched
    from deephisto_amd.tissue import TissueFilter

    dev = torch.device("cuda:0")
    for arch in ("resnet18", "resnet50"):
        slide, smp, model = whole_slide_case(dev, args.side, arch, "bf16", P, S)
        D = model.feature_width
        for filt in (None, TissueFilter("otsu")):
            if filt is not None:
                slide[:, args.side // 2:] = 255      # half glass
                torch.cuda.synchronize()
            info: dict = {}
            t = alternate({
                "predict": lambda: predict_full_patched(smp, model, 5, downscale=DOWN, tissue=filt),
                "extract": lambda: extract_embeddings(smp, model, tissue=filt, tissue_info=info),
                "extract_logits_map": lambda: extract_embeddings(smp, model, tissue=filt, return_logits=True).class_map(
                    DOWN, fill_class=-1),
            }, args.reps)
            n_kept = info.get("n_kept", smp.n_tiles)
            best = {k: min(v) for k, v in t.items()}
            rows.emit(mode="slide", arch=arch, dtype="bf16", side=args.side, patch=P, stride=S, tissue="otsu" if filt else "off",
                      n_tiles=smp.n_tiles, n_kept=n_kept, feature_width=D, feature_bytes=4 * D * n_kept, exchange_bytes=4 * D * n_kept,
                      predict_s=round(best["predict"], 4), extract_s=round(best["extract"], 4),
                      extract_logits_map_s=round(best["extract_logits_map"], 4),
                      extract_over_predict=round(best["extract"] / best["predict"], 4),
                      extract_logits_map_over_predict=round(best["extract_logits_map"] / best["predict"], 4),
                      all_s={k: [round(x, 4) for x in v] for k, v in t.items()})
        del slide, smp, model
        torch.cuda.empty_cache()


def kernels_mode(args, rows):
    import torch
    import torch.nn.functional as F
    from _timing import median_ms

    from deephisto_amd.embeddings import class_sums, normalize_rows, prototype_scores

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for n in (38416, 198916):
        for D in (512, 2048):
            x = torch.rand((n, D), generator=g, device=dev, dtype=torch.float32)
            y = torch.empty_like(x)
            copy_ms, _ = median_ms(lambda: y.copy_(x), args.reps)
            copy_rate = 8.0 * n * D / (copy_ms / 1e3)      # bytes read + written per second
            rows.emit(mode="kernels", what="copy", n=n, D=D, ms=round(copy_ms, 4), copy_rate_gb_s=round(copy_rate / 1e9, 1))
            ms, _ = median_ms(lambda: normalize_rows(x, out=y), args.reps)
            tms, _ = median_ms(lambda: F.normalize(x, dim=1, out=y), args.reps)
            # the kernel reads every row twice (the second pass out of cache where a row fits) and writes it once: 8 bytes per element needed
            rows.emit(mode="kernels", what="normalize", n=n, D=D, ms=round(ms, 4), torch_ms=round(tms, 4), over_torch=round(ms / tms, 3),
                      fraction_of_copy_rate=round(8.0 * n * D / (ms / 1e3) / copy_rate, 3))
            for K in (5, 64):
                p = torch.rand((K, D), generator=g, device=dev, dtype=torch.float32)
                ms, _ = median_ms(lambda: prototype_scores(x, p, 0.5), args.reps)
                tms, _ = median_ms(lambda: 0.5 * (x @ p.T), args.reps)
                need = 4.0 * (n * D + K * D + n * K)
                rows.emit(mode="kernels", what="scores", n=n, D=D, K=K, ms=round(ms, 4), torch_ms=round(tms, 4), over_torch=round(ms / tms, 3),
                          gfma_per_s=round(n * D * K / (ms / 1e3) / 1e9, 1), fraction_of_copy_rate=round(need / (ms / 1e3) / copy_rate, 3))
                lab = torch.randint(-1, K, (n,), generator=g, device=dev, dtype=torch.int32)      # about 1 / (K + 1) unlabelled
                dump = torch.where(lab < 0, K, lab).to(torch.int64)      # the torch expression sends unlabelled rows to an extra class
                ms, _ = median_ms(lambda: class_sums(x, lab, K), args.reps)

                def torch_sums():
                    out = torch.zeros((K + 1, D), dtype=torch.float32, device=dev)
                    return out.index_add_(0, dump, x)      # float atomics: neither ordered nor reproducible

                tms, _ = median_ms(torch_sums, args.reps)
                need = 4.0 * (float((lab >= 0).sum()) * D + n)
                rows.emit(mode="kernels", what="class_sums", n=n, D=D, K=K, ms=round(ms, 4), torch_ms=round(tms, 4),
                          over_torch=round(ms / tms, 3), fraction_of_copy_rate=round(need / (ms / 1e3) / copy_rate, 3))
            del x, y
            torch.cuda.empty_cache()


def main():
    from _timing import Rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["slide", "kernels"], default="slide")
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    rows = Rows()
    (slide_mode if args.mode == "slide" else kernels_mode)(args, rows)
    rows.write(args.out, "a" if args.append else "w")


if __name__ == "__main__":
    main()
