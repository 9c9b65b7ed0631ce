"""Cost of dh_embed_knn beside `torch.cdist(q, b).topk(k, largest=False)` on the same tensors.

Three sizes, uniform random rows: the slide's 198 916 tiles against a bank of 8 192 labelled tiles at D = 2048 (k = 8), against
a bank of 1 024 at D = 512 (k = 8), and the self-search of the slide after `PCA.reduce` to 64 columns (k = 16).  Median of
`--reps` event-timed calls after 3 warm-ups; element pairs per second (one pair = a subtract and a fused multiply-add).  The torch
side goes through the query rows in chunks of `--torch_chunk` rows where its n x m distance matrix would not fit, timed as one
call; `index_agreement` is the share of the kernel's indices that torch returns too (torch's distances come from the
|q|^2 + |b|^2 - 2 q.b form and its ties are broken differently, so the share is below 1 by design).

    python tools/knn_time.py [--reps 5] [--sizes big mid self] --out profiles/knn_time.json
"""
from __future__ import annotations

import argparse

SIZES = {"big": (198916, 8192, 2048, 8), "mid": (198916, 1024, 512, 8), "self": (198916, 198916, 64, 16)}


def main():
    import torch
    from _timing import Rows, median_ms

    from deephisto_amd.neighbours import nearest_rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", choices=list(SIZES), default=list(SIZES))
    ap.add_argument("--torch_chunk", type=int, default=16384, help="query rows per torch.cdist call when n * m floats exceed 2^33")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    rows = Rows()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.sizes:
        n, m, D, k = SIZES[name]
        q = torch.rand((n, D), generator=g, device=dev, dtype=torch.float32)
        b = q if name == "self" else torch.rand((m, D), generator=g, device=dev, dtype=torch.float32)
        index = torch.empty((n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((n, k), dtype=torch.float32, device=dev)
        ms, best = median_ms(lambda: nearest_rows(q, b, k, index, dist), args.reps)
        chunk = n if n * m <= 2 ** 33 else args.torch_chunk
        t_index = torch.empty((n, k), dtype=torch.int64, device=dev)

        def torch_side():
            for lo in range(0, n, chunk):
                t_index[lo:lo + chunk] = torch.cdist(q[lo:lo + chunk], b).topk(k, dim=1, largest=False).indices

        tms, tbest = median_ms(torch_side, min(args.reps, 3))
        ours = index.to(torch.int64)
        agree = float((ours[:, :, None] == t_index[:, None, :]).any(dim=2).float().mean())
        rows.emit(what="knn", size=name, n=n, m=m, D=D, k=k, ms=round(ms, 3), min_ms=round(best, 3), torch_ms=round(tms, 3),
                  torch_min_ms=round(tbest, 3), torch_chunk_rows=chunk, over_torch=round(ms / tms, 3),
                  tpairs_per_s=round(n * m * D / (ms / 1e3) / 1e12, 2), index_agreement=round(agree, 5))
        del q, b, index, dist, t_index, ours
        torch.cuda.empty_cache()
    rows.write(args.out, "a" if args.append else "w")


if __name__ == "__main__":
    main()
