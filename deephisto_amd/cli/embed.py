"""What the predict CLI does with the tile embeddings of the pass: `--save_embeddings`, `--prototypes`, `--clusters*`, `--pca*`,
`--knn*`, `--similar_*`.

`--save_embeddings PATH` writes every classified tile's pooled feature vector, origin, grid index and logits as one `.npz`
(rank 0; `SlideEmbeddings.load`); the class map is finished from the logits of that same forward pass
and is the map of a run without the flag, bit for bit.  `--prototypes PATH` with `--anno` fits one prototype per class on this
slide's annotated tiles and writes them; without `--anno` it loads them and writes `{stem}_prototype_map.jpg`, the
nearest-prototype class of every cell over the slide.  Both take the dense branch and a resident slide and are refused with
`--random_sampler`, `--ondisk`, `--tta` and `--proba`.
`--clusters K [--cluster_seed S] [--cluster_init kmeans++|maximin] [--save_clusters PATH]` runs k-means over the embeddings of
the same pass (no annotation needed; the same refusals) and writes `{stem}_clusters.jpg`, the cluster of
most covering tiles per cell in a K-colour palette over the slide, and `{stem}_clusters.json` (K, sizes, inertia, iterations,
converged); `--load_clusters PATH` applies a saved codebook instead of fitting.  `--regions_json` / `--export_anno` then
describe the cluster map's regions, named `cluster_0` ...; the class map and its JPEGs are those of a run without the flags.
`--pca N [--save_pca PATH]` fits the first N principal components of the embeddings of the same pass (DESIGN.md section 4.19;
the same refusals) and writes `{stem}_pca.jpg`, the first three components of every cell's tiles as red, green and blue, and
`{stem}_pca.json` (N, tiles, explained variance and ratios, milliseconds of scatter, eigen-solve and projection);
`--load_pca PATH` applies a saved basis instead of fitting.
`--knn K --knn_bank PATH` classifies every tile by its K nearest tiles of a labelled bank (the same
refusals): with `--anno` the bank is this slide's annotated tiles (`--knn_per_class N` keeps at most N of a class), written
to PATH with the leave-one-out accuracy printed; without `--anno` PATH is loaded.  Either way `{stem}_knn.jpg` and
`{stem}_knn_overlay.jpg` show the class of most neighbours per cell, and `--regions_json` / `--export_anno` describe that map.
`--similar_to Y,X [--similar_k K] [--similar_json PATH]` writes the K tiles of this slide most like the tile under that pixel
(origins and squared distances of the normalised embeddings, nearest first, the tile itself left out) as JSON."""
from __future__ import annotations

import time
from pathlib import Path

import torch

from ..clustering import INITS as CLUSTER_INITS, KMeans, cluster_description, cluster_map
from ..embeddings import PrototypeClassifier, tile_labels
from ..models.patch_cls_simple.model import resolve_arch
from ..neighbours import KNNClassifier, cap_per_class, similar_tiles
from ..pca import PCA
from ..scoring import rasterize_annotation
from ..visualize import KNOWN_COLORS, _save_jpeg
from .common import Run, dense_resident_only, embedding_flags, existing_file, need, save_pictures, write_json


def add_flags(ap) -> None:
    ap.add_argument("--save_embeddings", default=None, metavar="PATH",
                    help="every classified tile's pooled feature vector (512 / 2048 floats), origins and logits as one .npz (rank 0); "
                         "the class map comes from the same forward pass (dense branch, resident slide)")
    ap.add_argument("--prototypes", default=None, metavar="PATH",
                    help="nearest-class-mean scoring of the tile embeddings: with --anno, fit the class prototypes on this slide's "
                         "annotated tiles and write them to PATH; without, load PATH and write {stem}_prototype_map.jpg")
    ap.add_argument("--clusters", type=int, default=None, metavar="K",
                    help="k-means over the tile embeddings of this pass (1 .. 64 clusters, no annotation needed): writes "
                         "{stem}_clusters.jpg and {stem}_clusters.json (rank 0); --regions_json / --export_anno then describe the "
                         "cluster map's regions, named cluster_0 ...")
    ap.add_argument("--cluster_seed", type=int, default=None, metavar="S", help="with --clusters: the seed of the k-means++ draws (default 0)")
    ap.add_argument("--cluster_init", choices=list(CLUSTER_INITS), default=None, help="with --clusters: the seeding (default kmeans++)")
    ap.add_argument("--save_clusters", default=None, metavar="PATH", help="with --clusters: the fitted codebook as one .npz (rank 0)")
    ap.add_argument("--load_clusters", default=None, metavar="PATH",
                    help="apply the codebook of an earlier --save_clusters to this slide instead of fitting (K comes from the file)")
    ap.add_argument("--pca", type=int, default=None, metavar="N",
                    help="principal components of the tile embeddings of this pass (1 .. 64, no annotation needed): writes "
                         "{stem}_pca.jpg, the first three components as red, green and blue, and {stem}_pca.json (rank 0)")
    ap.add_argument("--save_pca", default=None, metavar="PATH", help="with --pca: the fitted basis as one .npz (rank 0)")
    ap.add_argument("--load_pca", default=None, metavar="PATH",
                    help="apply the basis of an earlier --save_pca to this slide instead of fitting (N comes from the file)")
    ap.add_argument("--knn", type=int, default=None, metavar="K",
                    help="k-nearest-neighbour classification of the tile embeddings against a bank of labelled tiles (1 .. 63, "
                         "needs --knn_bank): writes {stem}_knn.jpg and {stem}_knn_overlay.jpg (rank 0); --regions_json / "
                         "--export_anno then describe that map's regions")
    ap.add_argument("--knn_bank", default=None, metavar="PATH",
                    help="with --knn: with --anno, fit the bank on this slide's annotated tiles, write it to PATH and print the "
                         "leave-one-out accuracy; without, load PATH")
    ap.add_argument("--knn_per_class", type=int, default=None, metavar="N",
                    help="with --knn and --anno: at most N tiles of a class enter the bank (every ceil(count / N)-th, in tile order)")
    ap.add_argument("--similar_to", default=None, metavar="Y,X",
                    help="retrieval: the tiles of this slide most like the tile under pixel Y,X, as JSON (rank 0)")
    ap.add_argument("--similar_k", type=int, default=None, metavar="K", help="with --similar_to: how many tiles (1 .. 63, default 16)")
    ap.add_argument("--similar_json", default=None, metavar="PATH",
                    help="with --similar_to: where the JSON goes (default {out_dir}/{stem}_similar.json)")


def check(ap, args, model=None) -> None:
    """Checks --save_embeddings / --prototypes / --clusters / --pca / --knn / --similar_to; a bad combination is an argparse error."""
    fit_flags = args.save_clusters or args.cluster_seed is not None or args.cluster_init is not None
    need(ap, args.knn is None or args.knn_bank, "--knn needs --knn_bank")
    need(ap, not args.knn_bank or args.knn is not None, "--knn_bank needs --knn")
    need(ap, args.knn_per_class is None or args.knn is not None, "--knn_per_class needs --knn")
    need(ap, args.similar_to is not None or not (args.similar_k is not None or args.similar_json),
         "--similar_k and --similar_json need --similar_to")
    for flag, on in embedding_flags(args):
        if not on:
            continue
        dense_resident_only(ap, args, flag)
        need(ap, args.tta == "off", f"{flag} stores one forward pass per tile; it cannot be combined with --tta")
        need(ap, not args.proba, f"{flag} finishes the class map from the stored logits; it cannot be combined with --proba")
    if args.prototypes and not args.anno:
        existing_file(ap, "--prototypes", args.prototypes, " (with --anno the prototypes are fitted and written there)")
    need(ap, args.clusters is None or 1 <= args.clusters <= 64, f"--clusters must be in 1 .. 64, not {args.clusters}")
    if args.load_clusters:
        need(ap, not fit_flags, "--load_clusters applies a saved codebook: --save_clusters, --cluster_seed and --cluster_init belong to a fit")
        existing_file(ap, "--load_clusters", args.load_clusters)
    else:
        need(ap, args.clusters is not None or not fit_flags, "--save_clusters, --cluster_seed and --cluster_init need --clusters")
    need(ap, not ((args.clusters is not None or args.load_clusters) and args.min_region is not None),
         "--min_region cleans the class map; with --clusters the region flags describe the cluster map as it is")
    need(ap, args.pca is None or 1 <= args.pca <= 64, f"--pca must be in 1 .. 64, not {args.pca}")
    if args.load_pca:
        need(ap, not args.save_pca and args.pca is None, "--load_pca applies a saved basis: --pca and --save_pca belong to a fit")
        existing_file(ap, "--load_pca", args.load_pca)
    else:
        need(ap, args.pca is not None or not args.save_pca, "--save_pca needs --pca")
    knn_from_args(ap, args)


def knn_from_args(ap, args) -> None:
    """Checks --knn / --knn_bank / --knn_per_class and --similar_to / --similar_k; leaves the pixel of --similar_to as a
    (y, x) tuple in `args.similar_yx` (None without the flag)."""
    n_cls = len(KNOWN_COLORS)
    if args.knn is not None:
        need(ap, 1 <= args.knn <= 63, f"--knn must be in 1 .. 63 (leave-one-out asks for one neighbour more), not {args.knn}")
        need(ap, args.knn_per_class is None or args.anno, "--knn_per_class caps a fit: it needs --anno")
        need(ap, args.knn_per_class is None or args.knn_per_class >= 1, f"--knn_per_class must be >= 1, not {args.knn_per_class}")
        need(ap, args.clusters is None and not args.load_clusters,
             "--knn and --clusters each hand their own map to the region flags; run them one at a time")
        need(ap, args.min_region is None, "--min_region cleans the class map; with --knn the region flags describe the k-NN map as it is")
        if not args.anno:
            existing_file(ap, "--knn_bank", args.knn_bank, " (with --anno the bank is fitted and written there)")
            try:
                bank = KNNClassifier.load(args.knn_bank)
            except (ValueError, KeyError, OSError) as e:
                ap.error(f"--knn_bank {args.knn_bank}: not a KNNClassifier file ({e!r})")
            arch = resolve_arch(None) if args.arch == "auto" and not args.weights else args.arch
            width = {"resnet18": 512, "resnet50": 2048}.get(arch)   # auto with a checkpoint: known once it is read (report_knn)
            need(ap, bank.n_classes == n_cls and (width is None or bank.bank.shape[1] == width),
                 f"--knn_bank {args.knn_bank}: {bank.n_classes} classes x {bank.bank.shape[1]} floats do not fit this model "
                 f"and description ({n_cls} x {width or 'the model width'})")
    args.similar_yx = None
    if args.similar_to is not None:
        try:
            y, x = (int(v) for v in args.similar_to.split(","))
        except ValueError:
            ap.error(f"--similar_to takes Y,X (a pixel of the slide), not {args.similar_to!r}")
        if args.synthetic is not None and not args.pyramid:
            need(ap, 0 <= y < args.synthetic[0] and 0 <= x < args.synthetic[1],
                 f"--similar_to {y},{x} lies outside the slide ({args.synthetic[0]} x {args.synthetic[1]})")
        need(ap, min(y, x) >= 0, f"--similar_to {y},{x} lies outside the slide")
        need(ap, args.similar_k is None or 1 <= args.similar_k <= 63, f"--similar_k must be in 1 .. 63, not {args.similar_k}")
        args.similar_yx = (y, x)


def _truth_labels(run: Run) -> torch.Tensor:
    """The label of every tile of the pass under --anno: the annotation's at the cell under the tile's centre."""
    args = run.args
    truth, _ = rasterize_annotation(args.anno_records, run.anno_dsc, args.layer, run.smp.h, run.smp.w, args.downscale_vis, device=run.device)
    return tile_labels(run.embeddings, truth, args.downscale_vis)


def report_prototypes(run: Run) -> None:
    """--prototypes: with --anno, fit the class prototypes on this slide's annotated tiles (the label of a tile is the annotation's
    at the cell under its centre) and save them; without, load them and write the prototype class map over the slide."""
    args, emb, n_cls = run.args, run.embeddings, len(run.anno_dsc.anno_classes)
    if args.anno_records is not None:
        pc = PrototypeClassifier(n_cls).fit(emb, _truth_labels(run))
        Path(args.prototypes).parent.mkdir(parents=True, exist_ok=True)
        pc.save(args.prototypes)
        print(f"prototypes: {int(pc.counts.sum())} labelled tiles, per class {pc.counts.tolist()}, empty {pc.empty_classes} "
              f"-> {args.prototypes}", flush=True)
        return
    pc = PrototypeClassifier.load(args.prototypes, device=run.device)
    if pc.n_classes != n_cls or pc.prototypes.shape[1] != emb.width:
        raise ValueError(f"--prototypes {args.prototypes}: {pc.n_classes} classes x {pc.prototypes.shape[1]} floats do not fit this "
                         f"model and description ({n_cls} x {emb.width})")
    save_pictures(run, run.anno_dsc, pc.predict_map(emb, args.downscale_vis), overlay="prototype_map")


def report_knn(run: Run):
    """--knn: with --anno, fit the bank on this slide's annotated tiles (the label of a tile is the annotation's at the cell under
    its centre, --knn_per_class caps a class), save it and print the leave-one-out accuracy; without, load it.  Either way write
    `{stem}_knn.jpg` and `{stem}_knn_overlay.jpg` from the k-NN class map, which is returned."""
    args, emb, n_cls = run.args, run.embeddings, len(run.anno_dsc.anno_classes)
    if args.anno_records is not None:
        labels = _truth_labels(run)
        if args.knn_per_class is not None:
            labels = cap_per_class(labels, n_cls, args.knn_per_class)
        knn = KNNClassifier(n_cls, k=args.knn).fit(emb, labels)
        Path(args.knn_bank).parent.mkdir(parents=True, exist_ok=True)
        knn.save(args.knn_bank)
        loo = f"{knn.leave_one_out()[0]:.4f}" if len(knn.bank) else "none (an empty bank)"
        print(f"knn: k = {knn.k}, {len(knn.bank)} labelled tiles in the bank, per class {knn.counts.tolist()}, "
              f"leave-one-out accuracy {loo} -> {args.knn_bank}", flush=True)
    else:
        knn = KNNClassifier.load(args.knn_bank, device=run.device)
        knn.k = args.knn
        if knn.n_classes != n_cls or knn.bank.shape[1] != emb.width:
            raise ValueError(f"--knn_bank {args.knn_bank}: {knn.n_classes} classes x {knn.bank.shape[1]} floats do not fit this "
                             f"model and description ({n_cls} x {emb.width})")
    kmap = knn.predict_map(emb, args.downscale_vis)
    save_pictures(run, run.anno_dsc, kmap, mask="knn", overlay="knn_overlay")
    return kmap


def report_similar(run: Run) -> None:
    """--similar_to Y,X: the tiles of this slide most like the tile under that pixel, nearest first, as JSON."""
    args, emb = run.args, run.embeddings
    y, x = args.similar_yx
    if not (y < emb.h and x < emb.w):
        raise ValueError(f"--similar_to {y},{x} lies outside the slide ({emb.h} x {emb.w})")
    res = similar_tiles(emb, (y, x), k=args.similar_k or 16)
    doc = dict(pixel=[y, x], query_row=res["query_row"], query_origin=res["query_origin"].tolist(), patch_size=emb.patch_size,
               k=len(res["rows"]), rows=res["rows"].tolist(), origins=res["origins"].tolist(),
               dist=[float(d) for d in res["dist"]])
    path = Path(args.similar_json) if args.similar_json else run.out_dir / f"{run.stem}_similar.json"
    write_json(path, doc)
    print(f"similar: {len(res['rows'])} tiles like the one at {doc['query_origin']} -> {path}", flush=True)


def report_clusters(run: Run):
    """--clusters / --load_clusters: fit k-means on this slide's embeddings (or apply a saved codebook), write
    `{stem}_clusters.json` and, with visualisations, `{stem}_clusters.jpg`.  Returns (cluster map, its AnnoDescription)."""
    args, emb = run.args, run.embeddings
    if args.load_clusters:
        km = KMeans.load(args.load_clusters, device=run.device)
        if km.centres_.shape[1] != emb.width or (args.clusters is not None and args.clusters != km.n_clusters):
            raise ValueError(f"--load_clusters {args.load_clusters}: {km.n_clusters} clusters x {km.centres_.shape[1]} floats do not fit "
                             f"this run ({'any' if args.clusters is None else args.clusters} x {emb.width})")
        labels, dist = km.predict(emb, return_dist=True)
        sizes = torch.bincount(labels[labels >= 0].to(torch.int64), minlength=km.n_clusters).cpu().numpy().tolist()
        inertia = float(dist.double().sum())
    else:
        km = KMeans(args.clusters, init=args.cluster_init or "kmeans++", seed=args.cluster_seed or 0).fit(emb)
        labels, sizes, inertia = km.labels_, km.counts_.tolist(), km.inertia_
        if args.save_clusters:
            Path(args.save_clusters).parent.mkdir(parents=True, exist_ok=True)
            km.save(args.save_clusters)
    K = km.n_clusters
    print(f"clusters: {K} over {len(emb)} tiles, sizes {sizes}, inertia {inertia:.6g}, "
          + (f"codebook {args.load_clusters}" if args.load_clusters else
             f"{km.n_iter_} iterations, {'converged' if km.converged_ else 'not converged'}"), flush=True)
    dsc = cluster_description(K)
    cmap = cluster_map(emb, labels, K, args.downscale_vis)
    write_json(run.out_dir / f"{run.stem}_clusters.json", dict(
        n_clusters=K, n_tiles=len(emb), sizes=sizes, inertia=inertia, iterations=km.n_iter_, converged=km.converged_,
        init=km.init, seed=km.seed, normalize=km.normalize, fitted_here=not args.load_clusters,
        colors={a.label: list(a.color) for a in dsc.anno_classes}))
    save_pictures(run, dsc, cmap, overlay="clusters")
    return cmap, dsc


def report_pca(run: Run) -> None:
    """--pca / --load_pca: fit a principal-component basis on this slide's embeddings (or apply a saved one), write
    `{stem}_pca.json` and, with visualisations, `{stem}_pca.jpg`: the first min(3, N) components as red, green and blue."""
    args, emb, device = run.args, run.embeddings, run.device
    if args.load_pca:
        pca = PCA.load(args.load_pca, device=device)
        if pca.components_.shape[1] != emb.width:
            raise ValueError(f"--load_pca {args.load_pca}: a basis of {pca.components_.shape[1]} columns does not fit this run "
                             f"({emb.width})")
    else:
        pca = PCA(args.pca).fit(emb)
        if args.save_pca:
            Path(args.save_pca).parent.mkdir(parents=True, exist_ok=True)
            pca.save(args.save_pca)
    N = pca.n_components
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    pca.transform(emb)
    torch.cuda.synchronize(device)
    project_ms = 1e3 * (time.perf_counter() - t0)
    ratio = pca.explained_variance_ratio_
    print(f"pca: {N} components over {len(emb)} tiles, explained variance {float(ratio.sum()):.4f} "
          f"(first {float(ratio[0]):.4f}), " + (f"basis {args.load_pca}" if args.load_pca else f"fitted on {pca.n_samples_} rows"),
          flush=True)
    write_json(run.out_dir / f"{run.stem}_pca.json", dict(
        n_components=N, n_tiles=len(emb), n_samples=pca.n_samples_, explained_variance=pca.explained_variance_.tolist(),
        explained_variance_ratio=ratio.tolist(), scatter_ms=pca.timings_.get("scatter_ms"), eigen_ms=pca.timings_.get("eigen_ms"),
        project_ms=project_ms, fitted_here=not args.load_pca))
    if not args.no_visualizations:
        _save_jpeg(pca.colour_map(emb, args.downscale_vis, components=tuple(range(min(3, N)))), run.out_dir / f"{run.stem}_pca.jpg")


def report(run: Run) -> None:
    """The embedding steps in their order.  --knn and --clusters replace the map the region flags describe (`run.pred`), --clusters
    its description too."""
    args = run.args
    if args.prototypes:
        report_prototypes(run)
    if args.pca is not None or args.load_pca:
        report_pca(run)
    if args.similar_to is not None:
        report_similar(run)
    if args.knn is not None:
        run.pred = report_knn(run)
    if args.clusters is not None or args.load_clusters:
        run.pred, run.anno_dsc = report_clusters(run)
