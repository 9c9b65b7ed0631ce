"""The distance steps of the predict CLI: `--margin`, `--score_tolerance`, `--surface`, `--distance_json`.

`--margin LABEL:PX[,PX...]` cuts the map into bands of distance around class LABEL (edges in layer
pixels, negative inside the class, a single PX meaning `-PX,0,PX`), prints the classes per band and writes `{stem}_margin.jpg`,
one colour per band over the slide.  With `--anno`, `--score_tolerance PX` adds a score that leaves out the cells within PX
of a label change of the annotation and `--surface` the Hausdorff, HD95 and average symmetric surface distance of every class
the annotation holds.  `--distance_json PATH` writes all three as one report (rank 0).  They run on the map the region flags
describe (the cleaned one under `--min_region`) and are refused with `--clusters`; every other output is that of a run
without them."""
from __future__ import annotations

import torch

from ..anno.utils import AnnoDescription
from ..clustering import cluster_palette
from ..distance import band_composition, check_edges, margin_bands, save_distance_report, surface_distances, tolerant_score
from ..visualize import KNOWN_COLORS
from .common import Run, need, save_pictures


def add_flags(ap) -> None:
    ap.add_argument("--margin", default=None, metavar="LABEL:PX[,PX...]",
                    help="bands of distance around class LABEL, edges in layer pixels, negative inside the class (a single PX means "
                         "-PX,0,PX): prints the classes per band and writes {stem}_margin.jpg (rank 0)")
    ap.add_argument("--score_tolerance", type=int, default=None, metavar="PX",
                    help="with --anno: a second score that leaves out the cells within PX layer pixels of a label change of the annotation")
    ap.add_argument("--surface", action="store_true",
                    help="with --anno: Hausdorff, HD95 and average symmetric surface distance of every class the annotation holds")
    ap.add_argument("--distance_json", default=None, metavar="PATH",
                    help="with --margin, --score_tolerance or --surface: their results as one JSON (rank 0)")


def check(ap, args, model=None) -> None:
    """Checks --margin / --score_tolerance / --surface / --distance_json; leaves (label, edges in px) of --margin in
    `args.margin_spec` (None without the flag).  A bad combination is an argparse error."""
    args.margin_spec = None
    need(ap, args.score_tolerance is None or args.anno, "--score_tolerance needs --anno")
    need(ap, not args.surface or args.anno, "--surface needs --anno")
    need(ap, args.score_tolerance is None or args.score_tolerance >= 0, f"--score_tolerance must be >= 0, not {args.score_tolerance}")
    steps = [f for f, on in (("--margin", args.margin is not None), ("--score_tolerance", args.score_tolerance is not None),
                             ("--surface", args.surface)) if on]
    need(ap, steps or not args.distance_json, "--distance_json needs --margin, --score_tolerance or --surface")
    if steps and (args.clusters is not None or args.load_clusters):
        ap.error(f"{steps[0]} names the classes of the description; it cannot be combined with --clusters, whose map holds clusters")
    if args.margin is None:
        return
    label, sep, spelled = args.margin.partition(":")
    need(ap, sep and spelled, f"--margin takes LABEL:PX[,PX...], not {args.margin!r}")
    need(ap, label in KNOWN_COLORS, f"--margin label must be out of {', '.join(KNOWN_COLORS)}, not {label!r}")
    try:
        edges = [int(v) for v in spelled.split(",")]
    except ValueError:
        ap.error(f"--margin takes LABEL:PX[,PX...] with integer PX, not {args.margin!r}")
    if len(edges) == 1:
        need(ap, edges[0] > 0, f"--margin {args.margin}: a single PX must be > 0 (it stands for -PX,0,PX)")
        edges = [-edges[0], 0, edges[0]]
    try:
        edges = check_edges(edges)
    except ValueError:
        ap.error(f"--margin {args.margin}: the edges must ascend strictly (and stay below 2^31 px, at most 64 bands)")
    args.margin_spec = (label, edges)


def report(run: Run) -> None:
    """--margin / --score_tolerance / --surface on `run.pred` (the map the region flags describe) and `run.truth` (the annotation's
    label map, None without --anno): prints the figures, writes `{stem}_margin.jpg` and the report of --distance_json."""
    args, pred, truth, device = run.args, run.pred, run.truth, run.device
    labels = [""] * (max(a.id for a in run.anno_dsc.anno_classes) + 1)
    for a in run.anno_dsc.anno_classes:
        labels[a.id] = a.label
    d = args.downscale_vis
    margin = tolerant = surface = None
    if args.margin_spec is not None:
        label, edges = args.margin_spec
        bands = margin_bands(pred, [labels.index(label)], edges, d, device=device)
        counts = band_composition(pred, bands, len(labels), len(edges) - 1)
        margin = dict(label=label, edges_px=edges, class_labels=labels, counts=counts)
        print(f"margin of {label}, edges {edges} px; cells per band of {', '.join(labels)}, no class:", flush=True)
        for i, row in enumerate(counts.tolist()):
            print(f"  [{edges[i]}, {edges[i + 1]}) {row}", flush=True)
        dsc = AnnoDescription.with_known_colors({f"band_{i}": c for i, c in enumerate(cluster_palette(len(edges) - 1))})
        save_pictures(run, dsc, bands, overlay="margin")
    if args.score_tolerance is not None:
        score = tolerant_score(pred, truth, labels, args.score_tolerance, d, device=device)
        tolerant = dict(tolerance_px=args.score_tolerance, score=score)
        print(f"score without the cells within {args.score_tolerance} px of a label change:", flush=True)
        print(score, flush=True)
    if args.surface:
        held = torch.bincount(truth[truth >= 0].to(torch.int64), minlength=len(labels)).cpu().tolist()
        surface = {labels[k]: surface_distances(pred, truth, k, d, device=device) for k in range(len(labels)) if held[k] and labels[k]}
        for lb, s in surface.items():
            print(f"surface {lb}: hausdorff {s.hausdorff:.1f} px, hd95 {s.hd95:.1f} px, assd {s.assd:.2f} px "
                  f"({s.n_pred} predicted, {s.n_truth} annotated boundary cells)", flush=True)
    if args.distance_json:
        save_distance_report(args.distance_json, d, margin=margin, tolerant=tolerant, surface=surface)
