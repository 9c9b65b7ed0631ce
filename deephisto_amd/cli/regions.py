"""The region flags of the predict CLI: `--regions_json`, `--min_region`, `--clean_rounds`, `--export_anno`.

`--regions_json PATH` writes the table of the map's connected regions (rank 0); `--min_region CELLS
[--clean_rounds R]` first gives regions below CELLS cells the class of their large neighbours and writes
`{stem}_clean_mask.jpg` and `{stem}_clean_overlay.jpg`; `--export_anno PATH` writes the regions as polygons in the
annotation's JSON format.  The returned map and the three standard JPEGs are those of a run without these flags, and
`--anno` keeps scoring the uncleaned map (the cleaned one gets a second score)."""
from __future__ import annotations

from ..regions import export_annotation, extract_regions, save_regions
from ..scoring import score_prediction
from .common import Run, need, save_pictures


def add_flags(ap) -> None:
    ap.add_argument("--regions_json", default=None, metavar="PATH", help="the table of the map's connected regions as JSON (rank 0)")
    ap.add_argument("--min_region", type=int, default=None, metavar="CELLS",
                    help="regions below CELLS cells take their large neighbours' class; writes {stem}_clean_mask.jpg, {stem}_clean_overlay.jpg")
    ap.add_argument("--clean_rounds", type=int, default=None, metavar="R", help="with --min_region: cleanup rounds (default 1)")
    ap.add_argument("--export_anno", default=None, metavar="PATH", help="the regions as polygons in the annotation's JSON format (rank 0)")


def check(ap, args, model=None) -> None:
    """Checks the region flags; a bad combination is an argparse error."""
    need(ap, args.clean_rounds is None or args.min_region is not None, "--clean_rounds needs --min_region")
    need(ap, args.min_region is None or args.min_region >= 1, f"--min_region must be >= 1, not {args.min_region}")
    need(ap, args.clean_rounds is None or args.clean_rounds >= 1, f"--clean_rounds must be >= 1, not {args.clean_rounds}")


def report(run: Run):
    """The region flags: table, cleanup, polygons, the cleaned map's score and JPEGs.  Returns the map they describe: the
    cleaned one under --min_region, else `run.pred`."""
    args, anno_dsc = run.args, run.anno_dsc
    res = extract_regions(run.pred, anno_dsc, args.layer, args.downscale_vis, min_cells=args.min_region or 0,
                          rounds=args.clean_rounds or 1, polygons=bool(args.export_anno), device=run.device,
                          confidence=run.proba.confidence if run.proba is not None else None)
    print(f"regions: {res.k}" + (f", cleanup below {args.min_region} cells changed {res.n_changed} cells" if args.min_region else "")
          + (f", traced in {res.trace_s:.3f} s" if args.export_anno else ""), flush=True)
    if args.regions_json:
        save_regions(args.regions_json, res.regions, anno_dsc, args.downscale_vis, args.layer,
                     dict(min_region=args.min_region, clean_rounds=args.clean_rounds, n_changed=res.n_changed))
    if args.export_anno:
        export_annotation(args.export_anno, res.regions, res.polygons, anno_dsc)
    if args.min_region is None:
        return run.pred
    if args.anno_records is not None:
        print("cleaned map:", flush=True)
        print(score_prediction(res.class_map, args.anno_records, anno_dsc, args.layer, run.smp.h, run.smp.w, args.downscale_vis,
                               device=run.device), flush=True)
    save_pictures(run, anno_dsc, res.class_map, mask="clean_mask", overlay="clean_overlay")
    return res.class_map
