"""The predict CLI's score against an annotation: `--anno`, `--score_json`.

`--anno PATH` scores the class map against the slide's polygon annotation (rank 0): prints the table
and writes `{stem}_truth.jpg` and `{stem}_errors.jpg`; `--score_json PATH` writes the figures and the annotation's counts."""
from __future__ import annotations

import json
from pathlib import Path

from ..scoring import save_score, score_prediction
from ..visualize import KNOWN_COLORS
from .common import Run, existing_file, need


def add_flags(ap) -> None:
    ap.add_argument("--anno", default=None, metavar="PATH",
                    help="the slide's annotation JSON: score the class map against it; writes {stem}_truth.jpg, {stem}_errors.jpg")
    ap.add_argument("--score_json", default=None, metavar="PATH", help="with --anno: the score and the annotation's counts as JSON")


def anno_from_args(ap, args):
    """The records of --anno (None without it); a missing file, an annotation without a region of a known class and
    --score_json without --anno are argparse errors."""
    need(ap, args.anno or not args.score_json, "--score_json needs --anno")
    if not args.anno:
        return None
    existing_file(ap, "--anno", args.anno)
    try:
        records = json.loads(Path(args.anno).read_text())
        known = [a for a in records if a["class"] in KNOWN_COLORS]
    except (ValueError, TypeError, KeyError) as e:
        ap.error(f"--anno {args.anno}: not a JSON list of {{class, vertices}} records ({e!r})")
    need(ap, known, f"--anno {args.anno}: none of its {len(records)} regions belongs to a known class ({', '.join(KNOWN_COLORS)})")
    return records


def check(ap, args, model=None) -> None:
    """Leaves the records of --anno (or None) in `args.anno_records`."""
    args.anno_records = anno_from_args(ap, args)


def report(run: Run) -> None:
    """--anno: prints the score of `run.pred` and the annotation's counts, writes --score_json and leaves the annotation's label
    map and the outcome map in `run.truth` and `run.outcome` for the pictures and the distance steps."""
    args = run.args
    score, run.truth, run.outcome, anno_info = score_prediction(run.pred, args.anno_records, run.anno_dsc, args.layer, run.smp.h,
                                                                run.smp.w, args.downscale_vis, return_maps=True, device=run.device)
    print(score, flush=True)
    print(f"annotation: {anno_info['n_rings']} rings of {anno_info['n_regions']} regions, "
          f"{anno_info['skipped_class']} of unknown class, {anno_info['failed']} failed to parse", flush=True)
    if args.score_json:
        save_score(args.score_json, score, anno_info)
