"""The command line of examples/predict_full_patched.py, one module per flag group: each owns its flags (`add_flags`), its checks
and what rank 0 reports for it; common.py holds what they share.  A new group is one module and one line in each of FLAGS and
CHECKS.  Both orders are behaviour: FLAGS is the order of `--help`, CHECKS decides which message a command line that breaks
two rules gets."""
from __future__ import annotations

import argparse
from pathlib import Path

import torch

from ..anno.utils import AnnoDescription
from ..visualize import KNOWN_COLORS, perform_and_save_visualizations, save_proba
from . import base, distance, embed, filters, regions, routes, scoring, slide
from .common import Run

FLAGS = (base.add_flags, filters.add_flags, slide.add_flags, routes.add_flags, scoring.add_flags, regions.add_flags, embed.add_flags,
         distance.add_flags)
CHECKS = (regions.check, slide.check, filters.check, routes.check_tta, scoring.check, routes.proba_from_args, embed.check,
          routes.fine_from_args, distance.check)


def build_parser(description: str) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=description)
    for add_flags in FLAGS:
        add_flags(ap)
    return ap


def check_args(ap, args, model=None) -> None:
    """The flag checkers, before the process group or any GPU is touched; leaves the TissueFilter (or None) in
    `args.tissue_filter`, the QualityFilter (or None) in `args.quality_filter`, the StainNormalizer (or None) in `args.stain_norm`,
    the TestTimeAugmenter (or None) in `args.tta_aug`, the records of --anno (or None) in `args.anno_records`, the (label, edges) of
    --margin in `args.margin_spec` and the pixel of --similar_to in `args.similar_yx`.  `model`: the module injected into main,
    if any."""
    for check in CHECKS:
        check(ap, args, model)


def report_rank0(run: Run) -> None:
    """What rank 0, where the map is whole, prints and writes after the prediction: the score, the JPEGs, the probability
    files, then the embedding steps, the regions with the cleaned map's score and JPEGs, and the distance steps on the map the
    regions describe."""
    args = run.args
    run.anno_dsc, run.out_dir = AnnoDescription.with_known_colors(KNOWN_COLORS), Path(args.out_dir)
    run.src = None if args.no_visualizations else run.img if isinstance(run.img, torch.Tensor) or not run.smp.resident else run.smp.data_device
    if args.anno_records is not None:
        scoring.report(run)
    if not args.no_visualizations:
        perform_and_save_visualizations(run.src, run.anno_dsc, run.pred, out_dir=run.out_dir, stem=run.stem, device=run.device,
                                        proba=run.proba, heat_classes=args.heat, truth=run.truth, outcome=run.outcome)
    if args.save_proba:
        save_proba(args.save_proba, run.proba)
    embed.report(run)
    if args.regions_json or args.min_region is not None or args.export_anno:
        run.pred = regions.report(run)   # the cleaned map under --min_region
    if args.margin_spec is not None or args.score_tolerance is not None or args.surface:
        distance.report(run)
