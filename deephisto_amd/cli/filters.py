"""Which tiles the predict CLI classifies: `--tissue*`, `--min_sharpness`, `--max_ink`, `--quality_*`.

`--tissue otsu|<0..255>` classifies only the tiles that hold tissue (dense branch, resident slide; TissueFilter), with
`--tissue_min_fraction` and `--tissue_fill` (a class label, or -1 for no class) for the cells no kept tile covers.
`--min_sharpness N` and `--max_ink F` leave out the out-of-focus and the ink-marked tiles among those (DESIGN.md section 4.16;
QualityFilter; dense branch, resident slide; either switches the filter on, as does `--quality_fill`, which must name the
class of `--tissue_fill` when both filters run); `--quality_json PATH` writes thresholds, counts and the quartiles of the
scored tiles' sharpness (rank 0), from which to pick N."""
from __future__ import annotations

from ..quality import QualityFilter, sharpness_summary
from ..tissue import TissueFilter
from .common import dense_resident_only, fill_class, need, write_json


def add_flags(ap) -> None:
    ap.add_argument("--tissue", default="off", metavar="{off,otsu,<int>}",
                    help="classify only tiles with tissue: chroma threshold 'otsu' or 0..255 (dense branch only)")
    ap.add_argument("--tissue_min_fraction", type=float, default=0.25,
                    help="share of a tile's pixels that must be tissue (0.25: a conventional default, not validated here)")
    ap.add_argument("--tissue_fill", default="-1", help="class label for cells no kept tile covers, or -1 (no class)")
    ap.add_argument("--min_sharpness", type=int, default=None, metavar="N",
                    help="reject out-of-focus tiles: Laplacian variance of the luma over a tile's tissue pixels below N grey levels "
                         "squared (0..1040400; dense branch only; --quality_json reports the slide's quartiles)")
    ap.add_argument("--max_ink", type=float, default=None, metavar="F",
                    help="reject tiles with more than the share F of pen-mark or very dark pixels (0..1)")
    ap.add_argument("--quality_fill", default=None, help="class label for cells no kept tile covers, or -1 (as --tissue_fill)")
    ap.add_argument("--quality_json", default=None, metavar="PATH",
                    help="with the quality filter: thresholds, counts and the sharpness quartiles of the scored tiles as JSON (rank 0)")


def tissue_from_args(ap, args) -> TissueFilter | None:
    """The TissueFilter of the --tissue flags, or None for `--tissue off`; a bad combination is an argparse error."""
    if args.tissue == "off":
        return None
    dense_resident_only(ap, args, "--tissue")
    fill = fill_class(ap, "--tissue_fill", args.tissue_fill)
    try:
        threshold = "otsu" if args.tissue == "otsu" else int(args.tissue)
    except ValueError:
        ap.error(f"--tissue must be off, otsu or an integer threshold in [0, 255], not {args.tissue!r}")
    try:
        return TissueFilter(threshold, args.tissue_min_fraction, fill)
    except ValueError as e:
        ap.error(f"--tissue {args.tissue} / --tissue_min_fraction {args.tissue_min_fraction}: {e}")


def quality_from_args(ap, args) -> QualityFilter | None:
    """The QualityFilter of --min_sharpness / --max_ink / --quality_fill (any of them switches it on), or None; a bad
    combination is an argparse error."""
    if args.min_sharpness is None and args.max_ink is None and args.quality_fill is None:
        need(ap, not args.quality_json, "--quality_json needs --min_sharpness, --max_ink or --quality_fill")
        return None
    dense_resident_only(ap, args, "the quality filter")
    spelled = args.quality_fill if args.quality_fill is not None else "-1"
    fill = fill_class(ap, "--quality_fill", spelled)
    try:
        filt = QualityFilter(0 if args.min_sharpness is None else args.min_sharpness,
                             1.0 if args.max_ink is None else args.max_ink, fill_class=fill)
    except ValueError as e:
        ap.error(f"--min_sharpness {args.min_sharpness} / --max_ink {args.max_ink}: {e}")
    need(ap, 0 < args.patch_size <= 1024, f"the quality filter takes --patch_size in [1, 1024], not {args.patch_size}")
    need(ap, args.tissue_filter is None or args.tissue_filter.fill_class == filt.fill_class,
         f"--tissue_fill {args.tissue_fill} and --quality_fill {spelled} must name the same class")
    return filt


def check(ap, args, model=None) -> None:
    """Leaves the TissueFilter (or None) in `args.tissue_filter` and the QualityFilter (or None) in `args.quality_filter`."""
    args.tissue_filter = tissue_from_args(ap, args)
    args.quality_filter = quality_from_args(ap, args)


def report_kept(args, info: dict, qinfo: dict) -> None:
    """Rank 0's lines on what the two filters kept, and --quality_json: the filter's thresholds, the counts and the five-number
    summary of the scored tiles' sharpness."""
    if args.tissue_filter is not None:
        print(f"kept {info['n_kept']} of {info['n_tiles']} tiles, threshold {info['threshold']}", flush=True)
    filt = args.quality_filter
    if filt is None:
        return
    print(f"quality: {qinfo['n_kept']} of {qinfo['n_tiles']} tiles pass, {qinfo['rejected_blur']} blurred "
          f"(min_sharpness {qinfo['min_sharpness']}), {qinfo['rejected_ink']} ink-marked "
          f"(more than {qinfo['max_ink_pixels']} pixels)", flush=True)
    if args.quality_json:
        write_json(args.quality_json, dict(
            min_sharpness=qinfo["min_sharpness"], max_ink_fraction=filt.max_ink_fraction, max_ink_pixels=qinfo["max_ink_pixels"],
            ink_chroma=filt.ink_chroma, ink_margin=filt.ink_margin, dark_max=filt.dark_max, fill_class=filt.fill_class,
            threshold=qinfo["threshold"], n_tiles=qinfo["n_tiles"], n_kept=qinfo["n_kept"],
            rejected_blur=qinfo["rejected_blur"], rejected_ink=qinfo["rejected_ink"],
            sharpness=sharpness_summary(qinfo["stats"])))
