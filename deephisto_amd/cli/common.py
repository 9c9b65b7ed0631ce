"""What the flag groups of the predict CLI share: the record a run's reporters pass around, the list of the embedding flags, the
JSON and picture writers and the small refusals."""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Any

from ..anno.utils import AnnoDescription
from ..visualize import KNOWN_COLORS, _save_jpeg, perform_and_save_visualizations


@dataclass
class Run:
    """One run of the CLI: `_run` fills the prediction (`pred`, `proba`: None without --proba, `embeddings`: the SlideEmbeddings
    of the pass under an embedding flag, else None), `report_rank0` the rest.  `src`: what the pictures are drawn over (None under
    --no_visualizations); `truth`, `outcome`: the annotation's maps (None without --anno).  A reporter that replaces the map the
    later ones describe returns the new one, and `report_rank0` rebinds `pred`."""
    args: Any
    smp: Any
    img: Any
    stem: str
    device: Any
    pred: Any
    proba: Any = None
    embeddings: Any = None
    src: Any = None
    anno_dsc: Any = None
    out_dir: Path | None = None
    truth: Any = None
    outcome: Any = None


def embedding_flags(args) -> list[tuple[str, bool]]:
    """(flag, whether it is on) of every flag that consumes the tile embeddings: these take the features entry of the plan, are
    refused with --tta, --proba and --fine, and run on the dense sampler's grid of a resident slide.  `--clusters 0` counts as
    off, so that it reaches the range check of embed.check whatever else the command line holds; that check lets no 0 through."""
    return [("--save_embeddings", bool(args.save_embeddings)), ("--prototypes", bool(args.prototypes)),
            ("--clusters", bool(args.clusters)), ("--load_clusters", bool(args.load_clusters)),
            ("--pca", args.pca is not None), ("--load_pca", bool(args.load_pca)),
            ("--knn", args.knn is not None), ("--similar_to", args.similar_to is not None)]


def write_json(path, doc) -> None:
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(doc, indent=1) + "\n")


def save_pictures(run: Run, dsc, class_map, mask: str | None = None, overlay: str | None = None) -> None:
    """Visualises `class_map` over the slide without saving the three standard pictures, then writes the mask and / or the overlay
    as `{stem}_{mask}.jpg` / `{stem}_{overlay}.jpg` into the run's out_dir.  Nothing under --no_visualizations."""
    if run.args.no_visualizations:
        return
    pictures = perform_and_save_visualizations(run.src, dsc, class_map, stem=run.stem, save=False, device=run.device)
    run.out_dir.mkdir(exist_ok=True, parents=True)
    for picture, name in ((pictures[0], mask), (pictures[2], overlay)):
        if name:
            _save_jpeg(picture, run.out_dir / f"{run.stem}_{name}.jpg")


def need(ap, cond, msg: str) -> None:
    """An argparse error `msg` unless `cond`."""
    if not cond:
        ap.error(msg)


def existing_file(ap, flag: str, path, hint: str = "") -> None:
    need(ap, Path(path).is_file(), f"{flag} {path}: no such file{hint}")


def dense_resident_only(ap, args, who: str) -> None:
    """`who` (a flag, or a feature by name) runs over the dense sampler's grid of a resident slide: --random_sampler and --ondisk
    are argparse errors."""
    need(ap, not args.random_sampler, f"{who} works on the dense sampler's grid; it cannot be combined with --random_sampler")
    need(ap, not args.ondisk, f"{who} needs the slide resident in HBM; it cannot be combined with --ondisk")


def fill_class(ap, flag: str, spelled: str) -> int:
    """The class id of a --tissue_fill / --quality_fill value: a class label, or -1 for no class."""
    labels = {a.label: a.id for a in AnnoDescription.with_known_colors(KNOWN_COLORS).anno_classes}
    need(ap, spelled == "-1" or spelled in labels, f"{flag} must be one of {', '.join(labels)} or -1, not {spelled!r}")
    return labels.get(spelled, -1)
