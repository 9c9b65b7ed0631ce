"""How the predict CLI finishes the map from the forward pass: `--tta`, `--fine`, `--proba`, `--heat`, `--save_proba`.

`--tta flips|d4` classifies every tile in four or all eight orientations of the square and averages the logits per tile
(both fused routes, resident slide; refused with `--ondisk` and for a foreign model on the callback
route); overlays, scoring and regions read the untransformed slide and the map, as without it.
`--fine` builds the map from the class activation maps of the last conv (`predict_fine_patched`): every
tile's S x S per-position scores, S = patch_size / 32, go onto their own 32 x 32-pixel blocks, so the map's values change
every 32 px instead of once per tile footprint, from the same forward pass.  The canvas shape does not move: `--proba`,
`--heat`, `--save_proba`, `--anno`, the region flags, `--tissue`, the quality flags and `--stain` compose with it.  Dense
branch, resident slide, `--patch_size` a multiple of 32; refused with `--tta`, `--random_sampler`, `--ondisk` and the
embedding flags.
`--proba` also computes the per-cell mean softmax probabilities and writes the confidence JPEG;
`--heat LABEL ...` adds one heat map per class label; `--save_proba PATH` writes the probabilities as float16 PATH(.npy) and
the hit counts as PATH_count.npy (rank 0).  The returned class map stays the argmax of the logit sums."""
from __future__ import annotations

from ..models.patch_cls_simple.engine import ResNetHIP
from ..tta import TestTimeAugmenter
from ..visualize import KNOWN_COLORS
from .common import dense_resident_only, embedding_flags, need


def add_flags(ap) -> None:
    ap.add_argument("--tta", choices=["off", "flips", "d4"], default="off",
                    help="test-time augmentation: classify every tile in 4 (flips) or all 8 (d4) orientations of the square and "
                         "average the logits (resident slide; 4 / 8 times the forward work)")
    ap.add_argument("--fine", action="store_true",
                    help="the map from the class activation maps of the last conv: values change every 32 px, same forward pass "
                         "(dense sampler, resident slide, --patch_size a multiple of 32)")
    ap.add_argument("--proba", action="store_true", help="per-cell mean softmax probabilities; writes {stem}_confidence.jpg")
    ap.add_argument("--heat", nargs="+", default=[], metavar="LABEL",
                    help=f"with --proba: one {{stem}}_heat_LABEL.jpg per class label ({', '.join(KNOWN_COLORS)})")
    ap.add_argument("--save_proba", default=None, metavar="PATH",
                    help="with --proba: probabilities as float16 PATH(.npy), hit counts as PATH_count.npy (rank 0)")


def tta_from_args(ap, args, model=None) -> TestTimeAugmenter | None:
    """The TestTimeAugmenter of --tta, or None for `--tta off`; a bad combination is an argparse error.  `model`: the module
    injected into main, if any: a foreign one under --random_sampler goes the callback route, which has no views."""
    if args.tta == "off":
        return None
    need(ap, not args.ondisk, "--tta needs the slide resident in HBM; it cannot be combined with --ondisk")
    need(ap, not (args.random_sampler and model is not None and not isinstance(model, ResNetHIP)),
         "--tta runs on the fused routes (a ResNet18HIP or ResNet50HIP model); under --random_sampler a foreign model "
         "goes through the per-batch callback, which has no views")
    return TestTimeAugmenter(args.tta)


def check_tta(ap, args, model=None) -> None:
    """Leaves the TestTimeAugmenter (or None) in `args.tta_aug`."""
    args.tta_aug = tta_from_args(ap, args, model)


def proba_from_args(ap, args, model=None) -> None:
    """Checks the --proba flags; a bad combination or an unknown class label is an argparse error."""
    need(ap, args.proba or not args.heat, "--heat needs --proba")
    need(ap, args.proba or not args.save_proba, "--save_proba needs --proba")
    for lb in args.heat:
        need(ap, lb in KNOWN_COLORS, f"--heat labels must be out of {', '.join(KNOWN_COLORS)}, not {lb!r}")


def fine_from_args(ap, args, model=None) -> None:
    """Checks --fine; a bad combination is an argparse error."""
    if not args.fine:
        return
    dense_resident_only(ap, args, "--fine")
    need(ap, args.tta == "off", "--fine places every position of a tile's last feature map; a rotated view permutes them: it cannot be "
                                "combined with --tta")
    for flag, on in embedding_flags(args):
        need(ap, not on, f"{flag} finishes the class map from one logits row per tile; it cannot be combined with --fine")
    need(ap, args.patch_size % 32 == 0, f"--fine needs a --patch_size that is a multiple of 32, not {args.patch_size}")
