"""What the predict CLI does to the slide before anything reads it: `--pyramid`, `--stain*`.

`--pyramid` makes `--layer L` of a `--synthetic` slide or a `.npy` image the slide at 1/L of its resolution (DESIGN.md section
4.14): the exact area average, built on the device; everything below reads that layer, and `--stain` normalises it.
`--stain macenko` normalises the slide's stain appearance first (resident slide): the prediction, the
tissue filter and the overlays all read the normalised slide; `--stain_target PATH` takes another slide's saved fit as the
target instead of the default constants, `--save_stain_fit PATH` writes this slide's fit (rank 0)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from ..patch_samplers.full_samplers import FullImageDenseSampler
from ..stain import StainFit, StainNormalizer
from .common import existing_file, need


def add_flags(ap) -> None:
    ap.add_argument("--pyramid", action="store_true",
                    help="--layer L of a --synthetic slide or a .npy image is the slide at 1/L of its resolution, area-averaged on the "
                         "device (PyramidSlide); without it such a slide has one layer, whatever --layer says")
    ap.add_argument("--stain", choices=["off", "macenko"], default="off",
                    help="normalise the slide's stain appearance on the device before anything reads it (resident slide); "
                         "with --pyramid the layer is normalised, not the base")
    ap.add_argument("--stain_target", default=None, metavar="PATH", help="with --stain: a StainFit JSON (another slide's fit) as the target")
    ap.add_argument("--save_stain_fit", default=None, metavar="PATH", help="with --stain: this slide's StainFit as JSON (rank 0)")


def pyramid_from_args(ap, args) -> None:
    """Checks --pyramid; a bad combination is an argparse error."""
    if not args.pyramid:
        return
    need(ap, not args.ondisk, "--pyramid holds the layer resident in HBM; it cannot be combined with --ondisk")
    need(ap, args.synthetic is not None or Path(args.image).suffix == ".npy",
         f"--pyramid serves the layers of a --synthetic slide or a .npy image; {args.image} goes to psimage, "
         "which has layers of its own")


def stain_from_args(ap, args) -> StainNormalizer | None:
    """The StainNormalizer of the --stain flags, or None for `--stain off`; a bad combination is an argparse error."""
    if args.stain == "off":
        need(ap, not (args.stain_target or args.save_stain_fit), "--stain_target and --save_stain_fit need --stain macenko")
        return None
    need(ap, not args.ondisk, "--stain needs the slide resident in HBM; it cannot be combined with --ondisk")
    if args.stain_target:
        existing_file(ap, "--stain_target", args.stain_target)
        try:
            target = StainFit.from_json(Path(args.stain_target).read_text())
            return StainNormalizer(args.stain, target=target)
        except (ValueError, TypeError) as e:
            ap.error(f"--stain_target {args.stain_target}: not a usable StainFit ({e})")
    return StainNormalizer(args.stain)


def check(ap, args, model=None) -> None:
    """Leaves the StainNormalizer (or None) in `args.stain_norm`."""
    pyramid_from_args(ap, args)
    args.stain_norm = stain_from_args(ap, args)


def prepare(args, img, mode, device, rank):
    """The slide every route and the overlays read: the layer under --pyramid, normalised under --stain (rank 0 prints the fit
    and writes --save_stain_fit)."""
    if args.pyramid:
        # the layer takes the slide's place for every route below and for the overlays; --stain then
        # normalises the layer.  A .npy image goes up in bands, so HBM holds the layer and one band, never the whole scan
        from ..resample import PyramidSlide
        img = PyramidSlide(img, device=device).layer_device(args.layer)
    if args.stain_norm is not None:
        # the normalised slide takes the raw one's place for every route below and for the overlays (the map and the picture
        # under it must agree); every rank normalises its own copy, integer-exact, so all hold the same pixels
        if not isinstance(img, torch.Tensor):
            img = FullImageDenseSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                        mode=mode, stride=args.stride, device=device).data_device
        sinfo: dict = {}
        img = args.stain_norm.normalize(img, sinfo)
        fit = sinfo["fit"]
        if rank == 0:
            print(f"stain: identity fit ({fit.reason})" if fit.identity else
                  f"stain: {fit.n_stained} stained pixels, HE {np.round(np.array(fit.HE).T, 4).tolist()}, "
                  f"maxC {np.round(fit.maxC, 4).tolist()}", flush=True)
            if args.save_stain_fit:
                Path(args.save_stain_fit).parent.mkdir(parents=True, exist_ok=True)
                Path(args.save_stain_fit).write_text(fit.to_json())
    return img
