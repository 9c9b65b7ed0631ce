"""What a whole-slide run writes for people to look at (re-exported by examples/predict_full_patched.py): the class colours,
`perform_and_save_visualizations` (mask, slide and overlay JPEGs; confidence and heat maps of DESIGN.md section 4.8; the truth and
error maps of section 4.9) and `save_proba` (the probabilities as .npy files)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import tiles
from .psimage_compat import open_slide

KNOWN_COLORS = {   # predict_full_patched.py:139-148
    "AT": (245, 119, 34),    # orange
    "BG": (153, 255, 255),   # cyan
    "LP": (64, 170, 72),     # green
    "MM": (255, 0, 0),       # red
    "TUM": (33, 67, 156),    # blue
}


ERROR_COLORS = {"correct": (0, 255, 0), "wrong": (255, 0, 0)}   # the 2-row LUT of the outcome map (0, 1)


def _save_jpeg(array, path) -> None:
    """uint8[h, w, 3] (NumPy array or tensor) as a JPEG of quality 95, the reference's setting (predict_full_patched.py:98-113)."""
    from PIL import Image

    if isinstance(array, torch.Tensor):
        array = array.cpu().numpy()
    Image.fromarray(array).save(path, quality=95)


def perform_and_save_visualizations(img, anno_dsc, pred, out_dir: Path = Path("."), stem: str | None = None,
                                    alpha: float = 0.6, save: bool = True, device="cuda", proba=None, heat_classes=(),
                                    truth=None, outcome=None):
    """Colourised class mask, the slide at the map's resolution and their overlay -- predict_full_patched.py:81-113.

    `img`: path (psimage, when installed: `get_region(..., target_hw)` as the reference) or a uint8[H,W,3]
    array / GPU tensor, which is sampled at the map's resolution by nearest source pixel (psimage's own
    resampler is third-party and unknown here).  The colour lookup and the float64 blend run on the GPU
    (`dh_colorize_map`, `dh_overlay_blend`) and are bit-identical to the reference's NumPy lines.
    `proba`: the run's tiles.SlideProbabilities; with `save`, `{stem}_confidence.jpg` (the confidence in white over the slide)
    and one `{stem}_heat_{label}.jpg` per label of `heat_classes` (that class's mean probability in the class colour) are
    written as well (`dh_heatmap_blend`, float64 like the overlay).
    `truth` / `outcome`: the label map and the outcome map of a scored run (`scoring.score_prediction(..., return_maps=True)`);
    with `save`, `{stem}_truth.jpg` (the labels in the class colours, unlabelled cells black) and `{stem}_errors.jpg` (correct
    cells green, wrong cells red, blended over the slide with `alpha` like the overlay; unlabelled cells black) are written.
    Returns (mask, image, overlay) as uint8[h, w, 3] NumPy arrays; JPEGs are written when `save`."""
    dev = torch.device(device)
    by_label = {a.label: a for a in anno_dsc.anno_classes}
    unknown = [lb for lb in heat_classes if lb not in by_label]
    if unknown or (heat_classes and proba is None):
        raise ValueError(f"heat_classes {list(heat_classes)}: needs proba and labels out of {', '.join(by_label)}")
    pred_t = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred))
    pred_t = pred_t.to(dev, torch.int64).contiguous()
    h, w = int(pred_t.shape[0]), int(pred_t.shape[1])
    n_ids = max((a.id for a in anno_dsc.anno_classes), default=-1) + 1
    lut = torch.zeros((n_ids, 3), dtype=torch.uint8)
    for a in anno_dsc.anno_classes:
        lut[a.id] = torch.tensor(a.color, dtype=torch.uint8)
    colored = tiles.colorize_map(pred_t, lut)
    if isinstance(img, (str, Path)):
        stem = stem or Path(img).stem
        with open_slide(img) as psim:
            small = torch.from_numpy(np.ascontiguousarray(psim.get_region((0, 0), (psim.height, psim.width), target_hw=(h, w)))).to(dev)
    else:
        full = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
        full = full.to(dev)
        ys = (torch.arange(h, device=dev) * full.shape[0]) // h
        xs = (torch.arange(w, device=dev) * full.shape[1]) // w
        small = full[ys][:, xs].contiguous()
    overlay = tiles.overlay_blend(small, colored, alpha)
    mask_np, img_np, ov_np = colored.cpu().numpy(), small.cpu().numpy(), overlay.cpu().numpy()
    if save:
        out_dir = Path(out_dir)
        out_dir.mkdir(exist_ok=True, parents=True)
        stem = stem or "slide"
        _save_jpeg(mask_np, out_dir / f"{stem}_mask.jpg")
        _save_jpeg(img_np, out_dir / f"{stem}.jpg")
        _save_jpeg(ov_np, out_dir / f"{stem}_overlay.jpg")
        if proba is not None:
            _save_jpeg(tiles.heatmap_blend(small, proba.confidence.to(dev), (255, 255, 255), alpha), out_dir / f"{stem}_confidence.jpg")
            for lb in heat_classes:
                heat = tiles.heatmap_blend(small, proba.proba.to(dev)[..., by_label[lb].id], by_label[lb].color, alpha)
                _save_jpeg(heat, out_dir / f"{stem}_heat_{lb}.jpg")
        if truth is not None:
            _save_jpeg(tiles.colorize_map(truth.to(dev, torch.int64).contiguous(), lut), out_dir / f"{stem}_truth.jpg")
        if outcome is not None:
            two = torch.tensor([ERROR_COLORS["correct"], ERROR_COLORS["wrong"]], dtype=torch.uint8)
            errors = tiles.overlay_blend(small, tiles.colorize_map(outcome.to(dev, torch.int64).contiguous(), two), alpha)
            _save_jpeg(errors, out_dir / f"{stem}_errors.jpg")
    return mask_np, img_np, ov_np


def save_proba(path, proba) -> tuple[Path, Path]:
    """Writes `proba.proba` as float16 to `path` (.npy) and `proba.count` to the same name with `_count` before the suffix."""
    path = Path(path)
    if path.suffix != ".npy":
        path = path.with_name(path.name + ".npy")
    path.parent.mkdir(exist_ok=True, parents=True)
    count_path = path.with_name(path.stem + "_count.npy")
    np.save(path, proba.proba.cpu().numpy().astype(np.float16))
    np.save(count_path, proba.count.cpu().numpy())
    return path, count_path
