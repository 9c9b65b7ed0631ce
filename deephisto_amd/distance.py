"""Distance maps of a whole-slide class map: class masks, the exact Euclidean distance transform, and
what rests on it -- signed distances, round dilation and erosion, margin bands, boundary-tolerant scores, surface distances.

`class_mask` marks a class set, its boundary or every label change (`dh_class_mask`); `distance_transform` gives every cell
the squared distance to the nearest marked cell and, if asked, that cell's index (`dh_distance_transform`).  Everything else
compares those integers: `signed_distance`, `dilate` / `erode` / `open_` / `close`, `margin_bands` with `band_composition`,
`tolerant_score`, `surface_distances`.  torch is used for device memory, streams, comparisons and indexing only; the two
kernels have no CPU fallback.  All results are integers, or float64 figures derived on the host from sorted integers, so
they are the same on every run.
"""
from __future__ import annotations

import json
import math
from dataclasses import asdict, dataclass
from pathlib import Path

import numpy as np
import torch

from . import scoring, tiles
from ._lib import check, lib
from .regions import _as_map

MAX_SIDE = 32767          # kMaxSide of csrc/distance.hip: 2 * 32767^2 < 2^31
MAX_CLASSES = 64
INT32_MAX = 2 ** 31 - 1   # d2 without a feature cell
MODES = {"member": 0, "boundary": 1, "change": 2}


def class_bits(classes) -> int:
    """The 64-bit set of a class list for `dh_class_mask`; a class outside 0 .. 63 raises."""
    bits = 0
    for c in classes:
        if not 0 <= int(c) < MAX_CLASSES:
            raise ValueError(f"class {c} outside 0 .. {MAX_CLASSES - 1}")
        bits |= 1 << int(c)
    return bits


def _check_canvas(shape) -> None:
    if not (1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE):
        raise ValueError(f"a canvas of {shape[0]} x {shape[1]} cells is outside the distance kernels' 1 .. {MAX_SIDE} per side")


def _mask_bits(pred: torch.Tensor, bits: int, include_unclassified: bool, mode: int) -> torch.Tensor:
    _check_canvas(pred.shape)
    dh, dw = pred.shape
    mask = torch.empty((dh, dw), dtype=torch.uint8, device=pred.device)
    with torch.cuda.device(pred.device):
        check(lib().dh_class_mask(pred.data_ptr(), dh, dw, bits, int(bool(include_unclassified)), mode, mask.data_ptr(),
                                  tiles._stream(pred.device)), "dh_class_mask")
    return mask


def class_mask(pred, classes, include_unclassified: bool = False, mode: str = "member", device="cuda") -> torch.Tensor:
    """uint8[dh, dw] (0 / 1) on the device.  A cell is a member when its class is in `classes`, or when it is -1 and
    `include_unclassified` is set.  `mode` "member": the members; "boundary": the members with a 4-neighbour inside the canvas
    that is not a member (the canvas edge makes no boundary); "change": the cells with a 4-neighbour inside the canvas of a
    different value, -1 counting as a value (`classes` is ignored).  `pred`: a class map as `regions` takes it (a device
    tensor, a NumPy array or a finished `SlideProbabilities`) with values in -1 .. 63."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {', '.join(MODES)}, not {mode!r}")
    bits = class_bits(classes)
    return _mask_bits(_as_map(pred, device), bits, include_unclassified, MODES[mode])


def _as_mask(mask, device="cuda") -> torch.Tensor:
    if not isinstance(mask, torch.Tensor):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"a mask is a bool or uint8 map, not {mask.dtype}")
    if mask.dim() != 2 or mask.numel() == 0:
        raise ValueError(f"a mask is a non-empty [dh, dw] array, not {list(mask.shape)}")
    _check_canvas(mask.shape)
    if not mask.is_cuda:
        mask = mask.to(device)
    return mask.to(torch.uint8).contiguous()


def distance_transform(mask, return_nearest: bool = False, device="cuda"):
    """int32[dh, dw] on the device: for every cell the exact minimum over the feature cells (mask != 0) of dy^2 + dx^2, in
    cells.  `return_nearest`: also the int32 map of the linear index y' * dw + x' of the feature cell that attains it, the
    smallest index among equals.  Without a feature cell the distance is `INT32_MAX` and the index -1 everywhere."""
    mask = _as_mask(mask, device)
    dh, dw = mask.shape
    d2 = torch.empty((dh, dw), dtype=torch.int32, device=mask.device)
    nearest = torch.empty((dh, dw), dtype=torch.int32, device=mask.device) if return_nearest else None
    with torch.cuda.device(mask.device):
        work = torch.empty(int(lib().dh_distance_work_size(dh, dw)), dtype=torch.int32, device=mask.device)
        check(lib().dh_distance_transform(mask.data_ptr(), dh, dw, d2.data_ptr(), nearest.data_ptr() if return_nearest else None,
                                          work.data_ptr(), tiles._stream(mask.device)), "dh_distance_transform")
    return (d2, nearest) if return_nearest else d2


def signed_distance(pred, classes, include_unclassified: bool = False, device="cuda") -> torch.Tensor:
    """int32[dh, dw] signed squared distance to the border of a class set, from two transforms: outside the set +d^2 to the
    nearest member (>= 1), inside -d^2 to the nearest cell that is not a member (<= -1); `INT32_MAX` everywhere when the set
    is empty and -`INT32_MAX` when it is the whole canvas."""
    pred = _as_map(pred, device)
    bits = class_bits(classes)
    inside = _mask_bits(pred, bits, include_unclassified, 0)
    outside = _mask_bits(pred, bits ^ (2 ** 64 - 1), not include_unclassified, 0)   # the complement: every value is in one of them
    return torch.where(inside.bool(), -distance_transform(outside), distance_transform(inside))


def dilate(mask, radius_cells: int) -> torch.Tensor:
    """uint8 mask grown by the exact disc of `radius_cells`: the cells with d^2 <= r^2 to a feature cell."""
    r = _radius(radius_cells)
    return (distance_transform(mask) <= r * r).to(torch.uint8)


def erode(mask, radius_cells: int) -> torch.Tensor:
    """uint8 mask shrunk by the exact disc: the cells farther than r from every cell outside the mask (the canvas edge does
    not erode)."""
    r = _radius(radius_cells)
    mask = _as_mask(mask)
    return (distance_transform(mask == 0) > r * r).to(torch.uint8)


def open_(mask, radius_cells: int) -> torch.Tensor:
    """Erosion, then dilation, by the same disc: removes what the disc does not fit into."""
    return dilate(erode(mask, radius_cells), radius_cells)


def close(mask, radius_cells: int) -> torch.Tensor:
    """Dilation, then erosion: fills what the disc does not fit into."""
    return erode(dilate(mask, radius_cells), radius_cells)


def _radius(radius_cells) -> int:
    r = int(radius_cells)
    if r != radius_cells or not 0 <= r <= MAX_SIDE:
        raise ValueError(f"radius_cells = {radius_cells} must be an integer in 0 .. {MAX_SIDE}")
    return r


def _sq(x: int) -> int:
    return x * x if x >= 0 else -x * x


def check_edges(edges_px) -> list[int]:
    """The band edges as a list of ints; anything but a strictly ascending list of at least two integers raises."""
    edges = [int(e) for e in edges_px]
    if len(edges) < 2 or any(int(e) != e for e in edges_px) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"band edges must be at least two strictly ascending integers, not {list(edges_px)}")
    if len(edges) - 1 > MAX_CLASSES or max(abs(e) for e in edges) >= 2 ** 31:
        raise ValueError(f"at most {MAX_CLASSES} bands with edges below 2^31 px")
    return edges


def margin_bands(pred, classes, edges_px, downscale: int, include_unclassified: bool = False, device="cuda") -> torch.Tensor:
    """int64[dh, dw] band map in the class-map format.  `edges_px`: strictly ascending integers in layer pixels, negative
    meaning inside the set, e.g. [-500, 0, 500].  With s the signed squared distance in cells and sq(x) = sign(x) * x^2, a
    cell is in band i when sq(e_i) <= s * downscale^2 < sq(e_i+1), compared in int64: x -> sq(x) is monotone, so this is the
    comparison of the signed distances themselves, without a square root.  Cells outside all bands, and all cells when the
    set or its complement is empty (|s| = INT32_MAX), hold -1."""
    edges = check_edges(edges_px)
    d = int(downscale)
    if not 1 <= d <= 32768:
        raise ValueError(f"downscale = {downscale} outside 1 .. 32768")
    s = signed_distance(pred, classes, include_unclassified, device)
    sd = s.to(torch.int64) * (d * d)
    band = torch.full_like(sd, -1)
    for i, (lo, hi) in enumerate(zip(edges, edges[1:])):
        band = torch.where((sd >= _sq(lo)) & (sd < _sq(hi)), i, band)
    return torch.where(s.abs() == INT32_MAX, -1, band)


def band_composition(pred, bands: torch.Tensor, n_classes: int, n_bands: int) -> torch.Tensor:
    """int64[n_bands, n_classes + 1] (a host tensor): cells of class c in band b, the last column the cells of a band without
    a class.  It is `scoring.confusion` with the bands as the truth."""
    pred = _as_map(pred)
    n = max(int(n_classes), int(n_bands))
    counts = scoring.confusion(pred, bands.to(device=pred.device, dtype=torch.int32).contiguous(), n)
    return torch.cat([counts[:n_bands, :n_classes], counts[:n_bands, n:]], dim=1).contiguous()


@dataclass
class SurfaceDistance:
    """Distances between the boundaries of one class in a prediction and in the truth, in cells times downscale: `hausdorff`,
    `hd95`, `assd`; `n_pred` and `n_truth` are the boundary cells of either.  With an empty side the three figures are nan."""
    n_pred: int
    n_truth: int
    hausdorff: float
    hd95: float
    assd: float

    def to_dict(self) -> dict:
        """JSON-ready: nan written as None."""
        return {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in asdict(self).items()}


def nearest_rank(n: int, percent: int = 95) -> int:
    """The 1-based rank of the `percent`-th percentile of n values by nearest rank: ceil(percent * n / 100), in integers."""
    return (percent * int(n) + 99) // 100


def surface_figures(a_d2, b_d2, downscale: int = 1) -> SurfaceDistance:
    """The figures of two directed sets of squared distances (integer arrays, any order): each sorted as integers, then in
    float64 hausdorff = sqrt(largest of both), hd95 = the larger of the two sqrt(value of rank ceil(0.95 n)), assd =
    (sum(sqrt(a)) + sum(sqrt(b))) / (|a| + |b|), each times `downscale`; the sums are `np.sum` over the sorted values."""
    a = np.sort(np.asarray(a_d2, np.int64).ravel())
    b = np.sort(np.asarray(b_d2, np.int64).ravel())
    if a.size == 0 or b.size == 0:
        return SurfaceDistance(int(a.size), int(b.size), math.nan, math.nan, math.nan)
    ra, rb = np.sqrt(a.astype(np.float64)), np.sqrt(b.astype(np.float64))
    d = float(downscale)
    return SurfaceDistance(int(a.size), int(b.size), float(max(ra[-1], rb[-1])) * d,
                           float(max(ra[nearest_rank(a.size) - 1], rb[nearest_rank(b.size) - 1])) * d,
                           float((ra.sum() + rb.sum()) / (a.size + b.size)) * d)


def surface_distances(pred, truth, cls: int, downscale: int = 1, device="cuda") -> SurfaceDistance:
    """Hausdorff, HD95 and average symmetric surface distance of class `cls` between a predicted and an annotated map.

    A is the boundary ("boundary" mode of `class_mask`) of the class in `pred`, B in `truth`; the directed sets are d(a, B)
    for a in A and d(b, A) for b in B, read off two distance transforms at the boundary cells, downloaded and handed to
    `surface_figures`.  The figures mean something only for a class the annotation covers completely: where the annotation
    leaves tissue of the class unlabelled, its boundary is the annotator's, not the tissue's."""
    pred, truth = _as_map(pred, device), _as_map(truth, device)
    if pred.shape != truth.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and truth {tuple(truth.shape)} must match")
    a = class_mask(pred, [cls], mode="boundary").bool()
    b = class_mask(truth, [cls], mode="boundary").bool()
    if not bool(a.any()) or not bool(b.any()):
        return SurfaceDistance(int(a.sum()), int(b.sum()), math.nan, math.nan, math.nan)
    return surface_figures(distance_transform(b)[a].cpu().numpy(), distance_transform(a)[b].cpu().numpy(), downscale)


def tolerant_truth(truth, tolerance_px: int, downscale: int, device="cuda") -> torch.Tensor:
    """A copy of the int32 label map `truth` with -1 in every cell whose squared distance d2 to the nearest label-change cell
    ("change" mode of `class_mask`) has d2 * downscale^2 < tolerance_px^2, compared in int64."""
    tol, d = int(tolerance_px), int(downscale)
    if tol != tolerance_px or tol < 0 or not 1 <= d <= 32768:
        raise ValueError(f"tolerance_px = {tolerance_px} must be an integer >= 0 and downscale = {downscale} in 1 .. 32768")
    truth = _as_map(truth, device)
    d2 = distance_transform(class_mask(truth, [], mode="change"))
    out = truth.to(torch.int32)
    out[d2.to(torch.int64) * (d * d) < tol * tol] = -1
    return out


def tolerant_score(pred, truth, labels, tolerance_px: int, downscale: int, device="cuda") -> scoring.SlideScore:
    """`scoring.SlideScore` of `scoring.confusion` against `tolerant_truth(truth, tolerance_px, downscale)`: the cells within
    the tolerance of a label change of the annotation are left out.  `tolerance_px` = 0 is the plain confusion matrix;
    at downscale 1, 1 drops exactly the label-change cells.  `n_cells` stays the canvas size."""
    pred = _as_map(pred, device)
    counts = scoring.confusion(pred, tolerant_truth(truth, tolerance_px, downscale, pred.device), len(labels))
    return scoring.SlideScore(counts, labels, pred.numel())


def save_distance_report(path, downscale: int, margin: dict | None = None, tolerant: dict | None = None,
                         surface: dict | None = None) -> Path:
    """Writes the one JSON of the distance steps: {"downscale", "margin": {"label", "edges_px", "class_labels", "counts"},
    "tolerant": {"tolerance_px", "score"}, "surface": {label: SurfaceDistance.to_dict()}}; a step that did not run is None.
    `counts` is `band_composition` as lists, `score` a `SlideScore.to_dict()`; SlideScore and SurfaceDistance values are
    converted here."""
    def plain(v):
        if isinstance(v, (scoring.SlideScore, SurfaceDistance)):
            return v.to_dict()
        if isinstance(v, (torch.Tensor, np.ndarray)):
            return v.tolist()
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        return v
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_text(json.dumps(dict(downscale=int(downscale), margin=plain(margin), tolerant=plain(tolerant), surface=plain(surface)),
                               indent=1) + "\n")
    return path
