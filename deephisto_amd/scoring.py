"""Scoring a whole-slide class map against the slide's polygon annotation.

`rasterize_annotation` turns the annotation into an int32 label map on the prediction's canvas (`dh_rasterize_regions`),
`confusion` counts truth against prediction (`dh_confusion_matrix`), `SlideScore` derives the usual per-class and overall
figures from the integer matrix in float64 on the host, and `score_prediction` runs the three in one call.  torch is used
for device memory and streams only; there is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import io
import json
import math
from pathlib import Path

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .patch_samplers.region_samplers import RegionAnnotation, _load_annotation, _parse_annotations

MAX_CLASSES = 64   # MAX_CLS of csrc/accumulate.hip and csrc/score.hip


class _LayerSize:
    """The part of a PSImage-like reader that `_parse_annotations` asks for: the layer's size."""

    def __init__(self, h: int, w: int):
        self._size = (int(h), int(w))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def layer_size(self, layer):
        return self._size

    def get_region_from_layer(self, layer, p0, p1):
        raise RuntimeError("no pixels behind an annotation's layer size")


def _n_ids(anno_dsc) -> int:
    return max((a.id for a in anno_dsc.anno_classes), default=-1) + 1


def annotation_rings(anno, anno_dsc, layer: int, h: int, w: int):
    """(float64[n_vertices, 2] (x, y), int64[n_rings + 1] ring offsets, int32[n_rings] class ids, info) of an annotation.

    `anno`: a path to the JSON, the loaded list of `{"class", "vertices"}` records, or a list of RegionAnnotation (taken at
    the layer they were built for).  Records go through `_parse_annotations(..., layer, classes=<labels of anno_dsc>)`, so the
    rings are the samplers': counter-clockwise at the layer's scale, a repaired region contributing every ring it was split
    into.  `info`: n_rings, n_regions, skipped_class (regions whose class the description does not know) and failed (regions
    that did not parse)."""
    known = anno_dsc.anno_classes_dict
    if isinstance(anno, (list, tuple)) and anno and all(isinstance(a, RegionAnnotation) for a in anno):
        regions = [a for a in anno if a.class_ in known]
        skipped, failed = len(anno) - len(regions), 0
    else:
        records = _load_annotation(anno)
        n_known = sum(1 for a in records if a["class"] in known)
        skipped = len(records) - n_known
        with contextlib.redirect_stdout(io.StringIO()):   # the parser's progress lines
            by_class, _ = _parse_annotations([(_LayerSize(h, w), records)], layer, classes=list(known))
        regions = sorted((r for regs in by_class.values() for r in regs), key=lambda r: r.region_idx)
        failed = n_known - len(regions)
    rings, classes = [], []
    for reg in regions:
        for ring in (reg.polygon if isinstance(reg.polygon, list) else [reg.polygon]):
            rings.append(np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 2))
            classes.append(known[reg.class_].id)
    start = np.zeros(len(rings) + 1, np.int64)
    if rings:
        start[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings) if rings else np.zeros((0, 2), np.float64)
    info = dict(n_rings=len(rings), n_regions=len(regions), skipped_class=int(skipped), failed=int(failed))
    return np.ascontiguousarray(xy), start, np.asarray(classes, np.int32), info


def rasterize_rings(xy, ring_start, ring_class, n_classes: int, dh: int, dw: int, downscale: int, device="cuda") -> torch.Tensor:
    """int32[dh, dw] label map of the rings on the device (`dh_rasterize_regions`): the class id of the rings that hold the
    cell's centre ((cx + 0.5) * d, (cy + 0.5) * d) when they are of one class, else -1."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the label map is built in GPU memory (got device {dev})")
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    ring_start = np.ascontiguousarray(ring_start, dtype=np.int64)
    ring_class = np.ascontiguousarray(ring_class, dtype=np.int32)
    n = int(ring_class.shape[0])
    if ring_start.shape != (n + 1,) or (n and int(ring_start[-1]) != xy.shape[0]):
        raise ValueError(f"{n} rings need {n + 1} offsets that end at the {xy.shape[0]} vertices")
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes = {n_classes}: the scoring kernels take 1 to {MAX_CLASSES} classes")
    if dh <= 0 or dw <= 0:
        raise ValueError(f"the canvas of {dh} x {dw} cells is empty")
    out = torch.empty((dh, dw), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().dh_rasterize_regions(xy.ctypes.data_as(C.c_void_p) if n else None,
                                         ring_start.ctypes.data_as(C.c_void_p) if n else None,
                                         ring_class.ctypes.data_as(C.c_void_p) if n else None, n, int(n_classes), dh, dw,
                                         int(downscale), out.data_ptr(), tiles._stream(dev)), "dh_rasterize_regions")
    return out


def rasterize_annotation(anno, anno_dsc, layer: int, h: int, w: int, downscale: int, device="cuda"):
    """(int32[h // d, w // d] label map on the device, info) of an annotation for a layer of h x w pixels: the canvas of
    `ImagePredictorPatched.process()` / `predict_full_patched`.  See `annotation_rings` for `anno` and `info`."""
    n_cls = _n_ids(anno_dsc)
    if not 1 <= n_cls <= MAX_CLASSES:
        raise ValueError(f"the description has class ids up to {n_cls - 1}: the scoring kernels take 1 to {MAX_CLASSES} classes")
    xy, start, cls, info = annotation_rings(anno, anno_dsc, layer, h, w)
    return rasterize_rings(xy, start, cls, n_cls, h // downscale, w // downscale, downscale, device), info


def confusion(pred: torch.Tensor, truth: torch.Tensor, n_classes: int, return_outcome: bool = False):
    """int64[n, n + 1] confusion matrix (a host tensor; rows truth, columns prediction, the last column: labelled cells whose
    prediction is -1) of an int64 class map against an int32 label map of the same shape, both on the device
    (`dh_confusion_matrix`).  Cells whose truth is -1 are not counted.  `return_outcome`: also the int64 map of -1
    (unlabelled) / 0 (correct) / 1 (wrong) on the device."""
    tiles._require_cuda(pred, "pred")
    tiles._require_cuda(truth, "truth")
    if pred.dtype != torch.int64 or truth.dtype != torch.int32:
        raise ValueError(f"pred must be int64 and truth int32, not {pred.dtype} and {truth.dtype}")
    if pred.shape != truth.shape or pred.device != truth.device:
        raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} and truth {tuple(truth.shape)} on {truth.device} must match")
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes = {n_classes}: the scoring kernels take 1 to {MAX_CLASSES} classes")
    counts = np.zeros((n_classes, n_classes + 1), np.int64)
    outcome = torch.empty(tuple(pred.shape), dtype=torch.int64, device=pred.device) if return_outcome else None
    with torch.cuda.device(pred.device):
        check(lib().dh_confusion_matrix(pred.data_ptr(), truth.data_ptr(), pred.numel(), int(n_classes),
                                        counts.ctypes.data_as(C.c_void_p), outcome.data_ptr() if return_outcome else None,
                                        tiles._stream(pred.device)), "dh_confusion_matrix")
    counts = torch.from_numpy(counts)
    return (counts, outcome) if return_outcome else counts


def _ratio(num, den):
    return float(num) / float(den) if den else math.nan


class SlideScore:
    """Quality figures of one class map (or, added up, of a test set) from its confusion matrix int64[n, n + 1].

    `support` are the row sums; `n_labelled` their total; `n_unclassified` the labelled cells without a prediction (the last
    column); `n_unlabelled` the cells the annotation leaves out (`n_cells` - `n_labelled`; None when `n_cells` is unknown).
    Per class k, with tp = C[k, k], predicted = the sum of column k: precision tp / predicted, recall tp / support,
    iou tp / (support + predicted - tp), dice 2 tp / (support + predicted); a zero denominator gives nan.  `accuracy` is the
    trace over `n_labelled`; `mean_iou` and `mean_dice` average the classes with support.  All in float64 from the integers."""

    def __init__(self, confusion, labels, n_cells: int | None = None):
        c = confusion.cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
        if c.ndim != 2 or c.shape[1] != c.shape[0] + 1 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"a confusion matrix is an integer [n, n + 1] array, not {c.dtype}{list(c.shape)}")
        self.confusion = c.astype(np.int64)
        self.labels = [str(lb) for lb in labels]
        if len(self.labels) != c.shape[0]:
            raise ValueError(f"{len(self.labels)} labels for {c.shape[0]} classes")
        self.n_cells = None if n_cells is None else int(n_cells)
        n = c.shape[0]
        self.support = self.confusion.sum(axis=1)
        self.predicted = self.confusion[:, :n].sum(axis=0)
        self.n_labelled = int(self.support.sum())
        self.n_unclassified = int(self.confusion[:, n].sum())
        self.n_unlabelled = None if self.n_cells is None else self.n_cells - self.n_labelled
        tp = np.diagonal(self.confusion[:, :n])
        self.precision = np.array([_ratio(tp[k], self.predicted[k]) for k in range(n)], np.float64)
        self.recall = np.array([_ratio(tp[k], self.support[k]) for k in range(n)], np.float64)
        self.iou = np.array([_ratio(tp[k], self.support[k] + self.predicted[k] - tp[k]) for k in range(n)], np.float64)
        self.dice = np.array([_ratio(2 * tp[k], self.support[k] + self.predicted[k]) for k in range(n)], np.float64)
        self.accuracy = _ratio(tp.sum(), self.n_labelled)
        seen = self.support > 0
        self.mean_iou = float(np.mean(self.iou[seen])) if seen.any() else math.nan
        self.mean_dice = float(np.mean(self.dice[seen])) if seen.any() else math.nan

    def __add__(self, other: "SlideScore") -> "SlideScore":
        if not isinstance(other, SlideScore):
            return NotImplemented
        if other.labels != self.labels:
            raise ValueError(f"scores of different class lists: {self.labels} and {other.labels}")
        n_cells = None if self.n_cells is None or other.n_cells is None else self.n_cells + other.n_cells
        return SlideScore(self.confusion + other.confusion, self.labels, n_cells)

    def to_dict(self) -> dict:
        """JSON-ready: integers, and floats with nan written as None."""
        def f(v):
            return None if math.isnan(v) else float(v)
        return dict(labels=list(self.labels), confusion=self.confusion.tolist(), n_cells=self.n_cells,
                    support=self.support.tolist(), n_labelled=self.n_labelled, n_unlabelled=self.n_unlabelled,
                    n_unclassified=self.n_unclassified, accuracy=f(self.accuracy), mean_iou=f(self.mean_iou),
                    mean_dice=f(self.mean_dice),
                    per_class={lb: dict(support=int(self.support[k]), precision=f(self.precision[k]), recall=f(self.recall[k]),
                                        iou=f(self.iou[k]), dice=f(self.dice[k])) for k, lb in enumerate(self.labels)})

    @classmethod
    def from_dict(cls, d: dict) -> "SlideScore":
        return cls(np.asarray(d["confusion"], np.int64).reshape(len(d["labels"]), len(d["labels"]) + 1), d["labels"], d.get("n_cells"))

    def __str__(self) -> str:
        wd = max([5] + [len(lb) for lb in self.labels])
        lines = [f"{'class':<{wd}} {'support':>10} {'precision':>9} {'recall':>9} {'iou':>9} {'dice':>9}"]
        for k, lb in enumerate(self.labels):
            lines.append(f"{lb:<{wd}} {int(self.support[k]):>10d} {self.precision[k]:>9.4f} {self.recall[k]:>9.4f} "
                         f"{self.iou[k]:>9.4f} {self.dice[k]:>9.4f}")
        unl = "?" if self.n_unlabelled is None else str(self.n_unlabelled)
        lines.append(f"accuracy {self.accuracy:.4f}  mean iou {self.mean_iou:.4f}  mean dice {self.mean_dice:.4f}  "
                     f"labelled {self.n_labelled}  unlabelled {unl}  unclassified {self.n_unclassified}")
        return "\n".join(lines)


def score_prediction(pred, anno, anno_dsc, layer: int, h: int, w: int, downscale: int, return_maps: bool = False,
                     device="cuda"):
    """SlideScore of a class map against an annotation: label map, confusion matrix, figures.

    `pred`: the int64[h // d, w // d] class map of `predict_full_patched` / `predict_random_patched` (a device tensor) or of
    `ImagePredictorPatched.process()` (a NumPy array, uploaded), or a `tiles.SlideProbabilities`, whose `class_map` is scored.
    `return_maps`: also (truth int32, outcome int64) on the device and the rasteriser's `info`.  `device`: where a map that is
    not in GPU memory yet is uploaded to."""
    if isinstance(pred, tiles.SlideProbabilities):
        if not pred.finished:
            raise ValueError("the SlideProbabilities is unfinished: it has no class map yet")
        pred = pred.class_map
    if not isinstance(pred, torch.Tensor):
        pred = torch.from_numpy(np.ascontiguousarray(pred))
    if not pred.is_cuda:
        pred = pred.to(device)
    pred = pred.to(torch.int64).contiguous()
    if tuple(pred.shape) != (h // downscale, w // downscale):
        raise ValueError(f"the class map is {tuple(pred.shape)}, the canvas of {h} x {w} at downscale {downscale} is "
                         f"{(h // downscale, w // downscale)}")
    truth, info = rasterize_annotation(anno, anno_dsc, layer, h, w, downscale, pred.device)
    labels = [""] * _n_ids(anno_dsc)
    for a in anno_dsc.anno_classes:
        labels[a.id] = a.label
    counts, outcome = confusion(pred, truth, len(labels), return_outcome=True)
    score = SlideScore(counts, labels, pred.numel())
    return (score, truth, outcome, info) if return_maps else score


def save_score(path, score: SlideScore, info: dict | None = None) -> Path:
    """Writes `score.to_dict()` (plus the rasteriser's `info` counts) as JSON."""
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_text(json.dumps(dict(score.to_dict(), **({"annotation": info} if info is not None else {})), indent=1))
    return path


def synthetic_annotation(h: int, w: int, n_regions: int, n_vertices: int, labels, seed: int = 0, layer: int = 1) -> list[dict]:
    """A seeded closed-form annotation for slides without one (tests, tools, `--synthetic` runs): `n_regions` wavy rings of
    `n_vertices` vertices, r(t) = R * (1 + 0.25 * sin(k * t + phase)), centres anywhere on the h x w layer (so some rings hang
    over the border), R between 2 % and 12 % of the shorter side, classes drawn from `labels`.  Returns the JSON's list of
    `{"class", "vertices"}` records, vertices (x, y) in layer-1 coordinates (times `layer`)."""
    rng = np.random.default_rng(seed)
    labels = list(labels)
    t = np.arange(n_vertices, dtype=np.float64) * (2.0 * np.pi / n_vertices)
    out = []
    for _ in range(n_regions):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        rad = rng.uniform(0.02, 0.12) * min(h, w)
        k, phase = int(rng.integers(2, 9)), rng.uniform(0, 2 * np.pi)
        r = rad * (1.0 + 0.25 * np.sin(k * t + phase))
        v = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1) * float(layer)
        out.append({"class": labels[int(rng.integers(0, len(labels)))], "vertices": v.tolist()})
    return out
