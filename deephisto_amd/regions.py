"""Regions of a whole-slide class map: connected components, region table, cleanup, polygons.

`label_components` numbers the 4-connected components of equal class (`dh_label_components`), `region_table` collects their
integer figures (`dh_region_stats`) into a `SlideRegions`, `clean_map` gives components below a size the class of their large
neighbours (`dh_clean_small_regions`), `trace_polygons` turns regions of a downloaded label map into rings (NumPy, on the
host: usable without a GPU), `export_annotation` writes them as the annotation JSON the samplers and `scoring` read, and
`extract_regions` runs all of it in one call.  torch is used for device memory and streams only; the device parts have no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .patch_samplers import polygon

MAX_CLASSES = 64   # MAX_CLS of csrc/regions.hip
TABLE_COLUMNS = ("class", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x", "first", "conf_q")


def _as_map(pred, device="cuda") -> torch.Tensor:
    if isinstance(pred, tiles.SlideProbabilities):
        if not pred.finished:
            raise ValueError("the SlideProbabilities is unfinished: it has no class map yet")
        pred = pred.class_map
    if not isinstance(pred, torch.Tensor):
        pred = torch.from_numpy(np.ascontiguousarray(pred))
    if pred.dim() != 2 or pred.numel() == 0:
        raise ValueError(f"a class map is a non-empty [dh, dw] array, not {list(pred.shape)}")
    if not pred.is_cuda:
        pred = pred.to(device)
    return pred.to(torch.int64).contiguous()


def _check_classes(n_classes: int) -> int:
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f"n_classes = {n_classes}: the region kernels take 1 to {MAX_CLASSES} classes")
    return int(n_classes)


def label_components(pred, n_classes: int = MAX_CLASSES):
    """(int32[dh, dw] label map on the device, K) of an int64 class map with values in [-1, n_classes): 0 where the class is
    -1, else the id in 1..K of the cell's 4-connected component of equal class; ids ascend with the component's smallest
    linear cell index, so the numbering is unique.  A class outside the range raises (DH_EINVAL)."""
    n_cls = _check_classes(n_classes)
    pred = _as_map(pred)
    dh, dw = pred.shape
    labels = torch.empty((dh, dw), dtype=torch.int32, device=pred.device)
    k = C.c_int64(0)
    with torch.cuda.device(pred.device):
        work = torch.empty(int(lib().dh_label_work_size(dh * dw)), dtype=torch.int32, device=pred.device)
        check(lib().dh_label_components(pred.data_ptr(), dh, dw, n_cls, labels.data_ptr(), work.data_ptr(),
                                        C.byref(k), tiles._stream(pred.device)), "dh_label_components")
    return labels, int(k.value)


class SlideRegions:
    """The region table of one label map as NumPy columns, row i for id i + 1: `cls` int32, `area` int64 (cells), the
    half-open bounding box `y0, x0, y1, x1` (cells), `sum_y, sum_x` int64, `first` (the smallest linear cell index) and, when a
    confidence map was given, `conf_q` uint64 (else None).  `centroid` (float64[K, 2], (y, x) in cell units:
    (sum + area / 2) / area, the mean of the cell centres) and `mean_confidence` (conf_q / area / 2^32) are derived on the
    host in float64.  `shape` is the canvas (dh, dw)."""

    def __init__(self, table, shape, has_confidence: bool):
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, len(TABLE_COLUMNS))
        self.shape = (int(shape[0]), int(shape[1]))
        self.cls = t[:, 0].astype(np.int32)
        self.area, self.y0, self.x0, self.y1, self.x1, self.sum_y, self.sum_x, self.first = (t[:, c].copy() for c in range(1, 9))
        self.conf_q = t[:, 9].copy().view(np.uint64) if has_confidence else None

    def __len__(self) -> int:
        return int(self.cls.shape[0])

    @property
    def centroid(self) -> np.ndarray:
        a = self.area.astype(np.float64)
        return np.stack([(self.sum_y + a / 2) / a, (self.sum_x + a / 2) / a], axis=1)

    @property
    def mean_confidence(self):
        return None if self.conf_q is None else self.conf_q.astype(np.float64) / self.area.astype(np.float64) / 2.0 ** 32

    def to_records(self, anno_dsc, downscale: int, layer: int) -> list[dict]:
        """JSON-ready rows: id, class label, area in cells and in layer pixels, bounding box and centroid in layer pixels
        ((y, x), cell units times `downscale`), the same in layer-1 coordinates (times `layer`), mean confidence or None."""
        by_id = {a.id: a.label for a in anno_dsc.anno_classes}
        d, cen, conf = int(downscale), self.centroid * float(downscale), self.mean_confidence
        return [dict(id=i + 1, **{"class": by_id.get(int(self.cls[i]), str(int(self.cls[i])))}, area_cells=int(self.area[i]),
                     area_px=int(self.area[i]) * d * d,
                     bbox_px=[int(self.y0[i]) * d, int(self.x0[i]) * d, int(self.y1[i]) * d, int(self.x1[i]) * d],
                     centroid_px=[float(cen[i, 0]), float(cen[i, 1])],
                     centroid_layer1=[float(cen[i, 0]) * layer, float(cen[i, 1]) * layer],
                     confidence=None if conf is None else float(conf[i])) for i in range(len(self))]

    def __str__(self) -> str:
        conf = self.mean_confidence
        lines = [f"{'id':>8} {'class':>5} {'area':>10} {'y0':>6} {'x0':>6} {'y1':>6} {'x1':>6} {'cy':>9} {'cx':>9} {'conf':>7}"]
        cen = self.centroid
        for i in np.lexsort((np.arange(len(self)), -self.area)):   # by area, largest first; ties by id
            c = "-" if conf is None else f"{conf[i]:.4f}"
            lines.append(f"{i + 1:>8d} {int(self.cls[i]):>5d} {int(self.area[i]):>10d} {int(self.y0[i]):>6d} {int(self.x0[i]):>6d} "
                         f"{int(self.y1[i]):>6d} {int(self.x1[i]):>6d} {cen[i, 0]:>9.2f} {cen[i, 1]:>9.2f} {c:>7}")
        lines.append(f"{len(self)} regions, {int(self.area.sum())} cells of {self.shape[0]} x {self.shape[1]}")
        return "\n".join(lines)


def _table_dev(pred, labels, k, confidence=None) -> torch.Tensor:
    tiles._require_cuda(labels, "labels")
    if labels.dtype != torch.int32 or labels.shape != pred.shape or labels.device != pred.device:
        raise ValueError(f"labels must be int32{list(pred.shape)} on {pred.device}, not {labels.dtype}{list(labels.shape)} on {labels.device}")
    if not 0 <= int(k) <= pred.numel():
        raise ValueError(f"K = {k} outside [0, {pred.numel()}]")
    if confidence is not None:
        tiles._require_cuda(confidence, "confidence")
        if confidence.dtype != torch.float32 or confidence.shape != pred.shape or confidence.device != pred.device:
            raise ValueError(f"confidence must be float32{list(pred.shape)} on {pred.device}, not "
                             f"{confidence.dtype}{list(confidence.shape)} on {confidence.device}")
    table = torch.empty((int(k), len(TABLE_COLUMNS)), dtype=torch.int64, device=pred.device)
    with torch.cuda.device(pred.device):
        check(lib().dh_region_stats(pred.data_ptr(), labels.data_ptr(), confidence.data_ptr() if confidence is not None else None,
                                    pred.shape[0], pred.shape[1], int(k), table.data_ptr(), tiles._stream(pred.device)),
              "dh_region_stats")
    return table


def region_table(pred, labels: torch.Tensor, k: int, confidence: torch.Tensor | None = None) -> SlideRegions:
    """SlideRegions of a class map and its label map (`dh_region_stats`); `confidence`: a float32[dh, dw] device map
    (`SlideProbabilities.confidence`) whose quantised sum per region becomes `conf_q`."""
    pred = _as_map(pred)
    return SlideRegions(_table_dev(pred, labels, k, confidence).cpu().numpy(), pred.shape, confidence is not None)


def clean_map(pred, min_cells: int, rounds: int = 1, n_classes: int | None = None):
    """(cleaned int64 map on the device, number of cells that changed).  Per round: label the map; every component with
    area < `min_cells` takes the class that most of its (cell, 4-neighbour in a component that is not small) pairs vote for,
    the lowest class id on a tie, and stays without a vote; all small components are decided from the one labelling and
    rewritten at once (`dh_clean_small_regions`).  Cells of class -1 neither vote nor change.  Rounds end early when nothing
    changed.  The input is not modified.  `n_classes`: the width of the vote table (default: the map's largest class + 1)."""
    if int(min_cells) < 1 or int(rounds) < 1:
        raise ValueError(f"min_cells = {min_cells} and rounds = {rounds} must be >= 1")
    pred = _as_map(pred)
    if n_classes is None:
        n_classes = max(1, int(pred.max().item()) + 1)
    n_cls = _check_classes(n_classes)
    cur, total = pred, 0
    dh, dw = pred.shape
    for _ in range(int(rounds) if min_cells > 1 else 0):
        labels, k = label_components(cur, n_cls)
        table = _table_dev(cur, labels, k)
        votes = torch.empty((max(k, 1), n_cls), dtype=torch.int32, device=pred.device)
        out = torch.empty_like(cur)
        changed = C.c_int64(0)
        with torch.cuda.device(pred.device):
            check(lib().dh_clean_small_regions(cur.data_ptr(), labels.data_ptr(), table.data_ptr(), k, dh, dw, n_cls, int(min_cells),
                                               votes.data_ptr(), out.data_ptr(), C.byref(changed), tiles._stream(pred.device)),
                  "dh_clean_small_regions")
        if changed.value == 0:
            break
        cur, total = out, total + int(changed.value)
    return (cur.clone() if cur is pred else cur), total


def trace_polygons(labels_np, ids, downscale: int, layer: int) -> dict:
    """{id: (outer ring, [hole rings])} of the regions `ids` of a label map (NumPy, host).

    A region's boundary is the set of unit edges between one of its cells and a cell outside it (or outside the canvas).
    The edges are chained into closed rings of cell corners, walked with the region on one side; at a corner where four
    boundary edges meet the walk turns round the cell it came along, so rings may touch at a vertex but never cross: one
    outer ring per region and one ring per hole (a hole being a set of outside cells joined by edges or corners).  Collinear
    runs are merged to their end points.  A corner is (cx * d, cy * d) at the layer's scale and is written as
    (x, y) * layer, the layer-1 coordinates the annotation JSON stores; every ring is float64[n, 2] and counter-clockwise
    by `polygon.as_ccw`.  The cell centres ((cx + .5) d, (cy + .5) d) never lie on an edge."""
    lab = np.asarray(labels_np)
    if lab.ndim != 2 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"a label map is an integer [dh, dw] array, not {lab.dtype}{list(lab.shape)}")
    ids = [int(i) for i in ids]
    out = {i: [None, []] for i in ids}
    if not ids or lab.size == 0:
        return {i: (None, []) for i in ids}
    if min(ids) < 1:
        raise ValueError("region ids start at 1")
    pad = np.pad(lab.astype(np.int64), 1)            # 0 round the canvas: outside every region
    W = pad.shape[1]
    flat = pad.ravel()
    want = np.zeros(max(int(flat.max()), max(ids)) + 1, bool)
    want[ids] = True
    cells = np.flatnonzero(want[flat] & (flat > 0))
    # edge (d, c): side d of cell c, walked so that the cell is on the right.  d: 0 top (towards +x), 1 right (+y), 2 bottom
    # (-x), 3 left (-y).  out_[d]: the neighbour across the side; fwd[d]: the next cell in walking direction.
    out_ = np.array([-W, 1, W, -1])
    fwd = np.array([1, W, -1, -W])
    mine = flat[cells]
    keys, succ = [], []
    for d in range(4):
        c = cells[flat[cells + out_[d]] != mine]
        m = flat[c]
        ahead, diag = c + fwd[d], c + fwd[d] + out_[d]
        right = flat[ahead] != m                     # nothing ahead: turn right, round this cell (also at a pinch)
        straight = ~right & (flat[diag] != m)
        keys.append(c * 4 + d)
        succ.append(np.where(right, c * 4 + (d + 1) % 4, np.where(straight, ahead * 4 + d, diag * 4 + (d + 3) % 4)))
    keys, succ = np.concatenate(keys), np.concatenate(succ)
    order = np.argsort(keys, kind="stable")
    keys, succ = keys[order], succ[order]
    nxt = np.searchsorted(keys, succ)
    assert np.array_equal(keys[nxt], succ), "boundary edges do not chain"
    turn = (keys & 3) != (keys[nxt] & 3)             # the edge's end corner is a vertex
    while True:                                      # nxt -> the next edge that ends in a vertex (pointer doubling)
        stray = np.flatnonzero(~turn[nxt])
        if stray.size == 0:
            break
        nxt[stray] = nxt[nxt[stray]]
    c, d = keys >> 2, keys & 3
    cy, cx = c // W - 1, c % W - 1                   # canvas coordinates of the cell
    vx = cx + np.isin(d, (0, 1))                     # end corner: top -> (x+1, y), right -> (x+1, y+1), bottom -> (x, y+1), left -> (x, y)
    vy = cy + np.isin(d, (1, 2))
    scale = float(downscale) * float(layer)
    owner = flat[c]
    starts = np.flatnonzero(turn)
    seen = np.zeros(len(keys), bool)
    nxt_l = nxt.tolist()
    for e in starts.tolist():
        if seen[e]:
            continue
        ring = []
        while not seen[e]:
            seen[e] = True
            ring.append(e)
            e = nxt_l[e]
        ring = np.asarray(ring)
        v = np.stack([vx[ring], vy[ring]], axis=1).astype(np.float64) * scale
        slot = out[int(owner[ring[0]])]
        if polygon.signed_area(v) > 0:               # the region on the right of a walk towards +x along its top: positive
            assert slot[0] is None, "two outer rings for one region"
            slot[0] = polygon.as_ccw(v)
        else:
            slot[1].append(polygon.as_ccw(v))
    return {i: (o, h) for i, (o, h) in out.items()}


def export_annotation(path, regions: SlideRegions, polygons: dict, anno_dsc) -> Path:
    """Writes the regions of `polygons` ({id: (outer, holes)} from `trace_polygons`) as a JSON list of
    {"class": label, "vertices": outer ring, "holes": [rings...], "area_px": ..., "confidence": ...}; vertices are (x, y) in
    layer-1 coordinates, `area_px` the area the rings enclose in those coordinates (outer minus holes), `confidence` the
    region's mean confidence or None.  The reference's loader reads `class` and `vertices` and ignores the other keys: its
    annotation format cannot express a hole, so a region read back through `RegionAnnotation` is its outer ring, holes
    filled.  A ring that touches itself at a vertex (a diagonal pinch) is split by `polygon.repair` when read back."""
    by_id = {a.id: a.label for a in anno_dsc.anno_classes}
    conf = regions.mean_confidence
    records = []
    for i in sorted(polygons):
        outer, holes = polygons[i]
        if outer is None:
            continue
        records.append({"class": by_id[int(regions.cls[i - 1])], "vertices": outer.tolist(), "holes": [h.tolist() for h in holes],
                        "area_px": polygon.area(outer) - sum(polygon.area(h) for h in holes),
                        "confidence": None if conf is None else float(conf[i - 1])})
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_text(json.dumps(records))
    return path


@dataclass
class RegionResult:
    """What `extract_regions` returns: the (cleaned) class map and its label map on the device, K, the table, the number of
    cells the cleanup changed, {id: (outer, holes)} (None without `polygons`) and the host tracing wall time in seconds."""
    class_map: torch.Tensor
    labels: torch.Tensor
    k: int
    regions: SlideRegions
    n_changed: int
    polygons: dict | None
    trace_s: float

    def records(self, anno_dsc, downscale: int, layer: int) -> list[dict]:
        return self.regions.to_records(anno_dsc, downscale, layer)


def extract_regions(pred, anno_dsc, layer: int, downscale: int, min_cells: int = 0, rounds: int = 1, polygons: bool = True,
                    device="cuda", confidence: torch.Tensor | None = None) -> RegionResult:
    """The one-call form: optional cleanup (`min_cells` > 1), labelling, table, polygons of every region.

    `pred`: an int64[dh, dw] class map (device tensor, or a NumPy array, uploaded to `device`) or a `tiles.SlideProbabilities`,
    whose `class_map` is taken and whose `confidence` gives the table's mean confidence (of the cells' own predictions, also
    after a cleanup changed their class); `confidence`: that map for a `pred` given as a plain class map.  Classes are the ids
    of `anno_dsc`."""
    if confidence is None and isinstance(pred, tiles.SlideProbabilities) and pred.finished:
        confidence = pred.confidence
    cmap = _as_map(pred, device)
    n_cls = _check_classes(max((a.id for a in anno_dsc.anno_classes), default=-1) + 1)
    n_changed = 0
    if min_cells > 1:
        cmap, n_changed = clean_map(cmap, min_cells, rounds, n_cls)
    labels, k = label_components(cmap, n_cls)
    regions = region_table(cmap, labels, k, confidence)
    polys, t0 = None, time.perf_counter()
    if polygons:
        polys = trace_polygons(labels.cpu().numpy(), range(1, k + 1), downscale, layer)
    return RegionResult(cmap, labels, k, regions, n_changed, polys, time.perf_counter() - t0 if polygons else 0.0)


def save_regions(path, regions: SlideRegions, anno_dsc, downscale: int, layer: int, extra: dict | None = None) -> Path:
    """Writes `regions.to_records(...)` (plus `extra` entries) as JSON: {"shape", "n_regions", "regions": [...]}."""
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    path.write_text(json.dumps(dict(shape=list(regions.shape), n_regions=len(regions), downscale=int(downscale), layer=int(layer),
                                    **(extra or {}), regions=regions.to_records(anno_dsc, downscale, layer)), indent=1))
    return path
