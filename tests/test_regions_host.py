"""Regions of a class map, the host side: the NumPy restatement `regions_np` (labels, table, votes,
cleanup) that tests/test_gpu_regions.py holds the device to, pinned per class to scipy.ndimage.label; `trace_polygons`
(NumPy, no GPU) against an even-odd fill at the section 4.9 cell centres; export and reload through the annotation parser;
header / signature entries, formatting, CLI flag errors.  Everything here is integer-exact: no tolerance anywhere."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
LABELS = ["AT", "BG", "LP", "MM", "TUM"]


# ---- the restatement -----------------------------------------------------------------------------------------------------
def label_np(m):
    """(int32 label map, K) by the rule of section 4.10.  Row runs of one class are the nodes; runs of adjacent rows that
    overlap with the same class are joined by iterated minimum propagation over those pairs (hook the larger root below the
    smaller, then shorten every chain) until no pair joins two roots.  A root is its set's first run in raster order, so
    numbering the roots in order numbers the components by their smallest linear cell index."""
    m = np.asarray(m, np.int64)
    dh, dw = m.shape
    flat = m.ravel()
    n = flat.size
    fg = flat >= 0
    same_left = np.zeros(n, bool)
    same_left[1:] = flat[1:] == flat[:-1]
    same_left[::dw] = False
    start = fg & ~same_left
    run_of = np.cumsum(start) - 1
    n_runs = int(start.sum())
    i = np.flatnonzero(fg[dw:] & (flat[dw:] == flat[:-dw])) + dw
    a, b = run_of[i], run_of[i - dw]
    if len(i):
        keep = np.ones(len(i), bool)
        keep[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
        a, b = a[keep], b[keep]
    p = np.arange(n_runs)
    while len(a):
        ra, rb = p[a], p[b]
        live = ra != rb
        if not live.any():
            break
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        np.minimum.at(p, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    roots = np.flatnonzero(p == np.arange(n_runs))
    rank = np.zeros(n_runs + 1, np.int32)
    rank[roots] = np.arange(1, len(roots) + 1, dtype=np.int32)
    labels = np.where(fg, rank[p[np.maximum(run_of, 0)]] if n_runs else 0, 0).astype(np.int32)
    return labels.reshape(dh, dw), int(len(roots))


def label_bfs(m):
    """The same by the definition, one cell at a time (small maps only)."""
    m = np.asarray(m)
    dh, dw = m.shape
    lab = np.zeros((dh, dw), np.int32)
    k = 0
    for y in range(dh):
        for x in range(dw):
            if m[y, x] < 0 or lab[y, x]:
                continue
            k += 1
            lab[y, x] = k
            todo = [(y, x)]
            while todo:
                cy, cx = todo.pop()
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < dh and 0 <= nx < dw and not lab[ny, nx] and m[ny, nx] == m[y, x]:
                        lab[ny, nx] = k
                        todo.append((ny, nx))
    return lab, k


def table_np(m, labels, k, conf=None):
    """The region table as a dict of columns (row i: id i + 1), every figure an integer."""
    m, labels = np.asarray(m, np.int64), np.asarray(labels)
    dh, dw = m.shape
    idx = np.flatnonzero(labels.ravel() > 0)
    ids = labels.ravel()[idx].astype(np.int64) - 1
    y, x = idx // dw, idx % dw
    big = np.iinfo(np.int64).max
    t = dict(cls=np.zeros(k, np.int32), area=np.bincount(ids, minlength=k).astype(np.int64))
    t["cls"][ids] = m.ravel()[idx]
    for name, init, op, val in (("y0", big, np.minimum, y), ("x0", big, np.minimum, x), ("y1", 0, np.maximum, y + 1),
                                ("x1", 0, np.maximum, x + 1), ("sum_y", 0, np.add, y), ("sum_x", 0, np.add, x),
                                ("first", big, np.minimum, idx)):
        t[name] = np.full(k, init, np.int64)
        op.at(t[name], ids, val)
    if conf is not None:
        q = np.rint(np.asarray(conf, np.float32).astype(np.float64).ravel()[idx] * 2.0 ** 32).astype(np.int64).astype(np.uint64)
        t["conf_q"] = np.zeros(k, np.uint64)
        np.add.at(t["conf_q"], ids, q)
    return t


def clean_round_np(m, min_cells):
    """One cleanup round: (new map, changed cells)."""
    m = np.asarray(m, np.int64)
    dh, dw = m.shape
    labels, k = label_np(m)
    area = np.bincount(labels.ravel(), minlength=k + 1)
    small = area < min_cells
    small[0] = False
    n_cls = int(max(m.max(), 0)) + 1
    keys = []
    for cell, nb in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]),
                     (np.s_[:, :-1], np.s_[:, 1:])):
        s, t = labels[cell], labels[nb]
        vote = (s > 0) & small[s] & (t > 0) & ~small[t]
        keys.append(s[vote].astype(np.int64) * n_cls + m[nb][vote])
    key, count = np.unique(np.concatenate(keys), return_counts=True)
    comp, cls = key // n_cls, key % n_cls
    order = np.lexsort((cls, -count, comp))          # per component: most votes first, the lowest class id among equals
    comp, cls = comp[order], cls[order]
    lead = np.ones(len(comp), bool)
    lead[1:] = comp[1:] != comp[:-1]
    to = np.full(k + 1, -1, np.int64)
    to[comp[lead]] = cls[lead]
    new = to[labels]
    out = np.where(new >= 0, new, m)
    return out, int((out != m).sum())


def clean_np(m, min_cells, rounds=1):
    """(cleaned map, changed cells in all rounds); rounds end early when nothing changed."""
    cur, total = np.asarray(m, np.int64), 0
    for _ in range(rounds):
        out, changed = clean_round_np(cur, min_cells)
        if not changed:
            break
        cur, total = out, total + changed
    return cur.copy(), total


# ---- canvases (shared with the GPU tests) -----------------------------------------------------------------------------------
CANVASES = ["noise1", "noise5", "noise64", "noise1_gaps", "noise5_gaps", "noise64_gaps", "patch7", "patch14", "one_class",
            "all_minus1", "checkerboard", "spiral", "comb"]


def canvas(kind, shape, seed=0):
    """int64 class map of a kind of CANVASES; (map, n_cls)."""
    dh, dw = shape
    rng = np.random.default_rng(seed + 1000 * dh + dw)
    if kind.startswith("noise"):
        n_cls = int(re.match(r"noise(\d+)", kind).group(1))
        m = rng.integers(0, n_cls, shape)
        if kind.endswith("_gaps"):
            m[rng.random(shape) < 0.2] = -1
        return m.astype(np.int64), n_cls
    if kind.startswith("patch"):                      # a coarse noise grid, upsampled: what a patch classifier's map looks like
        f = int(kind[5:])
        coarse = rng.integers(-1, 5, (dh // f + 2, dw // f + 2))
        oy, ox = int(rng.integers(0, f)), int(rng.integers(0, f))
        m = np.repeat(np.repeat(coarse, f, axis=0), f, axis=1)[oy:oy + dh, ox:ox + dw]
        return np.ascontiguousarray(m, np.int64), 5
    if kind == "one_class":
        return np.full(shape, 3, np.int64), 5
    if kind == "all_minus1":
        return np.full(shape, -1, np.int64), 5
    if kind == "checkerboard":
        return ((np.arange(dh)[:, None] + np.arange(dw)[None, :]) & 1).astype(np.int64), 2
    if kind == "spiral":                              # class 1: one path, one cell wide, wound inwards; class 0: the corridor
        m = np.zeros(shape, np.int64)
        y0, x0, y1, x1 = 0, 0, dh - 1, dw - 1
        while y0 <= y1 and x0 <= x1:
            m[y0, x0:x1 + 1] = 1
            m[y0:y1 + 1, x1] = 1
            m[y1, x0:x1 + 1] = 1
            if y1 - y0 >= 2:
                m[y0 + 2:y1 + 1, x0] = 1
                if x1 - x0 >= 2:
                    m[y0 + 2, x0 + 1] = 1
            y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        return m, 2
    if kind == "comb":                                # teeth one cell wide down the whole canvas, joined along the top row
        m = np.zeros(shape, np.int64)
        m[:, ::2] = 4
        m[0, :] = 4
        m[dh - 1, 1::4] = -1
        return m, 5
    raise KeyError(kind)


def blob_map(dh, dw, seed, gap=2):
    """Discs of random radius and class on a jittered grid over -1, at least `gap` cells apart: regions without holes and
    without diagonal pinches (asserted where it is relied on)."""
    rng = np.random.default_rng(seed)
    m = np.full((dh, dw), -1, np.int64)
    pitch = 24
    yy, xx = np.mgrid[0:dh, 0:dw]
    for gy in range(0, dh - pitch + 1, pitch):
        for gx in range(0, dw - pitch + 1, pitch):
            if rng.random() < 0.2:
                continue
            r = rng.uniform(1.5, (pitch - gap) / 2 - 2)
            cy = gy + pitch / 2 + rng.uniform(-1.5, 1.5)
            cx = gx + pitch / 2 + rng.uniform(-1.5, 1.5)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = int(rng.integers(0, 5))
    return m


def holes_map():
    """Rings, a ring inside a ring's hole, a region whose hole is reached only across a corner, on a class-0 ground."""
    m = np.zeros((40, 50), np.int64)
    m[3:20, 3:25] = 1
    m[6:17, 6:22] = 2           # a hole of 1 filled by 2 ...
    m[9:14, 9:19] = 1           # ... which holds an island of 1
    m[10:12, 11:13] = -1        # with a gap of no class inside
    m[25:35, 5:15] = 3
    m[28, 8] = 0
    m[29, 9] = 0                # two hole cells that meet at a corner: one hole ring
    m[26:33, 30:45] = 4
    m[27:32, 31:44] = -1        # a thin frame round nothing
    return m


def pinch_map():
    """Regions that touch themselves across a corner (joined elsewhere), staircases and single cells."""
    m = np.full((30, 30), -1, np.int64)
    m[2:6, 2:6] = 1
    m[6:10, 6:10] = 1           # (5, 5) and (6, 6) meet at a corner ...
    m[2:10, 10] = 1
    m[2, 6:10] = 1
    m[9, 10] = 1                # ... and are joined round the outside: the outer ring touches itself
    m[6:10, 10] = 1
    for k in range(8):
        m[15 + k, 3 + k:5 + k] = 2   # a staircase two cells wide
    m[15:25, 15:25] = 3
    m[18, 18] = 0
    m[19, 19] = 0
    m[20, 18] = 0               # three holes in a diagonal chain: one ring through two pinches
    m[27, 27] = 4
    return m


# ---- 1. the restatement against the definition and scipy ---------------------------------------------------------------------
SMALL = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 129)]


@pytest.mark.parametrize("kind", CANVASES)
def test_restatement_equals_the_definition(kind):
    for shape in SMALL:
        m, n_cls = canvas(kind, shape)
        assert m.shape == shape and m.min() >= -1 and m.max() < n_cls
        got, k = label_np(m)
        want, k_want = label_bfs(m)
        assert k == k_want and np.array_equal(got, want), (kind, shape)


def test_restatement_pinned_to_scipy_per_class():
    ndimage = pytest.importorskip("scipy.ndimage")
    for kind in CANVASES:
        for shape in [(37, 53), (200, 333)]:
            m, n_cls = canvas(kind, shape)
            got, k = label_np(m)
            assert (got > 0).sum() == (m >= 0).sum() and (k == 0 or got.max() == k)
            first = np.full(k + 1, m.size, np.int64)
            np.minimum.at(first, got.ravel(), np.arange(m.size))
            assert k == 0 or np.all(np.diff(first[1:]) > 0), "ids do not ascend with the first cell"
            total = 0
            for c in range(n_cls):
                lab, n = ndimage.label(m == c)      # the default structure: 4-connected
                total += n
                sel = m == c
                # renumbered by first cell, scipy's components of class c are the restatement's
                pairs = np.unique(np.stack([lab[sel], got[sel]]), axis=1)
                assert pairs.shape[1] == n and len(np.unique(pairs[1])) == n, (kind, shape, c)
            assert total == k


def test_the_canvases_are_what_they_claim():
    m, _ = canvas("spiral", (65, 129))
    lab, k = label_np(m)
    assert k == 2 and (lab[m == 1] == 1).all()       # one path, one corridor
    path = m == 1
    nb = np.zeros(m.shape, int)
    nb[1:] += path[:-1]; nb[:-1] += path[1:]; nb[:, 1:] += path[:, :-1]; nb[:, :-1] += path[:, 1:]
    assert (nb[path] <= 2).mean() > 0.97             # one cell wide: a cell of the path has two neighbours on it
    m, _ = canvas("comb", (200, 300))
    lab, k = label_np(m)
    assert (lab[m == 4] == 1).all() and k > 100      # every tooth hangs on the spine
    m, _ = canvas("checkerboard", (37, 53))
    assert label_np(m)[1] == 37 * 53
    m, _ = canvas("patch14", (300, 300))
    assert 50 < label_np(m)[1] < 600 and (m == -1).any()


def test_table_and_cleanup_on_a_hand_case():
    m = np.array([[0, 0, 1, 1, 1],
                  [0, 2, 1, -1, 1],
                  [0, 0, 1, 1, 1],
                  [3, 0, 0, 0, 4]], np.int64)
    lab, k = label_np(m)
    assert k == 5 and lab.tolist() == [[1, 1, 2, 2, 2], [1, 3, 2, 0, 2], [1, 1, 2, 2, 2], [4, 1, 1, 1, 5]]
    conf = np.full(m.shape, 0.5, np.float32)
    conf[1, 1] = np.float32(2.0 ** -33)               # rint(0.5) = 0: half to even
    conf[3, 0] = np.float32(3 * 2.0 ** -33)           # rint(1.5) = 2
    t = table_np(m, lab, k, conf)
    assert t["cls"].tolist() == [0, 1, 2, 3, 4] and t["area"].tolist() == [8, 8, 1, 1, 1]
    assert (t["y0"].tolist(), t["x0"].tolist(), t["y1"].tolist(), t["x1"].tolist()) == ([0, 0, 1, 3, 3], [0, 2, 1, 0, 4], [4, 3, 2, 4, 4], [4, 5, 2, 1, 5])
    assert t["first"].tolist() == [0, 2, 6, 15, 19] and t["sum_y"].tolist() == [14, 8, 1, 3, 3] and t["sum_x"].tolist() == [8, 24, 1, 0, 4]
    assert t["conf_q"].tolist() == [8 * 2 ** 31, 8 * 2 ** 31, 0, 2, 2 ** 31]
    # min_cells 2: cell (1, 1) has 3 votes for class 0 and 1 for class 1; (3, 0) two for 0; (3, 4) one for 0 and one for 1: the tie goes to 0
    out, changed = clean_np(m, 2)
    assert changed == 3 and out.tolist() == [[0, 0, 1, 1, 1], [0, 0, 1, -1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0]]
    same, changed = clean_np(m, 1)
    assert changed == 0 and np.array_equal(same, m)
    # everything small: nobody votes, nothing changes
    out, changed = clean_np(m, 100, rounds=3)
    assert changed == 0 and np.array_equal(out, m)
    # a second round sees the first one's result
    m2 = np.zeros((9, 9), np.int64)
    m2[2:7, 2:7] = 1
    m2[4, 4] = 2
    m2[3, 3] = -1
    one, c1 = clean_np(m2, 25, rounds=1)              # the 23-cell ring of 1 and the cell of 2 are small; 2 has no large neighbour
    assert c1 == 23 and one[4, 4] == 2 and one[3, 3] == -1 and (one[2:7, 2:7] == 0).sum() == 23
    two, c2 = clean_np(m2, 25, rounds=3)
    assert c2 == 24 and two[4, 4] == 0 and two[3, 3] == -1


# ---- 2. trace_polygons -------------------------------------------------------------------------------------------------------
def inside_np(ring, px, py):
    """Even-odd rule of section 4.9 in float64: bool[len(py), len(px)]."""
    a, b = ring, np.roll(ring, -1, axis=0)
    out = np.zeros((len(py), len(px)), bool)
    for (ax, ay), (bx, by) in zip(a, b):
        rows = (ay > py) != (by > py)
        if not rows.any():
            continue
        xi = ax + (py[rows] - ay) * (bx - ax) / (by - ay)
        out[rows] ^= px[None, :] < xi[:, None]
    return out


def _check_trace(m, d, layer):
    from deephisto_amd import regions
    from deephisto_amd.patch_samplers import polygon
    lab, k = label_np(m)
    t = table_np(m, lab, k)
    polys = regions.trace_polygons(lab, range(1, k + 1), d, layer)
    assert sorted(polys) == list(range(1, k + 1))
    py = (np.arange(m.shape[0]) + 0.5) * d
    px = (np.arange(m.shape[1]) + 0.5) * d
    filled = np.zeros(m.shape, np.int32)
    n_holes = 0
    for i, (outer, holes) in polys.items():
        assert outer is not None and outer.dtype == np.float64
        fill = np.zeros(m.shape, bool)
        area = 0.0
        for r, sign in [(outer, 1.0)] + [(h, -1.0) for h in holes]:
            r = r / layer
            assert np.array_equal(r, np.rint(r)) and np.all(r % d == 0)
            assert polygon.signed_area(r) > 0, "ring is not counter-clockwise"
            e = np.roll(r, -1, axis=0) - r
            e_prev = np.roll(e, 1, axis=0)
            assert np.all(e[:, 0] * e_prev[:, 1] - e[:, 1] * e_prev[:, 0] != 0), "three collinear consecutive vertices"
            assert np.all((e == 0).sum(axis=1) == 1), "an edge that is not axis-parallel"
            fill ^= inside_np(r, px, py)
            area += sign * polygon.signed_area(r)
        assert area == t["area"][i - 1] * d * d, (i, area)
        assert not (filled[fill] != 0).any(), "two regions claim one cell"
        filled[fill] = i
        n_holes += len(holes)
    assert np.array_equal(filled, lab), f"{int((filled != lab).sum())} cells differ"
    return polys, n_holes


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_trace_fills_back_to_the_label_map_blobs_and_noise(seed):
    _, n_holes = _check_trace(blob_map(100, 130, seed), 16, 2)
    assert n_holes == 0
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-1, 4, (12, 15))
    _check_trace(np.repeat(np.repeat(coarse, 5, axis=0), 5, axis=1), 10, 1)      # patch-like, classes as ground: holes
    _check_trace(rng.integers(-1, 3, (40, 45)), 7, 3)                            # noise: pinches everywhere
    _, n_holes = _check_trace((rng.random((40, 45)) < 0.7).astype(np.int64), 7, 3)   # 70 % of one class: a region full of holes
    assert n_holes > 10


def test_trace_holes_and_pinches():
    polys, n_holes = _check_trace(holes_map(), 16, 2)
    assert n_holes >= 5
    lab, _ = label_np(holes_map())
    i = int(lab[25, 5])
    assert len(polys[i][1]) == 1 and len(polys[i][1][0]) == 8      # two cells across a corner: one hole ring, it touches itself
    polys, n_holes = _check_trace(pinch_map(), 4, 1)
    lab, _ = label_np(pinch_map())
    outer = polys[int(lab[2, 2])][0]
    assert len({tuple(v) for v in outer}) < len(outer), "the outer ring should visit the pinch corner twice"
    holes = polys[int(lab[15, 15])][1]
    assert len(holes) == 1 and len(holes[0]) == 12
    _check_trace(canvas("spiral", (21, 34))[0], 16, 1)
    _check_trace(canvas("checkerboard", (9, 12))[0], 16, 1)
    _check_trace(np.zeros((1, 1), np.int64), 16, 2)
    one = _check_trace(np.zeros((3, 5), np.int64), 16, 2)[0][1][0]
    assert sorted(map(tuple, one.tolist())) == [(0.0, 0.0), (0.0, 96.0), (160.0, 0.0), (160.0, 96.0)]


def test_trace_only_the_regions_asked_for():
    from deephisto_amd import regions
    lab, k = label_np(holes_map())
    some = regions.trace_polygons(lab, [2, k], 16, 1)
    everything = regions.trace_polygons(lab, range(1, k + 1), 16, 1)
    assert sorted(some) == [2, k]
    for i in some:
        assert np.array_equal(some[i][0], everything[i][0]) and len(some[i][1]) == len(everything[i][1])
    assert regions.trace_polygons(lab, [], 16, 1) == {}
    assert regions.trace_polygons(np.zeros((4, 4), np.int32), [1], 16, 1) == {1: (None, [])}
    with pytest.raises(ValueError, match="integer"):
        regions.trace_polygons(lab.astype(np.float32), [1], 16, 1)


# ---- 3. export, then reload through the annotation parser ----------------------------------------------------------------------
def _dsc():
    from deephisto_amd.anno.utils import AnnoDescription
    from deephisto_amd.examples.predict_full_patched import KNOWN_COLORS
    return AnnoDescription.with_known_colors(KNOWN_COLORS)


def slide_regions_np(m, conf=None):
    from deephisto_amd import regions
    lab, k = label_np(m)
    t = table_np(m, lab, k, conf)
    cols = [t["cls"].astype(np.int64), t["area"], t["y0"], t["x0"], t["y1"], t["x1"], t["sum_y"], t["sum_x"], t["first"],
            (t["conf_q"].view(np.int64) if conf is not None else np.zeros(k, np.int64))]
    return lab, k, regions.SlideRegions(np.stack(cols, axis=1) if k else np.zeros((0, 10), np.int64), m.shape, conf is not None)


@pytest.mark.parametrize("layer,d,seed", [(2, 16, 3), (1, 10, 4), (3, 7, 5)])
def test_export_then_reload_gives_the_same_rings(tmp_path, layer, d, seed):
    from deephisto_amd import regions, scoring
    m = blob_map(96, 120, seed)
    conf = np.random.default_rng(seed).random(m.shape).astype(np.float32)
    lab, k, table = slide_regions_np(m, conf)
    polys = regions.trace_polygons(lab, range(1, k + 1), d, layer)
    assert k >= 8
    for outer, holes in polys.values():          # the precondition: no holes, no ring that touches itself
        assert holes == [] and len({tuple(v) for v in outer}) == len(outer)
    path = regions.export_annotation(tmp_path / "out" / "pred.json", table, polys, _dsc())
    records = json.loads(path.read_text())
    assert len(records) == k and set(records[0]) == {"class", "vertices", "holes", "area_px", "confidence"}
    for i, r in enumerate(records):
        assert r["class"] == LABELS[table.cls[i]] and r["holes"] == []
        assert r["area_px"] == table.area[i] * (d * layer) ** 2
        assert r["confidence"] == float(table.mean_confidence[i]) and 0 < r["confidence"] < 1
    h, w = m.shape[0] * d, m.shape[1] * d
    xy, start, cls, info = scoring.annotation_rings(path, _dsc(), layer, h, w)
    assert info == dict(n_rings=k, n_regions=k, skipped_class=0, failed=0)
    assert cls.tolist() == table.cls.tolist()
    for i in range(k):
        assert np.array_equal(xy[start[i]:start[i + 1]] * layer, polys[i + 1][0]), i


# ---- 4. entries, formatting, flags -------------------------------------------------------------------------------------------
def test_header_and_signatures_name_the_entries(built_lib):
    from deephisto_amd import _lib
    header = (REPO / "include" / "deephisto_hip.h").read_text()
    for name in ("dh_label_components", "dh_region_stats", "dh_clean_small_regions", "dh_label_work_size"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(built_lib, name)
    assert built_lib.dh_label_work_size(4096) == 4096 + 2 and built_lib.dh_label_work_size(4097) == 4097 + 3
    # refused before any GPU call
    assert built_lib.dh_label_components(None, 4, 4, 5, None, None, None, None) == -22 and b"null pointer" in built_lib.dh_last_error()
    assert built_lib.dh_label_components(None, 0, 4, 5, None, None, None, None) == -22 and b"must be > 0" in built_lib.dh_last_error()
    assert built_lib.dh_label_components(None, 4, 4, 65, None, None, None, None) == -22 and b"n_cls=65" in built_lib.dh_last_error()
    assert built_lib.dh_label_components(None, 1 << 16, 1 << 15, 5, None, None, None, None) == -22 and b"too large" in built_lib.dh_last_error()
    assert built_lib.dh_region_stats(None, None, None, 4, 4, 17, None, None) == -22 and b"n_components=17" in built_lib.dh_last_error()
    assert built_lib.dh_region_stats(None, None, None, 4, 4, 3, None, None) == -22 and b"null pointer" in built_lib.dh_last_error()
    assert built_lib.dh_clean_small_regions(None, None, None, 0, 4, 4, 5, 0, None, None, None, None) == -22
    assert b"min_cells=0" in built_lib.dh_last_error()


def test_slide_regions_formatting_and_records():
    m = holes_map()
    conf = np.full(m.shape, 0.75, np.float32)
    lab, k, table = slide_regions_np(m, conf)
    assert len(table) == k and table.shape == m.shape
    lines = str(table).splitlines()
    assert len(lines) == k + 2 and lines[0].split() == ["id", "class", "area", "y0", "x0", "y1", "x1", "cy", "cx", "conf"]
    areas = [int(ln.split()[2]) for ln in lines[1:-1]]
    assert areas == sorted(areas, reverse=True) and sorted(areas) == sorted(table.area.tolist())
    assert lines[-1] == f"{k} regions, {int((m >= 0).sum())} cells of 40 x 50"
    assert all(ln.split()[-1] == "0.7500" for ln in lines[1:-1])
    rec = table.to_records(_dsc(), 16, 2)
    assert len(rec) == k and json.loads(json.dumps(rec)) == rec
    i = int(lab[25, 5]) - 1
    assert rec[i]["class"] == "MM" and rec[i]["area_cells"] == 98 and rec[i]["area_px"] == 98 * 256 and rec[i]["id"] == i + 1
    assert rec[i]["bbox_px"] == [25 * 16, 5 * 16, 35 * 16, 15 * 16] and rec[i]["confidence"] == 0.75
    ys, xs = np.nonzero(lab == i + 1)
    assert rec[i]["centroid_px"] == pytest.approx([(ys.mean() + 0.5) * 16, (xs.mean() + 0.5) * 16], abs=1e-9)
    assert rec[i]["centroid_layer1"] == [2 * v for v in rec[i]["centroid_px"]]
    _, _, bare = slide_regions_np(m)
    assert bare.conf_q is None and bare.mean_confidence is None and bare.to_records(_dsc(), 16, 2)[0]["confidence"] is None
    assert str(bare).splitlines()[1].split()[-1] == "-"
    assert str(slide_regions_np(np.full((3, 3), -1, np.int64))[2]).splitlines()[-1] == "0 regions, 0 cells of 3 x 3"


def test_wrappers_refuse_before_any_library_call():
    from deephisto_amd import regions
    with pytest.raises(ValueError, match="n_classes = 65"):
        regions.label_components(np.zeros((4, 4), np.int64), 65)
    with pytest.raises(ValueError, match="non-empty"):
        regions.label_components(np.zeros((2, 3, 4), np.int64))
    with pytest.raises(ValueError, match="must be >= 1"):
        regions.clean_map(np.zeros((4, 4), np.int64), 0)


def test_cli_refuses_bad_region_flags(capsys):
    from deephisto_amd.examples.predict_full_patched import main
    base = ["--synthetic", "600", "600", "--weights", ""]
    for extra, msg in ((["--clean_rounds", "2"], "--clean_rounds needs --min_region"),
                       (["--min_region", "0"], "--min_region must be >= 1"),
                       (["--min_region", "5", "--clean_rounds", "0"], "--clean_rounds must be >= 1")):
        with pytest.raises(SystemExit) as e:
            main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err


def test_new_names_are_exported_beside_their_siblings():
    from deephisto_amd import regions
    from deephisto_amd.examples import predict_full_patched as pfp
    for name in ("label_components", "region_table", "clean_map", "trace_polygons", "export_annotation", "extract_regions",
                 "SlideRegions", "save_regions"):
        assert getattr(pfp, name) is getattr(regions, name)
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        text = (REPO / doc).read_text()
        assert "dh_label_components" in text or "extract_regions" in text, doc
    assert "4.10" in (REPO / "DESIGN.md").read_text()
