"""Scoring a class map against a polygon annotation, host side: the NumPy restatements `rasterize_np` and
`confusion_np` that the GPU tests compare against, `rasterize_np` pinned to an independent exact test (integer vertices, integer
arithmetic on doubled coordinates), the label rule through the annotation parser, the figures of SlideScore on a hand-written
matrix, the C entries' refusals and the CLI's.  CPU only: no kernel runs."""
import ctypes as C
import json
import math

import numpy as np
import pytest

LABELS = ["AT", "BG", "LP", "MM", "TUM"]


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def ring_inside_np(ring, px, py):
    """bool[len(py), len(px)]: the even-odd rule of one ring at the points (px[j], py[i]), every edge at every point, float64
    element-wise: edge a -> b counts iff (a.y > p.y) != (b.y > p.y) and p.x < a.x + (p.y - a.y) * (b.x - a.x) / (b.y - a.y)."""
    ring = np.asarray(ring, np.float64)
    a, b = ring, np.roll(ring, -1, axis=0)
    ax, ay, bx, by = (v[None, None, :] for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
    X, Y = px[None, :, None], py[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        crosses = ((ay > Y) != (by > Y)) & (X < ax + (Y - ay) * (bx - ax) / (by - ay))
    return (crosses.sum(axis=2) & 1).astype(bool)


def ring_inside_rows_np(ring, px, py):
    """The same bits, without the [rows, columns, edges] array: the intercept of an edge depends on the row only, so it is computed
    per (row, edge) with the same float64 operations, and `p.x < intercept` holds for the first k columns, k by comparisons
    (searchsorted on the increasing p.x); rows outside [min y, max y) have no straddling edge."""
    ring = np.asarray(ring, np.float64)
    a, b = ring, np.roll(ring, -1, axis=0)
    inside = np.zeros((len(py), len(px)), bool)
    rows = np.nonzero((py >= ring[:, 1].min()) & (py < ring[:, 1].max()))[0]
    for r0 in range(0, len(rows), 256):
        rr = rows[r0:r0 + 256]
        Y = py[rr][:, None]
        straddle = (a[None, :, 1] > Y) != (b[None, :, 1] > Y)
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = a[None, :, 0] + (Y - a[None, :, 1]) * (b[None, :, 0] - a[None, :, 0]) / (b[None, :, 1] - a[None, :, 1])
        ri, ei = np.nonzero(straddle)
        v = xi[ri, ei]
        assert not np.isnan(v).any()
        k = np.searchsorted(px, v, side="left")          # number of columns with p.x < intercept
        toggles = np.zeros((len(rr), len(px) + 1), np.int64)
        np.add.at(toggles, (ri, np.zeros_like(k)), 1)
        np.add.at(toggles, (ri, k), 1)
        inside[rr] = (np.cumsum(toggles, axis=1)[:, :-1] & 1).astype(bool)
    return inside


def rasterize_np(xy, ring_start, ring_class, n_cls, dh, dw, d, dense=False):
    """int32[dh, dw]: the class of the rings that hold the cell's centre ((cx + 0.5) * d, (cy + 0.5) * d) when they are of exactly
    one class, else -1."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    px, py = (np.arange(dw) + 0.5) * d, (np.arange(dh) + 0.5) * d
    assert px.dtype == np.float64
    seen = np.zeros((n_cls, dh, dw), bool)
    for r, c in enumerate(ring_class):
        ring = xy[ring_start[r]:ring_start[r + 1]]
        seen[c] |= (ring_inside_np if dense else ring_inside_rows_np)(ring, px, py)
    n_seen = seen.sum(axis=0)
    return np.where(n_seen == 1, np.argmax(seen, axis=0), -1).astype(np.int32)


def confusion_np(pred, truth, n_cls):
    """(int64[n, n + 1] counts, int64 outcome map): rows truth, columns prediction, last column prediction -1; truth -1 is not
    counted; outcome -1 unlabelled / 0 correct / 1 wrong.  A prediction outside [-1, n) is an error."""
    pred, truth = np.asarray(pred, np.int64), np.asarray(truth, np.int64)
    if ((pred < -1) | (pred >= n_cls)).any():
        raise ValueError("prediction outside [-1, n_cls)")
    m = truth >= 0
    counts = np.zeros((n_cls, n_cls + 1), np.int64)
    np.add.at(counts, (truth[m], np.where(pred[m] < 0, n_cls, pred[m])), 1)
    return counts, np.where(m, (pred != truth).astype(np.int64), -1)


def metrics_np(c):
    """The figures of DESIGN.md 4.9 from an [n, n + 1] matrix, written out with Python floats."""
    n = len(c)
    div = lambda a, b: a / b if b else math.nan   # noqa: E731
    sup = [sum(c[k]) for k in range(n)]
    prd = [sum(c[t][k] for t in range(n)) for k in range(n)]
    out = dict(precision=[div(c[k][k], prd[k]) for k in range(n)], recall=[div(c[k][k], sup[k]) for k in range(n)],
               iou=[div(c[k][k], sup[k] + prd[k] - c[k][k]) for k in range(n)],
               dice=[div(2 * c[k][k], sup[k] + prd[k]) for k in range(n)],
               accuracy=div(sum(c[k][k] for k in range(n)), sum(sup)))
    live = [k for k in range(n) if sup[k]]
    out["mean_iou"] = div(sum(out["iou"][k] for k in live), len(live))
    out["mean_dice"] = div(sum(out["dice"][k] for k in live), len(live))
    return out


# ---- the independent exact test -----------------------------------------------------------------------------------------------------
def rasterize_exact(rings, classes, n_cls, dh, dw, d):
    """Integer vertices only.  Doubled coordinates make the centres integers: P = ((2 cx + 1) d, (2 cy + 1) d), A = 2 a.  The rule
    `P.x < A.x + (P.y - A.y) (B.x - A.x) / (B.y - A.y)` is decided without a division: (P.x - A.x) (B.y - A.y) < (P.y - A.y) (B.x - A.x)
    when B.y > A.y, the reverse otherwise.  Python integers: exact."""
    seen = np.zeros((n_cls, dh, dw), bool)
    PX = (2 * np.arange(dw, dtype=np.int64) + 1) * d
    for ring, c in zip(rings, classes):
        ring = np.asarray(ring)
        assert np.issubdtype(ring.dtype, np.integer)
        A = 2 * ring.astype(np.int64)
        B = np.roll(A, -1, axis=0)
        for cy in range(dh):
            PY = (2 * cy + 1) * d
            par = np.zeros(dw, np.int64)
            for (Ax, Ay), (Bx, By) in zip(A.tolist(), B.tolist()):
                if (Ay > PY) == (By > PY):
                    continue
                lhs, rhs = (PX - Ax) * (By - Ay), (PY - Ay) * (Bx - Ax)
                par += (lhs < rhs) if By > Ay else (lhs > rhs)
            seen[c, cy] |= (par & 1).astype(bool)
    n_seen = seen.sum(axis=0)
    return np.where(n_seen == 1, np.argmax(seen, axis=0), -1).astype(np.int32)


def _pack(rings, classes):
    start = np.zeros(len(rings) + 1, np.int64)
    start[1:] = np.cumsum([len(r) for r in rings])
    return np.concatenate([np.asarray(r, np.float64) for r in rings]), start, np.asarray(classes, np.int32)


def _star(cx, cy, r_out, r_in, n):
    t = np.arange(n) * (2 * np.pi / n)
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return np.stack([np.rint(cx + r * np.cos(t)), np.rint(cy + r * np.sin(t))], axis=1).astype(np.int64)


def integer_cases():
    """name -> (rings (integer vertex arrays), classes, n_cls, h, w, d): every shape the rule has to get right."""
    d = 16   # cell centres at 8 + 16 k: integers, so edges and vertices can lie exactly on them
    cases = {
        "convex": ([[(20, 30), (300, 60), (350, 280), (120, 380), (10, 200)]], [1], 5, 400, 400, d),
        "concave": ([[(10, 10), (390, 10), (390, 390), (200, 100), (10, 390)], [(40, 200), (180, 200), (180, 380), (100, 250)]],
                    [0, 0], 3, 400, 400, d),
        "star_1000": ([_star(500, 480, 450, 200, 1000)], [4], 5, 1000, 1100, d),
        # edges exactly on the centre lines x = 8 + 16 k, y = 8 + 16 k
        "rect_on_centres": ([[(8, 8), (200, 8), (200, 104), (8, 104)], [(56, 40), (56, 136), (152, 136), (152, 40)]], [2, 3], 5, 160, 240, d),
        # vertices exactly at a centre's y: the half-open rule counts each once
        "vertex_on_centre_row": ([[(30, 72), (100, 8), (170, 72), (230, 72), (230, 200), (120, 136), (30, 200)]], [1], 2, 240, 260, d),
        "partly_outside": ([[(-100, -50), (150, -80), (200, 120), (-60, 260)], [(250, 100), (500, 150), (420, 400), (200, 330)]],
                           [0, 1], 2, 300, 320, d),
        "wholly_outside": ([[(-300, -300), (-10, -300), (-10, -10), (-300, -10)], [(400, 50), (600, 50), (600, 200), (400, 200)],
                            [(50, 50), (120, 50), (120, 120), (50, 120)]], [0, 1, 2], 3, 300, 320, d),
        "same_class_overlap": ([[(10, 10), (200, 10), (200, 200), (10, 200)], [(100, 100), (300, 100), (300, 300), (100, 300)]],
                               [2, 2], 3, 320, 320, d),
        "two_class_overlap": ([[(10, 10), (200, 10), (200, 200), (10, 200)], [(100, 100), (300, 100), (300, 300), (100, 300)]],
                              [0, 2], 3, 320, 320, d),
        "self_crossing": ([[(20, 20), (300, 280), (300, 20), (20, 280)]], [1], 2, 300, 320, d),
        # d divides neither h nor w: centres at 5 + 10 k
        "ragged_d10": ([[(15, 25), (1200, 35), (1100, 900), (600, 500), (45, 985)], _star(620, 500, 300, 120, 36)], [3, 1], 5, 999, 1237, 10),
        "one_class_one_cell": ([[(0, 0), (16, 0), (16, 16), (0, 16)]], [0], 1, 16, 16, d),
    }
    return {k: ([np.asarray(r, np.int64) for r in rings], cls, n, h, w, dd) for k, (rings, cls, n, h, w, dd) in cases.items()}


def packed_cases():
    """name -> (xy, ring_start, ring_class, n_cls, dh, dw, d) for the GPU test: the integer cases, then float cases."""
    out = {}
    for name, (rings, cls, n, h, w, d) in integer_cases().items():
        out[name] = (*_pack(rings, cls), n, h // d, w // d, d)
    return out


def test_integer_cases_cover_what_they_claim():
    c = integer_cases()
    assert len(c["star_1000"][0][0]) >= 1000
    rings, _, _, _, _, d = c["rect_on_centres"]
    assert all((v - d // 2) % d == 0 for r in rings for v in np.asarray(r).ravel())
    ring = c["vertex_on_centre_row"][0][0]
    assert sum((y - 8) % 16 == 0 for _, y in ring.tolist()) >= 5
    assert c["ragged_d10"][3] % 10 and c["ragged_d10"][4] % 10


@pytest.mark.parametrize("name", list(integer_cases()))
def test_restatement_equals_the_exact_rule(name):
    """Every cell equal: the float64 restatement (both forms) against the division-free integer rule."""
    rings, cls, n, h, w, d = integer_cases()[name]
    xy, start, rc = _pack(rings, cls)
    want = rasterize_exact(rings, cls, n, h // d, w // d, d)
    got = rasterize_np(xy, start, rc, n, h // d, w // d, d)
    assert got.dtype == np.int32 and got.shape == (h // d, w // d)
    np.testing.assert_array_equal(got, want)
    if len(xy) <= 64 or name == "star_1000":
        np.testing.assert_array_equal(rasterize_np(xy, start, rc, n, h // d, w // d, d, dense=True), want)
    if name != "wholly_outside":
        assert (want >= 0).any()
    if name == "rect_on_centres":   # half-open on both axes: the first row / column on the edge is in, the last is out
        assert want[0, 0] == 2 and want[5, 11] == 2 and (want[6, :3] == -1).all() and (want[:2, 12] == -1).all()
        assert want[2, 3] == -1 and want[7, 8] == 3 and want[8, 8] == -1   # the overlap of two classes; the second ring alone
    if name == "two_class_overlap":
        assert want[3, 3] == 0 and want[10, 10] == -1 and want[15, 15] == 2
    if name == "same_class_overlap":
        assert want[3, 3] == 2 and want[10, 10] == 2 and want[15, 15] == 2
    if name == "wholly_outside":
        assert set(np.unique(want)) == {-1, 2}


def test_float_rings_dense_and_rowwise_forms_agree():
    """Non-integer vertices: only the shared float64 rule decides; the row-wise form is the dense form bit for bit."""
    from deephisto_amd.scoring import synthetic_annotation
    rec = synthetic_annotation(700, 900, 12, 97, LABELS, seed=3)
    rings = [np.asarray(r["vertices"], np.float64) / 2 for r in rec]
    xy, start, rc = _pack(rings, [LABELS.index(r["class"]) for r in rec])
    a = rasterize_np(xy, start, rc, 5, 35, 45, 10)
    np.testing.assert_array_equal(a, rasterize_np(xy, start, rc, 5, 35, 45, 10, dense=True))
    assert (a >= 0).any() and (a == -1).any()


# ---- the annotation parser's rings and the label rule ----------------------------------------------------------------------------
def _dsc():
    from deephisto_amd.anno.utils import AnnoDescription
    from deephisto_amd.examples.predict_full_patched import KNOWN_COLORS
    return AnnoDescription.with_known_colors(KNOWN_COLORS)


def _square(x0, y0, s):
    return [[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]]


def test_annotation_rings_label_rule_layers_and_counts(tmp_path):
    from deephisto_amd.patch_samplers.region_samplers import _parse_annotations
    from deephisto_amd.scoring import annotation_rings
    h, w, d = 400, 720, 10
    records = [
        {"class": "TUM", "vertices": _square(20, 20, 160)},
        {"class": "TUM", "vertices": _square(100, 100, 160)},          # overlaps the first: one class
        {"class": "LP", "vertices": _square(200, 200, 160)},           # overlaps the second: two classes -> -1
        {"class": "NOPE", "vertices": _square(0, 0, 50)},              # a class the description does not know
        # a bow-tie goes through polygon.repair, which keeps the lobe wound like the ring (the right one) as buffer(0) does
        {"class": "MM", "vertices": [[500, 40], [700, 300], [700, 40], [500, 300]]},
        # a ring that touches itself: repaired into its two lobes, both rings of the one region
        {"class": "AT", "vertices": [[400, 10], [500, 10], [500, 110], [600, 110], [600, 210], [500, 210], [500, 110], [400, 110]]},
        {"class": "BG", "vertices": [[5, 5], [9, 9]]},                 # fails to parse
    ]
    for layer in (1, 2):
        xy, start, cls, info = annotation_rings(records, _dsc(), layer, h, w)
        assert info == dict(n_rings=6, n_regions=5, skipped_class=1, failed=1)
        assert xy.dtype == np.float64 and start.dtype == np.int64 and cls.dtype == np.int32
        assert cls.tolist() == [4, 4, 2, 3, 0, 0] and start[-1] == len(xy)
        # the numbers are the parser's own
        regs, _ = _parse_annotations([(np.zeros((h, w, 3), np.uint8), records)], layer, classes=LABELS)
        assert np.array_equal(xy[start[0]:start[1]], regs["TUM"][0].polygon)
        assert np.array_equal(xy[start[3]:start[4]], regs["MM"][0].polygon) and start[4] - start[3] == 3
        lobes = regs["AT"][0].polygon
        assert isinstance(lobes, list) and len(lobes) == 2
        assert np.array_equal(xy[start[4]:start[6]], np.concatenate(lobes))
        m = rasterize_np(xy, start, cls, 5, h // d, w // d, d)
        s = 10 * layer   # layer coordinates per cell
        cell = lambda x, y: m[int(y // s), int(x // s)]   # noqa: E731
        assert cell(50, 50) == 4 and cell(150, 150) == 4 and cell(250, 150) == 4
        assert cell(230, 230) == -1 and cell(330, 330) == 2 and cell(12, 12) == -1
        assert cell(680, 170) == 3 and cell(510, 250) == -1 and cell(640, 60) == -1 and cell(640, 280) == -1
        assert cell(450, 60) == 0 and cell(550, 160) == 0 and cell(550, 60) == -1 and cell(450, 160) == -1
    # a path and RegionAnnotation objects give the same rings
    path = tmp_path / "a.json"
    path.write_text(json.dumps(records))
    xy2, start2, cls2, info2 = annotation_rings(path, _dsc(), 2, h, w)
    assert np.array_equal(xy2, xy) and np.array_equal(start2, start) and info2 == info
    regions = [r for lb in ("TUM", "LP", "MM", "AT") for r in regs[lb]]
    xy3, start3, cls3, info3 = annotation_rings(regions, _dsc(), 2, h, w)
    assert np.array_equal(xy3, xy) and np.array_equal(start3, start) and np.array_equal(cls3, cls)
    assert info3 == dict(info, failed=0, skipped_class=0)


def test_confusion_restatement_on_a_hand_case():
    truth = np.array([[0, 0, 1, -1], [2, 2, -1, 1]])
    pred = np.array([[0, 1, 1, 2], [-1, 2, 0, 0]])
    counts, outcome = confusion_np(pred, truth, 3)
    assert counts.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1]]
    assert outcome.tolist() == [[0, 1, 0, -1], [1, 0, -1, 1]]
    with pytest.raises(ValueError):
        confusion_np(np.array([3]), np.array([-1]), 3)
    assert not confusion_np(pred, np.full((2, 4), -1), 3)[0].any()


# ---- SlideScore --------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_slide_score_figures_sum_and_json():
    from deephisto_amd.scoring import SlideScore
    c1 = [[5, 1, 0, 2], [0, 0, 0, 0], [1, 0, 3, 0]]     # class 1: no support, predicted once; 2 unclassified cells of class 0
    s = SlideScore(np.array(c1), ["a", "b", "c"], n_cells=20)
    assert s.support.tolist() == [8, 0, 4] and s.n_labelled == 12 and s.n_unlabelled == 8 and s.n_unclassified == 2
    assert _close(s.precision, [5 / 6, 0.0, 1.0]) and _close(s.recall, [5 / 8, math.nan, 3 / 4])
    assert _close(s.iou, [5 / 9, 0.0, 3 / 4]) and _close(s.dice, [10 / 14, 0.0, 6 / 7])
    assert s.accuracy == 8 / 12 and s.mean_iou == (5 / 9 + 3 / 4) / 2 and s.mean_dice == (10 / 14 + 6 / 7) / 2
    want = metrics_np(c1)
    for k in ("precision", "recall", "iou", "dice"):
        assert _close(getattr(s, k), want[k]), k
    assert (s.accuracy, s.mean_iou, s.mean_dice) == (want["accuracy"], want["mean_iou"], want["mean_dice"])
    # a class nothing predicts and nothing labels: every figure nan, left out of the means
    c2 = [[2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 3]]
    s2 = SlideScore(np.array(c2), ["a", "b", "c"], n_cells=10)
    assert np.isnan([s2.precision[1], s2.recall[1], s2.iou[1], s2.dice[1]]).all() and math.isnan(s2.precision[2])
    assert s2.recall[2] == 0.0 and s2.mean_iou == 0.5
    both = s + s2
    assert both.confusion.tolist() == (np.array(c1) + np.array(c2)).tolist() and both.n_cells == 30 and both.n_unlabelled == 13
    assert _close(both.iou, metrics_np((np.array(c1) + np.array(c2)).tolist())["iou"])
    empty = SlideScore(np.zeros((3, 4), np.int64), ["a", "b", "c"])
    assert math.isnan(empty.accuracy) and math.isnan(empty.mean_iou) and empty.n_unlabelled is None
    # JSON round trip
    back = SlideScore.from_dict(json.loads(json.dumps(s.to_dict(), allow_nan=False)))
    assert back.confusion.tolist() == c1 and back.labels == s.labels and back.n_cells == 20
    assert back.to_dict() == s.to_dict() and s.to_dict()["per_class"]["b"]["recall"] is None
    text = str(s)
    assert "accuracy 0.6667" in text and "unclassified 2" in text and text.splitlines()[1].startswith("a ")
    with pytest.raises(ValueError):
        SlideScore(np.zeros((3, 3), np.int64), ["a", "b", "c"])
    with pytest.raises(ValueError):
        s + SlideScore(np.zeros((3, 4), np.int64), ["a", "b", "x"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments(built_lib):
    """Every case fails before a device call, so fake addresses are safe here."""
    lib = built_lib
    fake = C.c_void_p(1 << 20)
    xy = np.array([[0, 0], [10, 0], [10, 10], [0, 10], [5, 5], [6, 6]], np.float64)

    def err():
        return lib.dh_last_error()

    def ras(xy=xy, start=(0, 4), cls=(1,), n_cls=5, dh=10, dw=12, d=16, labels=fake, null=()):
        s, c = np.asarray(start, np.int64), np.asarray(cls, np.int32)
        ptr = lambda a, nm: None if nm in null else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        return lib.dh_rasterize_regions(ptr(xy, "xy"), ptr(s, "start"), ptr(c, "cls"), len(c), n_cls, dh, dw, d, labels, None)

    assert ras(labels=None) == -22 and b"labels" in err()
    for nm in ("xy", "start", "cls"):
        assert ras(null=(nm,)) == -22 and b"null pointer (xy, ring_start, ring_class)" in err()
    assert ras(start=(0, 4, 6), cls=(1, 2)) == -22 and b"ring 1 has 2 vertices" in err()
    assert ras(cls=(5,)) == -22 and b"class id 5 outside [0, 5)" in err()
    assert ras(cls=(-1,)) == -22 and b"class id -1" in err()
    assert ras(n_cls=65) == -22 and b"n_cls=65" in err()
    assert ras(n_cls=0) == -22 and b"n_cls=0" in err()
    assert ras(dh=0) == -22 and b"dh=0" in err()
    assert ras(dw=-3) == -22 and b"dw=-3" in err()
    assert ras(d=0) == -22 and b"downscale=0" in err()
    bad = xy.copy()
    bad[2, 1] = np.nan
    assert ras(xy=bad) == -22 and b"coordinate 5" in err()
    assert lib.dh_rasterize_regions(None, None, None, -1, 5, 10, 12, 16, fake, None) == -22 and b"n_rings=-1" in err()

    counts = np.ones((5, 6), np.int64)
    cp = counts.ctypes.data_as(C.c_void_p)
    assert lib.dh_confusion_matrix(fake, fake, 10, 65, cp, None, None) == -22 and b"n_cls=65" in err()
    assert lib.dh_confusion_matrix(fake, fake, 10, 0, cp, None, None) == -22 and b"n_cls=0" in err()
    assert lib.dh_confusion_matrix(fake, fake, -1, 5, cp, None, None) == -22 and b"n_cells=-1" in err()
    assert lib.dh_confusion_matrix(fake, fake, 10, 5, None, None, None) == -22 and b"counts" in err()
    assert lib.dh_confusion_matrix(None, fake, 10, 5, cp, None, None) == -22 and b"pred" in err()
    assert lib.dh_confusion_matrix(fake, None, 10, 5, cp, None, None) == -22 and b"truth" in err()
    assert lib.dh_confusion_matrix(None, None, 0, 5, cp, None, None) == 0 and not counts.any()   # no cells: all zero, no GPU call


def test_wrappers_refuse_before_any_library_call():
    import torch

    from deephisto_amd import scoring
    from deephisto_amd.anno.utils import AnnoClass, AnnoDescription
    with pytest.raises(ValueError, match="pred must live in GPU memory"):
        scoring.confusion(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="GPU memory"):
        scoring.rasterize_rings(np.zeros((3, 2)), [0, 3], [0], 5, 4, 4, 16, device="cpu")
    many = AnnoDescription([AnnoClass(id=i, label=f"c{i}") for i in range(65)])
    with pytest.raises(ValueError, match="1 to 64 classes"):
        scoring.rasterize_annotation([], many, 1, 64, 64, 16)


def test_cli_refuses_bad_score_flags(tmp_path, capsys, monkeypatch):
    """Refused by argparse before the process group or any GPU is touched."""
    from deephisto_amd import distributed
    from deephisto_amd.examples.predict_full_patched import main
    monkeypatch.setattr(distributed, "init_from_env", lambda *a, **k: pytest.fail("init_from_env was reached"))
    foreign = tmp_path / "foreign.json"
    foreign.write_text(json.dumps([{"class": "NOPE", "vertices": _square(0, 0, 100)}]))
    broken = tmp_path / "broken.json"
    broken.write_text("{not json")
    for extra, msg in ((["--score_json", str(tmp_path / "s.json")], "--score_json needs --anno"),
                       (["--anno", str(tmp_path / "missing.json")], "no such file"),
                       (["--anno", str(foreign)], "belongs to a known class"),
                       (["--anno", str(broken)], "not a JSON list")):
        with pytest.raises(SystemExit) as e:
            main(["--synthetic", "512", "512", "--weights", "", *extra])
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, msg
    assert not (tmp_path / "s.json").exists()


def test_new_names_are_exported_beside_their_siblings():
    import importlib
    import sys
    from pathlib import Path

    from deephisto_amd.examples import predict_full_patched as product
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "compat"))
    try:
        compat = importlib.import_module("examples.predict_full_patched")
    finally:
        sys.path.pop(0)
    for name in ("score_prediction", "rasterize_annotation", "confusion", "SlideScore", "save_score"):
        assert getattr(compat, name) is getattr(product, name), name
