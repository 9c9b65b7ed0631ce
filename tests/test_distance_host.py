"""Distance maps of a class map, the host side: the NumPy restatements that tests/test_gpu_distance.py
holds the device to -- `edt_bruteforce` (the definition), `edt_np` (separable, pinned to the definition and to scipy),
`mask_np`, `signed_np`, `bands_np`, `tolerant_truth_np`, `surface_np` -- checked on hand-made cases with known answers; header /
signature entries and the refusals that fire before any GPU call; CLI flag errors.  Everything is integer-exact."""
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_regions_host import blob_map  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
INT32_MAX = 2 ** 31 - 1


# ---- the restatements --------------------------------------------------------------------------------------------------------
def edt_bruteforce(mask):
    """(d2 int32, nearest int32) by the definition: over all feature cells the minimum of (dy^2 + dx^2, linear index)."""
    mask = np.asarray(mask) != 0
    dh, dw = mask.shape
    f = np.flatnonzero(mask.ravel())                  # ascending: argmin takes the smallest index among equals
    if f.size == 0:
        return np.full((dh, dw), INT32_MAX, np.int32), np.full((dh, dw), -1, np.int32)
    y, x = np.divmod(np.arange(dh * dw, dtype=np.int64), dw)
    d = (y[:, None] - f[None, :] // dw) ** 2 + (x[:, None] - f[None, :] % dw) ** 2
    k = d.argmin(axis=1)
    return d[np.arange(dh * dw), k].reshape(dh, dw).astype(np.int32), f[k].reshape(dh, dw).astype(np.int32)


def column_nearest_np(mask):
    """int64[dh, dw]: the row of the nearest feature cell of the cell's column, the upper of two equals; -1 without one."""
    mask = np.asarray(mask) != 0
    dh, dw = mask.shape
    rows = np.arange(dh, dtype=np.int64)[:, None]
    far = 4 * dh + 4
    up = np.maximum.accumulate(np.where(mask, rows, -far), axis=0)
    down = np.minimum.accumulate(np.where(mask, rows, far)[::-1], axis=0)[::-1]
    near = np.where(rows - up <= down - rows, up, down)
    return np.where((up < 0) & (down >= far), -1, near)


def edt_np(mask, window=None):
    """(d2 int32, nearest int32), separable: `column_nearest_np`, then per cell the minimum over the offsets -R .. R along the
    row of the key (k^2 + dy^2) * 2^31 + index, a cell's own column first and then outwards.  A column farther than R is
    strictly worse than a result <= R^2, so the offsets end as soon as every cell has one (checked every eighth step), and at
    the row's width at the latest.  `window` caps R for a mask that is known to have a feature within R cells of every
    cell: asserted."""
    mask = np.asarray(mask) != 0
    dh, dw = mask.shape
    none = np.int64(1) << 62
    if not mask.any():
        assert window is None or window >= dw - 1, f"no feature at all within the window of {window} columns"
        return np.full((dh, dw), INT32_MAX, np.int32), np.full((dh, dw), -1, np.int32)
    near = column_nearest_np(mask)
    rows = np.arange(dh, dtype=np.int64)[:, None]
    R = dw - 1 if window is None else min(int(window), dw - 1)
    col = np.where(near >= 0, ((near - rows) ** 2 << 31) + near * dw + np.arange(dw, dtype=np.int64)[None, :], none)
    best = col.copy()
    for r in range(1, R + 1):
        for k in (-r, r):
            lo, hi = max(0, -k), min(dw, dw - k)      # cells x in [lo, hi) have the column x + k
            cand = col[:, lo + k:hi + k]
            np.minimum(best[:, lo:hi], np.where(cand < none, cand + (np.int64(r * r) << 31), none), out=best[:, lo:hi])
        if r % 8 == 0 and int(best.max() >> 31) <= r * r:
            break
    d2 = best >> 31
    if R < dw - 1:
        assert int(d2.max()) <= R * R, f"a cell is farther than the window of {R} columns from every feature"
    return d2.astype(np.int32), (best & (2 ** 31 - 1)).astype(np.int32)


def member_np(m, classes, include_unclassified=False):
    m = np.asarray(m, np.int64)
    return np.isin(m, list(classes)) & (m >= 0) | ((m == -1) & bool(include_unclassified))


def mask_np(m, classes, include_unclassified=False, mode=0):
    """uint8 mask of `dh_class_mask`: 0 the members, 1 the members with an in-canvas 4-neighbour that is not one, 2 the cells
    with an in-canvas 4-neighbour of another value."""
    m = np.asarray(m, np.int64)
    if mode == 2:
        key, hit = m, np.zeros(m.shape, bool)
    else:
        key = member_np(m, classes, include_unclassified)
        if mode == 0:
            return key.astype(np.uint8)
        hit = np.zeros(m.shape, bool)
    hit[1:, :] |= key[1:, :] != key[:-1, :]
    hit[:-1, :] |= key[:-1, :] != key[1:, :]
    hit[:, 1:] |= key[:, 1:] != key[:, :-1]
    hit[:, :-1] |= key[:, :-1] != key[:, 1:]
    return (hit if mode == 2 else hit & key).astype(np.uint8)


def signed_np(m, classes, include_unclassified=False, edt=edt_np):
    inside = member_np(m, classes, include_unclassified)
    return np.where(inside, -edt(~inside)[0].astype(np.int64), edt(inside)[0].astype(np.int64)).astype(np.int32)


def _sq(e):
    return e * e if e >= 0 else -e * e


def bands_np(m, classes, edges_px, downscale, include_unclassified=False, edt=edt_np):
    return bands_of_signed_np(signed_np(m, classes, include_unclassified, edt), edges_px, downscale)


def bands_of_signed_np(s, edges_px, downscale):
    s = np.asarray(s).astype(np.int64)
    sd = s * downscale * downscale
    out = np.full(s.shape, -1, np.int64)
    for i in range(len(edges_px) - 1):
        out[(sd >= _sq(edges_px[i])) & (sd < _sq(edges_px[i + 1])) & (np.abs(s) != INT32_MAX)] = i
    return out


def composition_np(pred, bands, n_classes, n_bands):
    out = np.zeros((n_bands, n_classes + 1), np.int64)
    for b in range(n_bands):
        for c in list(range(n_classes)) + [-1]:
            out[b, c] = int(((bands == b) & (pred == c)).sum())
    return out


def tolerant_truth_np(truth, tolerance_px, downscale, edt=edt_np):
    truth = np.asarray(truth)
    d2 = edt(mask_np(truth, [], mode=2))[0].astype(np.int64)
    out = truth.astype(np.int32).copy()
    out[d2 * downscale * downscale < tolerance_px * tolerance_px] = -1
    return out


def confusion_np(pred, truth, n):
    out = np.zeros((n, n + 1), np.int64)
    for t in range(n):
        for p in list(range(n)) + [-1]:
            out[t, p] = int(((truth == t) & (pred == p)).sum())
    return out


def rank95_np(n):
    return -(-95 * n // 100)                          # ceil(0.95 n) in integers


def surface_np(pred, truth, cls, downscale=1, edt=edt_np):
    """dict(n_pred, n_truth, hausdorff, hd95, assd): the figures in float64 from the sorted integers, as section 4.22 states them."""
    a, b = mask_np(pred, [cls], mode=1) != 0, mask_np(truth, [cls], mode=1) != 0
    na, nb = int(a.sum()), int(b.sum())
    if na == 0 or nb == 0:
        return dict(n_pred=na, n_truth=nb, hausdorff=math.nan, hd95=math.nan, assd=math.nan)
    da = np.sqrt(np.sort(edt(b)[0][a].astype(np.int64)).astype(np.float64))
    db = np.sqrt(np.sort(edt(a)[0][b].astype(np.int64)).astype(np.float64))
    d = float(downscale)
    return dict(n_pred=na, n_truth=nb, hausdorff=float(max(da[-1], db[-1])) * d,
                hd95=float(max(da[rank95_np(na) - 1], db[rank95_np(nb) - 1])) * d, assd=float((da.sum() + db.sum()) / (na + nb)) * d)


# ---- masks for both test files -------------------------------------------------------------------------------------------------
def corner_masks(shape):
    """{name: mask}: the empty mask, the full one, a single feature in every corner and in the centre."""
    dh, dw = shape
    out = {"empty": np.zeros(shape, np.uint8), "full": np.ones(shape, np.uint8)}
    for name, (y, x) in dict(tl=(0, 0), tr=(0, dw - 1), bl=(dh - 1, 0), br=(dh - 1, dw - 1), centre=(dh // 2, dw // 2)).items():
        out[name] = np.zeros(shape, np.uint8)
        out[name][y, x] = 1
    return out


def symmetric_pair(shape):
    """Two features mirrored through the canvas centre on the anti-diagonal: the cells of the middle row(s), of the middle
    column(s) and of the diagonal between them are as far from one as from the other."""
    dh, dw = shape
    m = np.zeros(shape, np.uint8)
    k = min(dh, dw) // 4
    m[k, dw - 1 - k] = m[dh - 1 - k, k] = 1
    return m


def lattice_mask(shape, seed, pitch=24, jitter=5):
    """A feature per `pitch` x `pitch` box, jittered by up to `jitter`: every cell is within (pitch + jitter) * sqrt(2) cells of
    one, so a window of 2 * pitch columns holds the nearest."""
    dh, dw = shape
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.uint8)
    for y in range(0, dh, pitch):
        for x in range(0, dw, pitch):
            m[min(dh - 1, y + int(rng.integers(0, jitter + 1))), min(dw - 1, x + int(rng.integers(0, jitter + 1)))] = 1
    return m


def tiled_blob_map(shape, seed, tile=(250, 300)):
    """`blob_map` for a large canvas: one tile of discs repeated (a disc stays inside its pitch box, so the seams cut none)."""
    dh, dw = shape
    th, tw = min(dh, tile[0]), min(dw, tile[1])
    return np.ascontiguousarray(np.tile(blob_map(th, tw, seed), (-(-dh // th), -(-dw // tw)))[:dh, :dw])


def holed_blob_map(shape, seed):
    """`tiled_blob_map` (classes 0 .. 4 on -1; on a canvas too thin for a disc, runs of five cells of a random class or -1)
    with a class-63 stripe and -1 holes punched in."""
    dh, dw = shape
    rng = np.random.default_rng(seed + 7)
    if min(dh, dw) < 24:
        m = np.repeat(np.repeat(rng.integers(-1, 5, (dh // 5 + 1, dw // 5 + 1)), 5, axis=0), 5, axis=1)[:dh, :dw].astype(np.int64)
    else:
        m = tiled_blob_map(shape, seed)
    m[rng.random(shape) < 0.03] = -1
    m[:, dw // 3] = 63
    return np.ascontiguousarray(m)


SMALL = [(1, 1), (1, 47), (47, 1), (13, 21), (37, 40), (48, 48)]


# ---- 1. the separable restatement is the definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
def test_edt_np_equals_the_definition(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    masks = dict(corner_masks(shape), pair=symmetric_pair(shape))
    for density in (0.5, 0.05, 1 / 500):
        masks[f"random{density:.3f}"] = (rng.random(shape) < density).astype(np.uint8)
    masks["stripes_h"] = np.zeros(shape, np.uint8)
    masks["stripes_h"][::5, :] = 1
    masks["stripes_v"] = np.zeros(shape, np.uint8)
    masks["stripes_v"][:, 2::7] = 1
    for name, mask in masks.items():
        d2, near = edt_np(mask)
        want_d2, want_near = edt_bruteforce(mask)
        assert np.array_equal(d2, want_d2) and np.array_equal(near, want_near), name
        assert d2.dtype == np.int32 and near.dtype == np.int32


def test_the_symmetric_pair_ties_in_every_row_column_and_on_the_diagonal():
    mask = symmetric_pair((41, 41))
    (ya, xa), (yb, xb) = np.argwhere(mask)
    y, x = np.mgrid[0:41, 0:41]
    tie = (y - ya) ** 2 + (x - xa) ** 2 == (y - yb) ** 2 + (x - xb) ** 2
    assert tie.any(axis=0).all() and tie.any(axis=1).all() and tie[np.arange(41), np.arange(41)].all()
    d2, near = edt_np(mask)
    assert (near[tie] == ya * 41 + xa).all()          # the upper feature has the smaller index


def test_a_window_that_holds_the_nearest_gives_the_same_and_one_that_does_not_is_refused():
    mask = lattice_mask((90, 130), 3)
    full = edt_np(mask)
    win = edt_np(mask, window=48)
    assert np.array_equal(full[0], win[0]) and np.array_equal(full[1], win[1])
    with pytest.raises(AssertionError, match="window"):
        edt_np(corner_masks((60, 60))["tl"], window=10)


def test_edt_np_pinned_to_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for shape, mask in (((1000, 2049), lattice_mask((1000, 2049), 1)), ((300, 517), mask_np(blob_map(300, 517, 2), range(5), mode=1)),
                        ((64, 70), symmetric_pair((64, 70)))):
        iy, ix = ndimage.distance_transform_edt(mask == 0, return_distances=False, return_indices=True)
        y, x = np.mgrid[0:shape[0], 0:shape[1]]
        d2 = (iy.astype(np.int64) - y) ** 2 + (ix.astype(np.int64) - x) ** 2   # in integers from scipy's indices; its tie choice is its own
        assert np.array_equal(edt_np(mask, window=60)[0], d2), shape


# ---- 2. masks, signed distances, bands, tolerance, surface figures on hand-made cases --------------------------------------------
def test_mask_np_against_a_plain_loop():
    rng = np.random.default_rng(11)
    m = rng.integers(-1, 4, (9, 11)).astype(np.int64)
    m[0, :4], m[:, 10], m[8, 5:] = 63, 2, -1           # classes and -1 on the canvas edge
    for classes, incl in (([2], False), ([0, 2, 63], False), ([63], True), ([], True)):
        for mode in (0, 1, 2):
            want = np.zeros(m.shape, np.uint8)
            for y in range(9):
                for x in range(11):
                    inside = lambda v: (v in classes) or (v == -1 and incl)   # noqa: E731
                    nb = [m[ny, nx] for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= ny < 9 and 0 <= nx < 11]
                    if mode == 0:
                        want[y, x] = inside(m[y, x])
                    elif mode == 1:
                        want[y, x] = inside(m[y, x]) and any(not inside(v) for v in nb)
                    else:
                        want[y, x] = any(v != m[y, x] for v in nb)
            assert np.array_equal(mask_np(m, classes, incl, mode), want), (classes, incl, mode)
    one = np.full((5, 6), 3, np.int64)                  # one class to the canvas edge: no boundary, no change
    assert mask_np(one, [3], mode=0).all() and not mask_np(one, [3], mode=1).any() and not mask_np(one, [], mode=2).any()


def test_signed_distance_on_a_3_4_5_offset():
    m = np.zeros((10, 10), np.int64)
    m[2, 3] = 1
    s = signed_np(m, [1])
    assert s[5, 7] == 25 and s[2, 3] == -1 and s[2, 4] == 1 and s[9, 9] == 49 + 36
    block = np.zeros((9, 9), np.int64)
    block[2:7, 2:7] = 1                                # a 5 x 5 square: its centre is 3 cells from the nearest cell outside
    s = signed_np(block, [1])
    assert s[4, 4] == -9 and s[2, 2] == -1 and s[0, 0] == 8 and (s != 0).all()
    assert (signed_np(np.ones((3, 4), np.int64), [1]) == -INT32_MAX).all()
    assert (signed_np(np.ones((3, 4), np.int64), [2]) == INT32_MAX).all()
    assert (signed_np(np.full((3, 4), -1, np.int64), [], True) == -INT32_MAX).all()


def test_band_edges_that_land_on_a_cell():
    m = np.zeros((1, 8), np.int64)
    m[0, 0] = 1                                        # s = -1 at the member, x^2 to its right
    assert bands_np(m, [1], [0, 3, 5], 1)[0].tolist() == [-1, 0, 0, 1, 1, -1, -1, -1]    # 9 is in [9, 25), 25 is not
    assert bands_np(m, [1], [-1, 0, 3], 1)[0].tolist() == [0, 1, 1, -1, -1, -1, -1, -1]  # sq(-1) = -1 <= -1
    assert bands_np(m, [1], [-5, -1], 1)[0].tolist() == [-1] * 8                          # -1 is not < -1
    # downscale 16, an edge of 40 px: s * 256 < 1600 holds for s = 1, 4; 1600 <= s * 256 < 10000 for s = 9 .. 36
    assert bands_np(m, [1], [0, 40, 100], 16)[0].tolist() == [-1, 0, 0, 1, 1, 1, 1, -1]
    assert (bands_np(np.ones((2, 3), np.int64), [1], [-500, 0, 500], 16) == -1).all()     # no border at all
    comp = composition_np(np.array([[1, 0, 0, 2, -1, 2, 0, 0]]), bands_np(m, [1], [0, 3, 5], 1), 3, 2)
    assert comp.tolist() == [[2, 0, 0, 0], [0, 0, 1, 1]]


def test_tolerant_truth_on_a_hand_case():
    truth = np.full((1, 10), -1, np.int32)
    truth[0, 2:8] = 1                                  # changes at cells 1 | 2 and 7 | 8
    assert tolerant_truth_np(truth, 0, 1)[0].tolist() == truth[0].tolist()
    assert tolerant_truth_np(truth, 1, 1)[0].tolist() == [-1, -1, -1, 1, 1, 1, 1, -1, -1, -1]   # exactly the change cells
    assert tolerant_truth_np(truth, 2, 1)[0].tolist() == [-1, -1, -1, -1, 1, 1, -1, -1, -1, -1]  # d2 = 1 < 4, d2 = 4 is not
    assert tolerant_truth_np(truth, 16, 16)[0].tolist() == tolerant_truth_np(truth, 1, 1)[0].tolist()
    assert tolerant_truth_np(truth, 17, 16)[0].tolist() == tolerant_truth_np(truth, 2, 1)[0].tolist()   # 256 < 289
    flat = np.full((3, 3), 2, np.int32)                # no label change anywhere: nothing within any tolerance
    assert np.array_equal(tolerant_truth_np(flat, 500, 16), flat)
    pred = np.array([[1, 1, 1, 1, 0, 1, 1, 1, 0, 0]])
    assert confusion_np(pred, tolerant_truth_np(truth, 1, 1), 2).tolist() == [[0, 0, 0], [1, 3, 0]]


def test_surface_figures_of_concentric_squares_identical_boundaries_and_an_empty_side():
    pred, truth = np.zeros((40, 40), np.int64), np.zeros((40, 40), np.int64)
    pred[10:30, 10:30] = 1
    truth[5:35, 5:35] = 1
    s = surface_np(pred, truth, 1)
    assert (s["n_pred"], s["n_truth"]) == (4 * 19, 4 * 29)
    # corner to corner; of the 116 truth cells the four corners are 50 away and the eight beside them 41: rank 111 is a 41
    assert s["hausdorff"] == math.sqrt(50.0) and s["hd95"] == math.sqrt(41.0)
    assert surface_np(pred, truth, 1, downscale=16)["hausdorff"] == math.sqrt(50.0) * 16
    assert 5.0 <= s["assd"] <= math.sqrt(50.0)
    same = surface_np(pred, pred, 1)
    assert (same["hausdorff"], same["hd95"], same["assd"]) == (0.0, 0.0, 0.0) and same["n_pred"] == same["n_truth"] == 76
    none = surface_np(pred, truth, 3)
    assert (none["n_pred"], none["n_truth"]) == (0, 0) and all(math.isnan(none[k]) for k in ("hausdorff", "hd95", "assd"))
    half = surface_np(pred, np.zeros((40, 40), np.int64), 1)
    assert (half["n_pred"], half["n_truth"]) == (76, 0) and math.isnan(half["assd"])


def test_nearest_rank_and_the_module_s_figures():
    from deephisto_amd import distance
    assert [rank95_np(n) for n in (1, 19, 20, 21, 100)] == [1, 19, 19, 20, 95]
    assert [distance.nearest_rank(n) for n in (1, 19, 20, 21, 100)] == [1, 19, 19, 20, 95]
    rng = np.random.default_rng(4)
    for na, nb in ((1, 1), (19, 20), (21, 100), (100, 19)):
        a, b = rng.integers(0, 500, na), rng.integers(0, 500, nb)
        got = distance.surface_figures(a, b, 16)
        sa, sb = np.sort(a), np.sort(b)
        assert got.hausdorff == math.sqrt(max(sa[-1], sb[-1])) * 16.0
        assert got.hd95 == max(math.sqrt(sa[rank95_np(na) - 1]), math.sqrt(sb[rank95_np(nb) - 1])) * 16.0
        assert got.assd == float((np.sqrt(sa.astype(np.float64)).sum() + np.sqrt(sb.astype(np.float64)).sum()) / (na + nb)) * 16.0
        assert (got.n_pred, got.n_truth) == (na, nb)
    empty = distance.surface_figures(np.zeros(0, np.int32), [4, 9])
    assert (empty.n_pred, empty.n_truth) == (0, 2) and math.isnan(empty.hausdorff)
    assert empty.to_dict() == dict(n_pred=0, n_truth=2, hausdorff=None, hd95=None, assd=None)
    assert distance.class_bits([0, 5, 63]) == 1 | 1 << 5 | 1 << 63 and distance.class_bits([]) == 0
    with pytest.raises(ValueError, match="outside 0"):
        distance.class_bits([64])
    for bad in ([0], [0, 0, 5], [5, 0], [0, 1.5]):
        with pytest.raises(ValueError, match="ascending"):
            distance.check_edges(bad)
    assert distance.check_edges([-500, 0, 500]) == [-500, 0, 500]


def test_save_distance_report_writes_one_json(tmp_path):
    import json
    from deephisto_amd import distance, scoring
    score = scoring.SlideScore(np.array([[3, 1, 0], [0, 2, 1]]), ["a", "b"], 12)
    sd = distance.SurfaceDistance(4, 0, math.nan, math.nan, math.nan)
    path = distance.save_distance_report(tmp_path / "sub" / "d.json", 16, margin=dict(label="a", edges_px=[-16, 0, 16],
                                         class_labels=["a", "b"], counts=np.arange(6).reshape(2, 3)),
                                         tolerant=dict(tolerance_px=32, score=score), surface={"a": sd})
    doc = json.loads(path.read_text())
    assert doc["downscale"] == 16 and doc["margin"]["counts"] == [[0, 1, 2], [3, 4, 5]] and doc["margin"]["edges_px"] == [-16, 0, 16]
    assert doc["tolerant"] == dict(tolerance_px=32, score=score.to_dict())
    assert doc["surface"] == {"a": dict(n_pred=4, n_truth=0, hausdorff=None, hd95=None, assd=None)}
    assert json.loads(distance.save_distance_report(tmp_path / "e.json", 4).read_text()) == dict(downscale=4, margin=None, tolerant=None, surface=None)


# ---- 3. entries and refusals, no kernel run ---------------------------------------------------------------------------------------
def test_header_and_signatures_name_the_entries(built_lib):
    from deephisto_amd import _lib
    header = (REPO / "include" / "deephisto_hip.h").read_text()
    for name in ("dh_class_mask", "dh_distance_work_size", "dh_distance_transform"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(built_lib, name)
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert "dh_distance_transform" in (REPO / doc).read_text(), doc
    assert "4.22" in (REPO / "DESIGN.md").read_text()
    assert built_lib.dh_abi_version() == 1


def test_entries_refuse_bad_arguments_before_any_gpu_call(built_lib):
    err = lambda: built_lib.dh_last_error().decode()   # noqa: E731
    assert built_lib.dh_distance_transform(None, 32768, 4, None, None, None, None) == -22 and "32767" in err()
    assert built_lib.dh_distance_transform(None, 4, 32768, None, None, None, None) == -22 and "32767" in err()
    assert built_lib.dh_distance_transform(None, 0, 4, None, None, None, None) == -22 and "32767" in err()
    assert built_lib.dh_distance_transform(None, 4, 4, None, None, None, None) == -22 and "null pointer" in err()
    assert built_lib.dh_class_mask(None, 4, 4, 1, 0, 3, None, None) == -22 and "mode=3" in err()
    assert built_lib.dh_class_mask(None, 4, 4, 1, 0, -1, None, None) == -22 and "mode=-1" in err()
    assert built_lib.dh_class_mask(None, 4, 40000, 1, 0, 0, None, None) == -22 and "32767" in err()
    assert built_lib.dh_class_mask(None, 4, 4, 1, 0, 0, None, None) == -22 and "null pointer" in err()
    assert built_lib.dh_distance_work_size(0, 5) == 0 and built_lib.dh_distance_work_size(5, 32768) == 0
    assert built_lib.dh_distance_work_size(128, 10) == 1280 + 20 and built_lib.dh_distance_work_size(129, 10) == 1290 + 40
    assert built_lib.dh_distance_work_size(32767, 32767) == 32767 * 32767 + 2 * 256 * 32767


def test_wrappers_refuse_before_any_library_call():
    from deephisto_amd import distance
    with pytest.raises(ValueError, match="mode must be"):
        distance.class_mask(np.zeros((4, 4), np.int64), [1], mode="edge")
    with pytest.raises(ValueError, match="outside 0"):
        distance.class_mask(np.zeros((4, 4), np.int64), [70])
    with pytest.raises(ValueError, match="bool or uint8"):
        distance.distance_transform(np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError, match="non-empty"):
        distance.distance_transform(np.zeros((4,), np.uint8))
    with pytest.raises(ValueError, match="32767"):
        distance.distance_transform(np.zeros((1, 32768), np.uint8))
    with pytest.raises(ValueError, match="radius_cells"):
        distance.dilate(np.zeros((4, 4), np.uint8), -1)
    with pytest.raises(ValueError, match="ascending"):
        distance.margin_bands(np.zeros((4, 4), np.int64), [1], [5, 5], 16)
    with pytest.raises(ValueError, match="tolerance_px"):
        distance.tolerant_truth(np.zeros((4, 4), np.int32), -1, 16)


def test_new_names_are_exported_beside_their_siblings():
    from deephisto_amd import distance
    from deephisto_amd.examples import predict_full_patched as pfp
    for name in ("class_mask", "distance_transform", "signed_distance", "dilate", "erode", "open_", "close", "margin_bands",
                 "band_composition", "surface_distances", "tolerant_score", "SurfaceDistance", "save_distance_report"):
        assert getattr(pfp, name) is getattr(distance, name), name


# ---- 4. CLI flags -------------------------------------------------------------------------------------------------------------------
BASE = ["--synthetic", "600", "600", "--weights", ""]


def _anno_file(tmp_path):
    import json
    from deephisto_amd.scoring import synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    path = tmp_path / "anno.json"
    path.write_text(json.dumps(synthetic_annotation(600, 600, 3, 16, list(KNOWN_COLORS), seed=1)))
    return str(path)


@pytest.mark.parametrize("extra,msg", [
    (["--score_tolerance", "32"], "--score_tolerance needs --anno"),
    (["--surface"], "--surface needs --anno"),
    (["--margin", "XYZ:100"], "--margin"),
    (["--margin", "TUM"], "--margin"),
    (["--margin", "TUM:"], "--margin"),
    (["--margin", "TUM:abc"], "--margin"),
    (["--margin", "TUM:100,50"], "ascend"),
    (["--margin", "TUM:0,0,50"], "ascend"),
    (["--margin", "TUM:0"], "--margin"),
    (["--margin", "TUM:-20"], "--margin"),
    (["--distance_json", "d.json"], "--distance_json needs"),
    (["--margin", "TUM:100", "--clusters", "4"], "--clusters"),
])
def test_cli_refuses_bad_distance_flags(built_lib, capsys, extra, msg):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(BASE + extra)
    with pytest.raises(SystemExit) as e:
        _check_args(ap, args)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_refuses_a_negative_tolerance(built_lib, capsys, tmp_path):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(BASE + ["--anno", _anno_file(tmp_path), "--score_tolerance", "-4"])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert "--score_tolerance" in capsys.readouterr().err


def test_cli_takes_the_distance_flags(built_lib, tmp_path):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(BASE + ["--anno", _anno_file(tmp_path), "--margin", "TUM:-200,0,100,500", "--score_tolerance", "32", "--surface",
                                 "--distance_json", str(tmp_path / "d.json"), "--min_region", "9"])
    _check_args(ap, args)
    assert args.margin_spec == ("TUM", [-200, 0, 100, 500]) and args.score_tolerance == 32 and args.surface
    args = ap.parse_args(BASE + ["--margin", "LP:64"])
    _check_args(ap, args)
    assert args.margin_spec == ("LP", [-64, 0, 64])
    plain = ap.parse_args(BASE)
    _check_args(ap, plain)
    assert plain.margin_spec is None and plain.score_tolerance is None and not plain.surface and plain.distance_json is None
