"""GPU: `dh_class_mask`, `dh_distance_transform` and the Python layer of deephisto_amd/distance.py against
the NumPy restatements of tests/test_distance_host.py.  Everything is bit for bit: no tolerance anywhere."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_distance_host import (INT32_MAX, bands_of_signed_np, composition_np, confusion_np, corner_masks, edt_bruteforce,  # noqa: E402
                                edt_np, holed_blob_map, lattice_mask, mask_np, signed_np, surface_np, symmetric_pair,
                                tiled_blob_map, tolerant_truth_np)
from test_regions_host import blob_map  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = (1000, 2049)
MASK_SHAPES = [(1, 1), (1, 4097), (4097, 1), (37, 53), (65, 129), BIG]
SMALL_SHAPES = [(1, 1), (37, 53), (65, 129), (64, 64)]            # at most 129 wide: edt_bruteforce is the reference
CLASS_SETS = [([2], False), ([0, 3, 4], False), ([63], False), ([], True)]   # one class, several, class 63, "-1 only"


@pytest.fixture(scope="module")
def dist(built_lib):
    from deephisto_amd import distance
    assert torch.cuda.is_available()
    return distance


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def big_case():
    """The two masks of the largest canvas with a restatement, and `edt_np` of each, computed once: a jittered lattice (a feature
    within 41 cells of every cell, asserted by the window) and the boundaries of a blob map."""
    lattice = lattice_mask(BIG, 5)
    blobs = mask_np(tiled_blob_map(BIG, 6), range(5), mode=1)
    return dict(lattice=(lattice, edt_np(lattice, window=48)), blobs=(blobs, edt_np(blobs)))


# ---- dh_class_mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_class_mask_equals_the_restatement(dist, shape):
    m = holed_blob_map(shape, seed=shape[0] + shape[1])
    dev = _dev(m)
    for classes, incl in CLASS_SETS:
        for mode, code in dist.MODES.items():
            got = dist.class_mask(dev, classes, incl, mode)
            assert got.dtype == torch.uint8 and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), mask_np(m, classes, incl, code)), (classes, incl, mode)


def test_class_mask_refuses_a_class_out_of_range(dist):
    from deephisto_amd._lib import DeephistoHipError
    m = np.zeros((5, 7), np.int64)
    for bad in (64, -2):
        m[3, 4] = bad
        with pytest.raises(DeephistoHipError, match="outside"):
            dist.class_mask(m, [0])
    m[3, 4] = 63
    assert int(dist.class_mask(m, [63]).sum()) == 1


# ---- dh_distance_transform ---------------------------------------------------------------------------------------------------
def _check(dist, mask, want):
    d2, near = dist.distance_transform(_dev(mask), return_nearest=True)
    assert d2.dtype == torch.int32 and near.dtype == torch.int32
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(near.cpu().numpy(), want[1])


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_transform_of_the_corner_cases_equals_the_definition(dist, shape):
    """The empty and the full mask, a single feature in each corner (the farthest candidate: past the plain scan, through every
    block of the row) and in the centre, and the symmetric pair, whose ties hold the smallest-index rule."""
    rng = np.random.default_rng(shape[1])
    masks = dict(corner_masks(shape), pair=symmetric_pair(shape), sparse=(rng.random(shape) < 1 / 500).astype(np.uint8),
                 dense=(rng.random(shape) < 0.5).astype(np.uint8))
    for name, mask in masks.items():
        want = edt_bruteforce(mask)
        if name == "empty":
            assert (want[0] == INT32_MAX).all() and (want[1] == -1).all()
        d2, near = dist.distance_transform(_dev(mask), return_nearest=True)
        assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(near.cpu().numpy(), want[1]), name


@pytest.mark.parametrize("shape", [(1, 4097), (4097, 1), (128, 256), (2, 32767)])
def test_transform_of_the_long_and_the_tiled_canvases(dist, shape):
    """One row (no column pass to speak of), one column (no row pass), a canvas on every tile multiple, and the widest row the
    entry takes (its LDS row is the largest)."""
    rng = np.random.default_rng(shape[0])
    sparse = (rng.random(shape) < 1 / 700).astype(np.uint8)
    sparse[0, 0] = 1
    for mask in (sparse, lattice_mask(shape, 9)):
        _check(dist, mask, edt_np(mask))
    ends = np.zeros(shape, np.uint8)
    ends[-1, -1] = 1                                              # the far corner alone: closed form
    d2, near = dist.distance_transform(_dev(ends), return_nearest=True)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    assert np.array_equal(d2.cpu().numpy(), (shape[0] - 1 - y) ** 2 + (shape[1] - 1 - x) ** 2) and bool((near == shape[0] * shape[1] - 1).all())


@pytest.mark.parametrize("name", ["lattice", "blobs"])
def test_transform_of_the_largest_canvas_with_a_restatement(dist, big_case, name):
    mask, want = big_case[name]
    _check(dist, mask, want)


def test_the_same_bits_whatever_the_launch(dist, big_case):
    """Twice, on another stream, without the index map, and transposed: d2 transposes exactly, the nearest cell wherever the
    restatement says the minimum is attained by one cell only."""
    mask, want = big_case["lattice"]
    dev = _dev(mask)
    first = dist.distance_transform(dev, return_nearest=True)
    again = dist.distance_transform(dev, return_nearest=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = dist.distance_transform(dev, return_nearest=True)
        bare = dist.distance_transform(dev)                       # nearest = NULL
    side.synchronize()
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1]) and torch.equal(first[0], bare)
    t_d2, t_near = dist.distance_transform(dev.t().contiguous(), return_nearest=True)
    assert torch.equal(t_d2.t(), first[0])
    # unique minimum: the restatement of the transposed mask names the same cell
    dh, dw = mask.shape
    n_t = edt_np(mask.T, window=48)[1].astype(np.int64)
    back = ((n_t % dh) * dw + n_t // dh).T                        # (x', y') of the transposed canvas as an index of this one
    unique = back == want[1]
    assert unique.mean() > 0.9
    got_back = (t_near.cpu().numpy().astype(np.int64) % dh) * dw + t_near.cpu().numpy().astype(np.int64) // dh
    assert np.array_equal(got_back.T[unique], want[1][unique])


def test_a_whole_slide_canvas_with_one_corner_feature(dist):
    """3 125 x 3 125, the feature in the bottom right corner: every row scans to its far end.  d2 in closed form."""
    n = 3125
    mask = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    mask[n - 1, n - 1] = 1
    d2, near = dist.distance_transform(mask, return_nearest=True)
    r = (n - 1 - torch.arange(n, device="cuda", dtype=torch.int32)) ** 2
    assert torch.equal(d2, r[:, None] + r[None, :]) and bool((near == n * n - 1).all())


def test_a_whole_slide_canvas_of_blobs_against_scipy(dist):
    ndimage = pytest.importorskip("scipy.ndimage")
    n = 3125
    mask = mask_np(tiled_blob_map((n, n), 8, tile=(625, 625)), range(5), mode=1)
    iy, ix = ndimage.distance_transform_edt(mask == 0, return_distances=False, return_indices=True)
    y, x = np.mgrid[0:n, 0:n]
    want = (iy.astype(np.int64) - y) ** 2 + (ix.astype(np.int64) - x) ** 2
    assert np.array_equal(dist.distance_transform(_dev(mask)).cpu().numpy(), want)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(37, 53), (300, 517)])
def maps(request):
    """(prediction, truth) of one shape: a blob map with holes, and the same blobs shifted and partly relabelled as the truth."""
    shape = request.param
    pred = holed_blob_map(shape, seed=shape[0])
    pred[pred == 63] = 1
    truth = np.roll(blob_map(shape[0], shape[1], shape[0]), (2, -3), axis=(0, 1)).astype(np.int32)
    truth[truth == 4] = 0
    return pred, truth


@pytest.mark.parametrize("downscale", [1, 16])
def test_signed_distance_and_margin_bands(dist, maps, downscale):
    pred, _ = maps
    dev = _dev(pred)
    for classes, incl in (([1], False), ([0, 2], False), ([], True), ([7], False)):
        got = dist.signed_distance(dev, classes, incl)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), signed_np(pred, classes, incl)), (classes, incl)
    signed = signed_np(pred, [1, 3])
    for edges in ([-500, 0, 500], [-32, -5, 0, 16, 33, 80], [3, 4]):
        bands = dist.margin_bands(dev, [1, 3], edges, downscale)
        want = bands_of_signed_np(signed, edges, downscale)
        assert bands.dtype == torch.int64 and np.array_equal(bands.cpu().numpy(), want), edges
        comp = dist.band_composition(dev, bands, 5, len(edges) - 1)
        assert comp.dtype == torch.int64 and np.array_equal(comp.numpy(), composition_np(pred, want, 5, len(edges) - 1)), edges
    assert bool((dist.margin_bands(dev, [7], [-500, 0, 500], downscale) == -1).all())          # an empty set has no border


def test_dilate_and_erode_are_exact_discs(dist, maps):
    pred, _ = maps
    mask = (pred == 1) | (pred == 2)
    dev = _dev(mask)
    d_out, d_in = edt_np(mask)[0].astype(np.int64), edt_np(~mask)[0].astype(np.int64)
    for r in (0, 1, 3, 7):
        assert np.array_equal(dist.dilate(dev, r).cpu().numpy(), (d_out <= r * r).astype(np.uint8)), r
        assert np.array_equal(dist.erode(dev, r).cpu().numpy(), (d_in > r * r).astype(np.uint8)), r
    grown = d_out <= 9
    assert np.array_equal(dist.close(dev, 3).cpu().numpy(), (edt_np(~grown)[0].astype(np.int64) > 9).astype(np.uint8))
    shrunk = d_in > 9
    want = (edt_np(shrunk)[0].astype(np.int64) <= 9) if shrunk.any() else np.zeros(mask.shape, bool)
    assert np.array_equal(dist.open_(dev, 3).cpu().numpy(), want.astype(np.uint8))


@pytest.mark.parametrize("downscale", [1, 16])
def test_tolerant_score(dist, maps, downscale):
    from deephisto_amd import scoring
    pred, truth = maps
    p, t = _dev(pred), _dev(truth)
    labels = ["a", "b", "c", "d", "e"]
    plain = scoring.confusion(p, t, 5)
    zero = dist.tolerant_score(p, t, labels, 0, downscale)
    assert np.array_equal(zero.confusion, plain.numpy()) and zero.n_cells == pred.size
    for tol in (1, 16, 17, 40):
        cut = tolerant_truth_np(truth, tol, downscale)
        assert np.array_equal(dist.tolerant_truth(t, tol, downscale).cpu().numpy(), cut), tol
        got = dist.tolerant_score(p, t, labels, tol, downscale)
        assert np.array_equal(got.confusion, confusion_np(pred, cut, 5)) and got.n_cells == pred.size, tol
    if downscale == 1:                                            # a tolerance of one pixel drops exactly the label-change cells
        assert np.array_equal(dist.tolerant_truth(t, 1, 1).cpu().numpy() != truth, (mask_np(truth, [], mode=2) != 0) & (truth != -1))
    assert np.array_equal(t.cpu().numpy(), truth)                # the input is not modified


@pytest.mark.parametrize("downscale", [1, 16])
def test_surface_distances(dist, maps, downscale):
    pred, truth = maps
    p, t = _dev(pred), _dev(truth)
    for cls in (0, 1, 2, 3, 4, 9):
        got, want = dist.surface_distances(p, t, cls, downscale), surface_np(pred, truth, cls, downscale)
        assert (got.n_pred, got.n_truth) == (want["n_pred"], want["n_truth"]), cls
        for key in ("hausdorff", "hd95", "assd"):
            g, w = getattr(got, key), want[key]
            assert g == w or (math.isnan(g) and math.isnan(w)), (cls, key)
    assert math.isnan(dist.surface_distances(p, t, 9).assd) and dist.surface_distances(p, t, 4).n_truth == 0
    same = dist.surface_distances(p, p, 1, downscale)
    assert (same.hausdorff, same.hd95, same.assd) == (0.0, 0.0, 0.0) and same.n_pred == same.n_truth > 0
