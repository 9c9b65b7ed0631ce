"""Host side of deephisto_amd/clustering.py: the k-means++ draw, the canonical numbering, the KMeans file
and the argument checks, and the float64 reference of the GPU tests meeting its own margin condition.  No GPU."""
import sys
import zipfile
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cluster_ref as cr  # noqa: E402


def test_draw_index_never_draws_a_row_of_weight_zero():
    from deephisto_amd.clustering import draw_index
    w = np.array([0, 0, 3, 0, 1, 0, 0, 4, 0], np.float32)
    drawn = {draw_index(w, u) for u in np.linspace(0.0, 1.0, 4001, endpoint=False)}
    assert drawn == {2, 4, 7}
    assert draw_index(w, 0.0) == 2 and draw_index(w, 3 / 8 - 1e-9) == 2 and draw_index(w, 3 / 8) == 4 and draw_index(w, 0.5) == 7
    freq = np.bincount([draw_index(w, u) for u in np.random.default_rng(0).random(20000)], minlength=9) / 20000
    assert np.allclose(freq, w / w.sum(), atol=0.02)


def test_draw_index_stays_in_range_at_both_ends():
    from deephisto_amd.clustering import draw_index
    w = np.array([0.25, 0, 1e-30, 7, 0, 0], np.float32)
    assert draw_index(w, 0.0) == 0
    assert draw_index(w, np.nextafter(1.0, 0.0)) == 3
    assert draw_index(w, 1.0) == 3                     # a u the generator never gives: still the last row that weighs anything
    assert draw_index(np.array([5.0], np.float32), 0.999) == 0
    big = np.full(1000, 3e38, np.float32)              # float32 sums would overflow; the cumulative sums are float64
    assert draw_index(big, 0.5) == 500


def test_draw_index_falls_back_to_row_zero_and_ignores_what_is_not_finite():
    from deephisto_amd.clustering import draw_index, farthest_index
    assert draw_index(np.zeros(7, np.float32), 0.73) == 0
    w = np.array([np.inf, 0, np.nan, 2, np.inf], np.float32)   # a row of NaN has distance +inf and label -1
    assert {draw_index(w, u) for u in (0.0, 0.3, 0.999)} == {3}
    assert farthest_index(w) == 3
    assert farthest_index(np.array([1, 9, 2, 9], np.float32)) == 1   # the first maximum
    with pytest.raises(ValueError):
        draw_index(np.zeros(0, np.float32), 0.5)


def test_canonical_order_by_size_then_old_number():
    from deephisto_amd.clustering import canonical_order
    assert canonical_order([5, 9, 1]).tolist() == [1, 0, 2]
    assert canonical_order([4, 7, 4, 7, 0]).tolist() == [1, 3, 0, 2, 4]
    assert canonical_order([3, 3, 3]).tolist() == [0, 1, 2]
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = rng.integers(0, 6, rng.integers(1, 65))
        assert canonical_order(c).tolist() == cr.canonical_ref(c).tolist()


def test_kmeans_file_round_trip_without_pickle(tmp_path):
    from deephisto_amd.clustering import KMeans
    km = KMeans(3, init="maximin", seed=11, max_iter=7, normalize=False)
    km.centres_ = torch.from_numpy(np.random.default_rng(0).standard_normal((3, 64)).astype(np.float32))
    km.counts_ = np.array([9, 5, 2], np.int64)
    km.inertia_, km.n_iter_, km.converged_ = 12.5, 4, True
    path = tmp_path / "codebook.npz"
    km.save(path)
    with zipfile.ZipFile(path) as z:
        assert sorted(z.namelist()) == ["centres.npy", "counts.npy", "meta.npy"]
    with np.load(path, allow_pickle=False) as z:       # raises on a pickled member
        assert all(z[k].dtype != object for k in z.files)
    back = KMeans.load(path)
    assert torch.equal(back.centres_, km.centres_) and back.counts_.tolist() == [9, 5, 2]
    assert (back.n_clusters, back.init, back.seed, back.max_iter, back.normalize) == (3, "maximin", 11, 7, False)
    assert (back.inertia_, back.n_iter_, back.converged_) == (12.5, 4, True)
    with pytest.raises(ValueError, match="no centres"):
        KMeans(2).save(tmp_path / "empty.npz")
    np.savez(tmp_path / "other.npz", meta=np.array('{"format": "something else"}'))
    with pytest.raises(ValueError, match="not a KMeans file"):
        KMeans.load(tmp_path / "other.npz")


def test_kmeans_argument_checks():
    from deephisto_amd.clustering import KMeans, cluster_description
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="n_clusters"):
            KMeans(k)
    with pytest.raises(ValueError, match="init"):
        KMeans(3, init="random")
    with pytest.raises(ValueError, match="initial centres"):
        KMeans(3, init=np.zeros((4, 64), np.float32))
    with pytest.raises(ValueError, match="max_iter"):
        KMeans(3, max_iter=-1)
    with pytest.raises(ValueError, match="no centres"):
        KMeans(3).predict(torch.zeros((2, 64)))
    assert KMeans(64).n_clusters == 64 and KMeans(1, init=np.zeros((1, 64), np.float32)).init == "explicit"
    dsc = cluster_description(64)
    assert [a.label for a in dsc.anno_classes[:2]] == ["cluster_0", "cluster_1"] and [a.id for a in dsc.anno_classes] == list(range(64))
    assert len({tuple(a.color) for a in dsc.anno_classes}) == 64, "64 distinct colours"
    assert [a.color for a in cluster_description(5).anno_classes] == [a.color for a in dsc.anno_classes[:5]]


def test_one_ranks_share_is_refused_by_name():
    from deephisto_amd.clustering import KMeans
    from deephisto_amd.embeddings import SlideEmbeddings
    emb = SlideEmbeddings(torch.zeros((4, 64)), np.zeros((4, 2)), np.arange(4), patch_size=32, stride=32, h=64, w=64, row_range=(0, 4))
    with pytest.raises(ValueError, match="gather=False"):
        KMeans(2).fit(emb)
    with pytest.raises(ValueError, match="gather=False"):
        KMeans(2).fit([emb])


def test_the_reference_meets_its_margin_condition_with_no_row_excluded():
    """What the GPU tests of the fit rest on: on the blobs, from the initial centres they use, every row's second-nearest float64
    distance exceeds its nearest by more than ((1 + g) / (1 - g))^2 at every iteration (lloyd_ref asserts it), the first
    assignment cuts a blob, and the run ends on the blobs themselves."""
    x, which, centres = cr.blobs()
    assert x.shape == (1030, 64) and x.dtype == np.float32
    init = cr.blob_init(centres)
    first = cr.assign_ref(x, init).argmin(1)
    assert np.bincount(first).tolist() != list(cr.BLOB_SIZES), "the first assignment is not yet the result"
    ref = cr.lloyd_ref(x, init)
    assert ref["converged"] and ref["n_iter"] == 2 and ref["counts"].tolist() == list(cr.BLOB_SIZES)
    assert np.array_equal(ref["labels"], which)        # sizes descend with the blob number, so canonical numbers are blob numbers
    twin = centres.copy()
    twin[3] = twin[1]                                  # the reseeding case: the top two distances are apart as well
    ref2 = cr.lloyd_ref(x, twin)
    assert ref2["converged"] and ref2["counts"].tolist() == list(cr.BLOB_SIZES)


def test_cluster_map_reference_on_a_hand_case():
    o = np.array([[0, 0], [0, 16], [16, 0]], np.int32)   # three 32 x 32 tiles on a 48 x 64 canvas, 16-pixel cells
    m = cr.cluster_map_ref(o, [2, 1, 1], 3, 32, 16, 48, 64, fill_class=-1)
    assert m.tolist() == [[2, 1, 1, -1], [1, 1, 1, -1], [1, 1, -1, -1]]
