"""GPU: KNNClassifier and similar_tiles (deephisto_amd/neighbours.py) on the blobs of cluster_ref.

On `cluster_ref.blobs()` (1030 x 64, four blobs of 400, 310, 200 and 120 rows) every row's nine nearest rows lie in its own blob,
by a margin no float32 rounding touches (float64, on the CPU: the worst 9th own-blob distance is 124 against a nearest foreign
distance of 2870; after normalisation 0.065 against 1.35).  So a k-NN vote with k <= 9 must reproduce the blobs exactly."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cluster_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(dev):
    from deephisto_amd.neighbours import KNNClassifier
    x, which, _ = cr.blobs()
    xd = torch.from_numpy(x).to(dev)
    knn = KNNClassifier(4, k=5).fit(xd[::2], which[::2].astype(np.int32))
    return dict(x=x, which=which, xd=xd, knn=knn)


def _slide(features, cols=40, P=32, S=16, **kw):
    """A SlideEmbeddings whose tile i sits at (S * (i // cols), S * (i % cols))."""
    from deephisto_amd.embeddings import SlideEmbeddings
    n = len(features)
    i = np.arange(n)
    origins = np.stack([S * (i // cols), S * (i % cols)], axis=1).astype(np.int32)
    return SlideEmbeddings(features, origins, i, patch_size=P, stride=S, h=int(origins[:, 0].max()) + P, w=S * (cols - 1) + P,
                           n_unique=n, **kw)


def test_fit_on_every_other_row_predicts_the_rest(dev, case):
    knn, which = case["knn"], case["which"]
    assert knn.bank.shape == (515, 64) and knn.labels.dtype == torch.int32 and knn.counts.dtype == np.int64
    assert knn.counts.tolist() == np.bincount(which[::2], minlength=4).tolist() and knn.counts.sum() == 515
    held = case["xd"][1::2]
    pred = knn.predict(held)
    assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), which[1::2])
    votes = knn.votes(held)
    assert votes.dtype == torch.int32 and tuple(votes.shape) == (515, 4)
    assert np.array_equal(votes.cpu().numpy(), 5 * np.eye(4, dtype=np.int32)[which[1::2]]), "all five neighbours are of the own blob"
    index, dist = knn.neighbours(held)
    assert tuple(index.shape) == (515, 5) and np.array_equal(knn.labels.cpu().numpy()[index.cpu().numpy()], np.repeat(which[1::2, None], 5, 1))
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()) and float(dist.max()) < 0.2
    raw = type(knn)(4, k=9, normalize=False).fit(case["xd"][::2], which[::2])      # unnormalised rows, labels as int64
    assert np.array_equal(raw.predict(held).cpu().numpy(), which[1::2]) and float(raw.neighbours(held)[1].max()) < 400
    unlabelled = which.astype(np.int32).copy()
    unlabelled[1::2] = -1                                                           # the same bank from all rows, half unlabelled
    unlabelled[0] = 7                                                               # a label past the classes does not enter either
    same = type(knn)(4, k=5).fit(case["xd"], unlabelled)
    assert torch.equal(same.bank, knn.bank[1:]) and torch.equal(same.labels, knn.labels[1:])
    both = type(knn)(4, k=5).fit([case["xd"][:300], _slide(case["xd"][300:])], [unlabelled[:300], unlabelled[300:]])
    assert torch.equal(both.bank, same.bank) and torch.equal(both.labels, same.labels)
    with pytest.raises(ValueError, match="labels for"):
        type(knn)(4).fit(case["xd"], unlabelled[:-1])
    with pytest.raises(ValueError, match="columns"):
        knn.predict(torch.zeros((3, 128), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="no bank"):
        type(knn)(4).predict(held)


def test_leave_one_out_is_perfect_on_the_blobs(case):
    acc, confusion = case["knn"].leave_one_out()
    assert acc == 1.0 and confusion.dtype == np.int64
    assert np.array_equal(confusion, np.diag(case["knn"].counts))
    far = type(case["knn"])(4, k=64).fit(case["xd"][::2], case["which"][::2])
    with pytest.raises(ValueError, match="k must be in"):
        far.leave_one_out()


def test_predict_map_is_the_plurality_of_the_predicted_labels(dev, case):
    from deephisto_amd import tiles
    from deephisto_amd.embeddings import SlideEmbeddings
    from deephisto_amd.neighbours import KNNClassifier
    h, w, P, S, d = 160, 128, 32, 16, 16
    grid, n_unique = tiles.tile_grid(h, w, P, S, 1)
    grid = grid[:n_unique]
    rng = np.random.default_rng(8)
    keep = ~((grid[:, 0] < 64) & (grid[:, 1] < 48)) & (rng.random(n_unique) < 0.8)     # a corner gone whole, gaps elsewhere
    tile_index = np.flatnonzero(keep)
    origins, n = grid[tile_index], len(tile_index)
    rows = 1 + 2 * rng.permutation(515)[:n]                                            # held-out rows, blobs mixed over the grid
    emb = SlideEmbeddings(case["xd"][rows].contiguous(), origins, tile_index, patch_size=P, stride=S, h=h, w=w)
    labels = case["which"][rows]
    for fill in (-1, 2):
        got = case["knn"].predict_map(emb, d, fill_class=fill)
        want = cr.cluster_map_ref(origins, labels, 4, P, d, h, w, fill)
        assert got.dtype == torch.int64 and tuple(got.shape) == (h // d, w // d) and np.array_equal(got.cpu().numpy(), want)
        assert (want[:3, :2] == fill).all() and len(np.unique(want)) >= 3
    # tiles without a neighbour (NaN rows, unnormalised: a normalised NaN row is a zero row) vote for nothing
    feat = case["xd"][rows].clone()
    feat[torch.from_numpy(origins[:, 1] >= 96).to(dev)] = float("nan")
    lost = np.where(origins[:, 1] >= 96, -1, labels)
    raw = KNNClassifier(4, k=5, normalize=False).fit(case["xd"][::2], case["which"][::2])
    emb_nan = SlideEmbeddings(feat, origins, tile_index, patch_size=P, stride=S, h=h, w=w)
    assert np.array_equal(raw.predict(emb_nan).cpu().numpy(), lost)
    want = cr.cluster_map_ref(origins, lost, 4, P, d, h, w, -1)
    assert np.array_equal(raw.predict_map(emb_nan, d).cpu().numpy(), want) and (want[:, 7] == -1).all()


def test_similar_tiles_stay_in_the_blob(dev, case):
    from deephisto_amd.neighbours import similar_tiles
    which, emb = case["which"], _slide(case["xd"])
    for row in (0, 517, 1029, int(np.flatnonzero(which == 3)[0])):
        res = similar_tiles(emb, row)
        assert res["rows"].dtype == np.int32 and res["rows"].shape == (16,) and res["origins"].shape == (16, 2)
        assert res["dist"].dtype == np.float32 and np.all(np.diff(res["dist"]) >= 0) and res["dist"][-1] < 0.2
        assert row not in res["rows"] and len(set(res["rows"].tolist())) == 16 and np.all(which[res["rows"]] == which[row])
        assert np.array_equal(res["origins"], emb.origins[res["rows"]]) and res["query_row"] == row
        with_self = similar_tiles(emb, row, exclude_self=False)
        assert with_self["rows"][0] == row and with_self["dist"][0] == 0.0
        assert np.array_equal(with_self["rows"][1:], res["rows"][:15])
    y, x = emb.origins[517]
    by_pixel = similar_tiles(emb, (int(y) + 5, int(x) + 5), k=5)         # the first tile whose footprint holds the pixel
    first = similar_tiles(emb, by_pixel["query_row"], k=5)
    assert by_pixel["query_row"] == 517 - 41 and np.array_equal(by_pixel["rows"], first["rows"])
    other = _slide(case["xd"][::2])                                      # a search across slides keeps every row of the bank
    across = similar_tiles(emb, 4, k=8, bank=other)
    assert across["rows"][0] == 2 and across["dist"][0] == 0.0 and np.all(which[::2][across["rows"]] == which[4])
    assert np.array_equal(across["origins"], other.origins[across["rows"]])
    with pytest.raises(ValueError, match="k must be in"):
        similar_tiles(emb, 0, k=64)
    with pytest.raises(ValueError, match="covers"):
        similar_tiles(emb, (10 ** 6, 0))
    with pytest.raises(ValueError, match="columns"):
        similar_tiles(emb, 0, bank=_slide(torch.zeros((4, 128), dtype=torch.float32, device=dev)))


def test_save_and_load_reproduce_predict(dev, case, tmp_path):
    from deephisto_amd.neighbours import KNNClassifier
    knn = case["knn"]
    knn.save(tmp_path / "bank.npz")
    back = KNNClassifier.load(tmp_path / "bank.npz", device=dev)
    assert torch.equal(back.bank, knn.bank) and torch.equal(back.labels, knn.labels) and np.array_equal(back.counts, knn.counts)
    a, b = knn.neighbours(case["xd"]), back.neighbours(case["xd"])
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1].cpu().numpy().view(np.uint32), b[1].cpu().numpy().view(np.uint32))
    assert torch.equal(knn.predict(case["xd"]), back.predict(case["xd"])) and torch.equal(knn.votes(case["xd"]), back.votes(case["xd"]))
    on_cpu = KNNClassifier.load(tmp_path / "bank.npz")                    # a bank loaded to the host follows the queries' device
    assert torch.equal(on_cpu.predict(case["xd"]), knn.predict(case["xd"]))


def test_one_ranks_share_is_refused(dev, case):
    from deephisto_amd.neighbours import KNNClassifier, similar_tiles
    share = _slide(case["xd"][:100], row_range=(0, 100))
    with pytest.raises(ValueError, match="one rank's rows only"):
        KNNClassifier(4).fit(share, case["which"][:100])
    with pytest.raises(ValueError, match="one rank's rows only"):
        case["knn"].predict(share)
    with pytest.raises(ValueError, match="one rank's rows only"):
        case["knn"].predict_map(share)
    with pytest.raises(ValueError, match="one rank's rows only"):
        similar_tiles(share, 0)
    with pytest.raises(ValueError, match="one rank's rows only"):
        similar_tiles(_slide(case["xd"][:100]), 0, bank=share)
