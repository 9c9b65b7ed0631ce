"""GPU: dh_embed_assign, KMeans and cluster_map (deephisto_amd/clustering.py) against tests/helpers/cluster_ref.py.

The kernel sweep: D in {64, 512, 2048}, K in {1, 5, 16, 17, 64} (both instantiations at their border), n in {1, 31, 33, 65, 1025} (one
row, both sides of the 32-row tile, two tiles plus a row, past the 256-row tile of the K <= 16 instantiation), seeded normal rows
and centres, every row held to the float64 distances by the gate g = (D + 4) u.  Worst observed |dist - d64| / d64 on the MI355X:
see DESIGN.md section 4.18 (the test prints it per case)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cluster_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

DS, KS, NS = (64, 512, 2048), (1, 5, 16, 17, 64), (1, 31, 33, 65, 1025)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE: dict = {}


def _rows_of(D):
    """float32[1025, D] rows, the same for every test that asks (computed once and never written)."""
    if ("x", D) not in _CACHE:
        f = np.random.default_rng(2000 + D).standard_normal((max(NS), D)).astype(np.float32)
        f.setflags(write=False)
        _CACHE["x", D] = f
    return _CACHE["x", D]


def _centres_of(D, K):
    if ("c", D, K) not in _CACHE:
        c = np.random.default_rng(31 * D + K).standard_normal((K, D)).astype(np.float32)
        c.setflags(write=False)
        _CACHE["c", D, K] = c
    return _CACHE["c", D, K]


def _d64(D, K):
    """float64[1025, K] distances of the cached rows and centres: once per (D, K), sliced for every n."""
    if ("d", D, K) not in _CACHE:
        _CACHE["d", D, K] = cr.assign_ref(_rows_of(D), _centres_of(D, K))
    return _CACHE["d", D, K]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- the kernel against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_assign_against_float64(dev, D, K, n):
    from deephisto_amd.clustering import nearest_centres
    x, c = _t(_rows_of(D)[:n], dev), _t(_centres_of(D, K), dev)
    k0 = 0 if K != 5 else 7
    label = torch.full((n + 1,), -77, dtype=torch.int32, device=dev)
    dist = torch.full((n + 1,), -5.0, dtype=torch.float32, device=dev)
    lab, dst = nearest_centres(x, c, label[:n], dist[:n], k0=k0)
    worst = cr.check_assign(_d64(D, K)[:n], lab.cpu().numpy(), dst.cpu().numpy(), D, k0)
    print(f"assign D={D} K={K} n={n}: worst |dist - d64| / d64 = {worst:.2f} u (first-order bound {D + 2} u)")
    assert int(label[n]) == -77 and float(dist[n]) == -5.0, "the guard row behind n is untouched"
    assert float(dst.min()) >= 0.0
    lab2, dst2 = nearest_centres(x, c, k0=k0)
    assert torch.equal(lab2, lab) and np.array_equal(_bits(dst2), _bits(dst)), "a second launch gives the same bits"


# ---- exact cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (5, 16, 17, 64))
def test_exact_cases(dev, K):
    from deephisto_amd.clustering import nearest_centres
    D, n = 512, 67
    f, c = _rows_of(D)[:n].copy(), _centres_of(D, K).copy()
    f[9] = c[3]                      # bit-equal to centre 3
    c[4] = c[2]                      # centres 2 and 4 bit-equal: 4 never wins
    f[20] = c[4]                     # even for the row that sits on both
    f[40] = np.nan
    f[41, 5] = np.inf                # a row with one infinite element: every distance +inf
    lab, dst = nearest_centres(_t(f, dev), _t(c, dev))
    lab, dst = lab.cpu().numpy(), dst.cpu().numpy()
    assert lab[9] == 3 and dst[9] == 0.0 and not np.signbit(dst[9])
    assert lab[20] == 2 and dst[20] == 0.0
    assert not (lab == 4).any(), "the higher of two bit-equal centres never wins"
    assert lab[40] == -1 and dst[40] == np.inf, "a row of NaN gets (-1, +inf)"
    assert lab[41] == -1 and dst[41] == np.inf
    ok = np.ones(n, bool)
    ok[[40, 41]] = False
    cr.check_assign(cr.assign_ref(f[ok], c), lab[ok], dst[ok], D)
    # an all-zero row against an all-zero centre, alone and as the last of K
    z = torch.zeros((1, D), dtype=torch.float32, device=dev)
    lab0, dst0 = nearest_centres(z, z)
    assert int(lab0[0]) == 0 and float(dst0[0]) == 0.0
    cz = c.copy()
    cz[K - 1] = 0
    labz, dstz = nearest_centres(z, _t(cz, dev))
    assert int(labz[0]) == K - 1 and float(dstz[0]) == 0.0


def test_empty_launch_is_a_no_op(dev):
    from deephisto_amd.clustering import nearest_centres
    lab, dst = nearest_centres(torch.empty((0, 64), dtype=torch.float32, device=dev), torch.zeros((3, 64), dtype=torch.float32, device=dev))
    assert lab.shape == (0,) and dst.shape == (0,)


# ---- launch independence, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 5, 16, 17, 64))
@pytest.mark.parametrize("D", (64, 2048))
def test_launch_independence(dev, D, K):
    """Rows 5..40 alone, inside the full launch, and from a pointer shifted by one row: equal distance bits, equal labels."""
    from deephisto_amd.clustering import nearest_centres
    n = 300
    x, c = _t(_rows_of(D)[:n], dev), _t(_centres_of(D, K), dev)
    lab, dst = nearest_centres(x, c)
    lab_a, dst_a = nearest_centres(x[5:41], c)
    assert torch.equal(lab_a, lab[5:41]) and np.array_equal(_bits(dst_a), _bits(dst[5:41]))
    lab_s, dst_s = nearest_centres(x[1:], c)
    assert torch.equal(lab_s, lab[1:]) and np.array_equal(_bits(dst_s), _bits(dst[1:]))
    out_l, out_d = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    nearest_centres(x[1:], c, out_l[1:], out_d[1:])      # outputs shifted by one element as well
    assert torch.equal(out_l[1:], lab[1:]) and np.array_equal(_bits(out_d[1:]), _bits(dst[1:])) and int(out_l[0]) == 0


# ---- merge, bit for bit ------------------------------------------------------------------------------------------------------
def test_merge_in_passes(dev):
    """130 centres as 64 + 64 + 2 with k0 = 0, 64, 128 and merge = 0, 1, 1: the host's lexicographic minimum of three unmerged
    launches, and within the float64 gate over all 130."""
    from deephisto_amd.clustering import nearest_centres
    D, n = 512, 333
    f = _rows_of(D)[:n]
    c = np.random.default_rng(130).standard_normal((130, D)).astype(np.float32)
    c[100] = c[17]                                        # a tie across passes: the lower index, held from the first pass, stays
    c[129] = f[50]                                        # a row that only the last pass (the K <= 16 instantiation) sets to 0
    x, cd = _t(f, dev), _t(c, dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    dst = torch.empty(n, dtype=torch.float32, device=dev)
    parts = []
    for k0, k1 in ((0, 64), (64, 128), (128, 130)):
        nearest_centres(x, cd[k0:k1], lab, dst, k0=k0, merge=k0 > 0)
        pl, pd = nearest_centres(x, cd[k0:k1], k0=k0)
        parts.append((pd.cpu().numpy(), pl.cpu().numpy()))
    want_d, want_l = cr.lexmin([p[0] for p in parts], [p[1] for p in parts])
    assert np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(_bits(dst), want_d.view(np.uint32))
    assert not (want_l == 100).any() and want_l[50] == 129 and want_d[50] == 0.0
    cr.check_assign(cr.assign_ref(f, c), want_l, want_d, D)
    with pytest.raises(ValueError, match="merge"):
        nearest_centres(x, cd[:3], merge=True)


# ---- refusals by name ----------------------------------------------------------------------------------------------------------
def _raw(built_lib, dev, D=64, K=3, k0=0, feat="ok", centres="ok", label="ok", dist="ok", n=4):
    x = torch.zeros((n + 1, max(D, 64)), dtype=torch.float32, device=dev)
    c = torch.zeros((64, max(D, 64)), dtype=torch.float32, device=dev)
    lb = torch.zeros(n, dtype=torch.int32, device=dev)
    ds = torch.zeros(n, dtype=torch.float32, device=dev)
    ptr = {"ok": lambda t: t.data_ptr(), "null": lambda t: None, "odd": lambda t: t.data_ptr() + 4}
    rc = built_lib.dh_embed_assign(ptr[feat](x), n, D, ptr[centres](c), K, k0, 0, ptr[label](lb), ptr[dist](ds), None)
    torch.cuda.synchronize()
    assert not lb.any() and not ds.any(), "a refused call launches nothing"
    return rc, built_lib.dh_last_error().decode()


def test_refuses_D_96(built_lib, dev):
    rc, msg = _raw(built_lib, dev, D=96)
    assert rc == -22 and "dh_embed_assign" in msg and "D = 96" in msg


def test_refuses_K_0(built_lib, dev):
    rc, msg = _raw(built_lib, dev, K=0)
    assert rc == -22 and "dh_embed_assign" in msg and "K = 0" in msg


def test_refuses_K_65(built_lib, dev):
    rc, msg = _raw(built_lib, dev, K=65)
    assert rc == -22 and "dh_embed_assign" in msg and "K = 65" in msg


def test_refuses_negative_k0(built_lib, dev):
    rc, msg = _raw(built_lib, dev, k0=-1)
    assert rc == -22 and "dh_embed_assign" in msg and "k0 = -1" in msg


@pytest.mark.parametrize("which", ("feat", "centres", "label", "dist"))
def test_refuses_a_null_pointer(built_lib, dev, which):
    rc, msg = _raw(built_lib, dev, **{which: "null"})
    assert rc == -22 and "dh_embed_assign" in msg and "null" in msg


@pytest.mark.parametrize("which", ("feat", "centres"))
def test_refuses_a_misaligned_pointer(built_lib, dev, which):
    rc, msg = _raw(built_lib, dev, **{which: "odd"})
    assert rc == -22 and "dh_embed_assign" in msg and "aligned" in msg


# ---- k-means end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_case(dev):
    x, which, centres = cr.blobs()
    init = cr.blob_init(centres)
    return dict(x=x, which=which, centres=centres, init=init, ref=cr.lloyd_ref(x, init), xd=_t(x, dev))


def test_fit_equals_the_float64_lloyd(dev, blob_case):
    """normalize=False, so that the float64 reference reads the very float32 rows the kernels read."""
    from deephisto_amd.clustering import KMeans
    b, ref = blob_case, blob_case["ref"]
    km = KMeans(4, init=b["init"], normalize=False).fit(b["xd"])
    assert km.converged_ and km.n_iter_ == ref["n_iter"] == 2
    assert km.labels_.dtype == torch.int32 and np.array_equal(km.labels_.cpu().numpy(), ref["labels"]), "same partition, same numbering"
    assert km.counts_.dtype == np.int64 and km.counts_.tolist() == ref["counts"].tolist() == list(cr.BLOB_SIZES)
    x64, lab = b["x"].astype(np.float64), ref["labels"]
    m = int(ref["counts"].max())
    got = km.centres_.cpu().numpy().astype(np.float64)
    for k in range(4):
        mean_abs = np.abs(x64[lab == k]).mean(0)
        err = np.abs(got[k] - ref["centres"][k])
        print(f"centre {k}: worst error {np.max(err / mean_abs) / cr.U:.2f} u mean|x| (gate {m + 2} u)")
        assert np.all(err <= (m + 2) * cr.U * mean_abs)
    rel = abs(km.inertia_ - ref["inertia"]) / ref["inertia"]
    print(f"inertia: relative error {rel / cr.U:.2f} u (gate {64 + 4} u)")
    assert rel <= cr.gate(64)
    # the same bits twice; predict on the fitted rows gives the labels
    again = KMeans(4, init=b["init"], normalize=False).fit(b["xd"])
    assert np.array_equal(_bits(again.centres_), _bits(km.centres_)) and torch.equal(again.labels_, km.labels_)
    assert torch.equal(km.predict(b["xd"]), km.labels_)


@pytest.mark.parametrize("init", ("kmeans++", "maximin"))
def test_seedings_pick_distinct_rows_and_repeat(dev, blob_case, init):
    from deephisto_amd.clustering import KMeans
    b = blob_case
    before = b["xd"].clone()
    km = KMeans(4, init=init, seed=3).fit(b["xd"])                   # normalize=True
    assert torch.equal(b["xd"], before), "normalize=True leaves the caller's tensor unwritten"
    rows = km.seed_rows_
    assert len(rows) == 4 and len(set(rows)) == 4 and all(0 <= r < 1030 for r in rows)
    again = KMeans(4, init=init, seed=3).fit(b["xd"])
    assert again.seed_rows_ == rows
    assert np.array_equal(_bits(again.centres_), _bits(km.centres_)) and torch.equal(again.labels_, km.labels_)
    assert again.inertia_ == km.inertia_ and again.n_iter_ == km.n_iter_
    assert torch.equal(km.predict(b["xd"]), km.labels_), "converged or not, a fit ends on an assignment to the centres it returns"
    assert km.counts_.tolist() == sorted(km.counts_.tolist(), reverse=True) and int(km.counts_.sum()) == 1030
    assert np.bincount(km.labels_.cpu().numpy(), minlength=4).tolist() == km.counts_.tolist()
    if init == "maximin":   # one row per blob, whatever the order: the farthest row from k blobs' seeds lies in another blob
        assert sorted(b["which"][rows].tolist()) == [0, 1, 2, 3]
        assert km.converged_ and km.counts_.tolist() == list(cr.BLOB_SIZES) and np.array_equal(km.labels_.cpu().numpy(), b["which"])


def test_fit_of_a_list_equals_fit_of_the_concatenation(dev, blob_case):
    from deephisto_amd.clustering import KMeans
    from deephisto_amd.embeddings import SlideEmbeddings
    xd = blob_case["xd"]
    a = SlideEmbeddings(xd[:500].contiguous(), np.zeros((500, 2)), np.arange(500), patch_size=32, stride=32, h=4096, w=4096,
                        n_unique=500, n_padded=500)
    whole = KMeans(4, seed=1).fit(xd)
    parts = KMeans(4, seed=1).fit([a, xd[500:]])
    assert np.array_equal(_bits(parts.centres_), _bits(whole.centres_)) and torch.equal(parts.labels_, whole.labels_)
    assert parts.counts_.tolist() == whole.counts_.tolist() and parts.inertia_ == whole.inertia_
    assert torch.equal(KMeans(4, seed=1).fit(a).labels_, KMeans(4, seed=1).fit(xd[:500]).labels_), "a SlideEmbeddings is its features"


def test_twin_initial_centres_reseed_the_empty_cluster(dev, blob_case):
    """Initial centres 1 and 3 bit-equal: the tie rule leaves cluster 3 empty, its centre becomes the row of largest distance, and
    the run equals the float64 restatement of that rule (which asserts that the two farthest rows are apart by the gate)."""
    from deephisto_amd.clustering import KMeans, nearest_centres
    b = blob_case
    twin = b["centres"].copy()
    twin[3] = twin[1]
    first, _ = nearest_centres(b["xd"], _t(twin, dev))
    assert not (first == 3).any() and int((first == 1).sum()) >= 310
    ref = cr.lloyd_ref(b["x"], twin)
    km = KMeans(4, init=twin, normalize=False).fit(b["xd"])
    assert km.converged_ and km.n_iter_ == ref["n_iter"]
    assert np.array_equal(km.labels_.cpu().numpy(), ref["labels"]) and km.counts_.tolist() == ref["counts"].tolist()
    assert np.allclose(km.centres_.cpu().numpy(), ref["centres"], rtol=0, atol=(400 + 2) * cr.U * np.abs(b["x"]).max())   # m = 400 rows


# ---- the cluster map, bit for bit against NumPy -----------------------------------------------------------------------------------
def test_cluster_map_equals_the_plurality_per_cell(dev):
    from deephisto_amd import tiles
    from deephisto_amd.clustering import cluster_description, cluster_map
    from deephisto_amd.embeddings import SlideEmbeddings
    from deephisto_amd.regions import extract_regions
    h, w, P, S, d, K = 160, 128, 32, 16, 16, 5
    grid, n_unique = tiles.tile_grid(h, w, P, S, 1)
    grid = grid[:n_unique]
    rng = np.random.default_rng(8)
    keep = ~((grid[:, 0] < 64) & (grid[:, 1] < 48)) & (rng.random(n_unique) < 0.8)     # a corner gone whole, gaps elsewhere
    tile_index = np.flatnonzero(keep)
    origins = grid[tile_index]
    n = len(tile_index)
    labels = rng.integers(0, K, n).astype(np.int32)
    labels[origins[:, 0] >= 112] = 3                       # a uniform band, so that regions of some size exist
    emb = SlideEmbeddings(torch.zeros((n, 64), dtype=torch.float32, device=dev), origins, tile_index, patch_size=P, stride=S, h=h, w=w)
    for fill in (-1, 2):
        want = cr.cluster_map_ref(origins, labels, K, P, d, h, w, fill)
        got = cluster_map(emb, _t(labels, dev), K, downscale=d, fill_class=fill)
        assert got.dtype == torch.int64 and tuple(got.shape) == (h // d, w // d)
        assert np.array_equal(got.cpu().numpy(), want)
        assert (want[:3, :2] == fill).all(), "cells only missing tiles cover"
    lost = labels.copy()
    lost[origins[:, 1] >= 96] = -1                         # tiles without a cluster vote for nothing
    want = cr.cluster_map_ref(origins, lost, K, P, d, h, w, -1)
    assert np.array_equal(cluster_map(emb, lost, K, downscale=d).cpu().numpy(), want) and (want[:, 7] == -1).all()
    got = cluster_map(emb, labels, K, downscale=d)
    want = cr.cluster_map_ref(origins, labels, K, P, d, h, w, -1)
    dsc = cluster_description(K)
    a, b = extract_regions(got, dsc, 1, d, device=dev), extract_regions(want, dsc, 1, d, device=dev)
    assert a.k == b.k and a.k > 1 and torch.equal(a.labels, b.labels) and torch.equal(a.class_map, b.class_map)
    assert a.regions.to_records(dsc, d, 1) == b.regions.to_records(dsc, d, 1) and sorted(a.polygons) == sorted(b.polygons)
    for rid, (outer, holes) in a.polygons.items():
        assert np.array_equal(outer, b.polygons[rid][0]) and len(holes) == len(b.polygons[rid][1])
        assert all(np.array_equal(x, y) for x, y in zip(holes, b.polygons[rid][1]))
    assert {r["class"] for r in a.regions.to_records(dsc, d, 1)} <= {f"cluster_{k}" for k in range(K)}
