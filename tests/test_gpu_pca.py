"""GPU: PCA, reduce and colour_map (deephisto_amd/pca.py) against tests/helpers/pca_ref.py.

The planted spectrum (n = 1030, past one chunk; D = 64 and 128): the device fit against the float64 PCA of the same float32 rows, the
eigenvalues by Weyl's bound ||E||_F and the components by the Davis-Kahan bound 2 ||E||_F / gap_j, E being the covariance error the
scatter kernel's element gate allows (pca_ref.pca_ref; tests/test_pca_host.py checks on the CPU how small these bounds are)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cluster_ref as cr  # noqa: E402
import pca_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _emb(features, origins, tile_index, h, w, P, S, **kw):
    from deephisto_amd.embeddings import SlideEmbeddings
    return SlideEmbeddings(features, origins, tile_index, patch_size=P, stride=S, h=h, w=w, **kw)


_PLANTED: dict = {}


def _planted(D, dev):
    if D not in _PLANTED:
        x, q = pr.planted(D=D)
        x.setflags(write=False)
        _PLANTED[D] = dict(x=x, q=q, ref=pr.pca_ref(x, 3), xd=_t(x, dev))
    return _PLANTED[D]


# ---- the planted spectrum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_fit_against_the_float64_pca(dev, D):
    from deephisto_amd.pca import PCA
    case = _planted(D, dev)
    ref = case["ref"]
    pca = PCA(3).fit(case["xd"])
    assert pca.n_samples_ == 1030 and pca.mean_.is_cuda and pca.components_.is_cuda
    assert pca.mean_.dtype == torch.float32 and tuple(pca.components_.shape) == (3, D) and pca.components_.dtype == torch.float32
    assert np.array_equal(_bits(pca.mean_), _bits(ref["mean32"])), "the mean is the contract's: class_sums' order, one rounding"
    lam = pca.explained_variance_
    assert lam.dtype == np.float64 and lam.shape == (3,) and np.all(np.diff(lam) < 0)
    err = np.abs(lam - ref["lam"][:3])
    print(f"D = {D}: |lambda - lambda64| = {err} (Weyl bound {ref['E_fro']:.3e})")
    assert np.all(err <= ref["E_fro"])
    v = pca.components_.cpu().numpy().astype(np.float64)
    for j in range(3):
        w = ref["vec"][j]
        sin = float(np.linalg.norm(v[j] - (v[j] @ w) * w) / np.linalg.norm(v[j]))
        bound = 2 * ref["E_fro"] / ref["gap"][j]
        print(f"D = {D} component {j}: sin(theta) = {sin:.3e} (Davis-Kahan bound {bound:.3e})")
        assert sin <= bound
        assert v[j, int(np.argmax(np.abs(v[j])))] > 0, "the sign rule"
        assert float(v[j] @ w) > 0, "and the reference's sign with it"
        assert abs(float(np.linalg.norm(v[j])) - 1.0) <= 4 * pr.U
    ratio = pca.explained_variance_ratio_
    assert ratio.dtype == np.float64 and float(ratio.sum()) <= 1.0 and np.all(ratio > 0)
    # lambda / trace: the eigenvalue is within ||E||_F, the trace within trace(E)
    assert np.all(np.abs(ratio - ref["lam"][:3] / ref["trace"]) <= (ref["E_fro"] + ref["E_trace"]) / (ref["trace"] - ref["E_trace"]))
    # the same bits twice, and over a list of two halves
    again = PCA(3).fit(case["xd"])
    assert np.array_equal(_bits(again.components_), _bits(pca.components_)) and np.array_equal(again.explained_variance_, lam)
    half = _emb(case["xd"][:500].contiguous(), np.zeros((500, 2)), np.arange(500), 4096, 4096, 32, 32, n_unique=500, n_padded=500)
    parts = PCA(3).fit([half, case["xd"][500:]])
    assert np.array_equal(_bits(parts.components_), _bits(pca.components_)) and np.array_equal(_bits(parts.mean_), _bits(pca.mean_))
    assert np.array_equal(parts.explained_variance_, lam) and np.array_equal(parts.explained_variance_ratio_, ratio)


# ---- whitening and transform -----------------------------------------------------------------------------------------------------------
def test_whitened_columns_have_unit_variance(dev):
    """transform with whiten against the float64 projection of the same float32 differences, components and scales (the project
    gate g per element), and the columns' sample variance against 1.  What the variance may differ by: the exact projection's
    variance is v^T C v / lambda_j with C the exact covariance about the float32 mean, within ||E||_F / lambda_j + 8 u of 1 (v is the
    device covariance's eigenvector; 8 u for the float32 rounding of v and of the scale); the elements' errors move it by at most
    2 sqrt(var) sqrt(sum g^2 / (n - 1)) to first order (2.1 here)."""
    from deephisto_amd.pca import PCA
    case = _planted(64, dev)
    x, ref, n = case["x"], case["ref"], 1030
    pca = PCA(3, whiten=True).fit(case["xd"])
    z = pca.transform(case["xd"])
    assert tuple(z.shape) == (n, 3) and z.dtype == torch.float32
    scale = (1.0 / np.sqrt(pca.explained_variance_)).astype(np.float32)
    want, gate = pr.project_ref(x, pca.mean_.cpu().numpy(), pca.components_.cpu().numpy(), scale)
    z64 = z.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(z64 - want) <= gate)
    var = z64.var(axis=0, ddof=1)
    tol = ref["E_fro"] / pca.explained_variance_ + 8 * pr.U + 2.1 * np.sqrt((gate ** 2).sum(0) / (n - 1))
    print(f"whitened variances - 1 = {var - 1.0} (allowed {tol})")
    assert np.all(np.abs(var - 1.0) <= tol)
    plain = PCA(3).fit(case["xd"]).transform(case["xd"])
    assert np.all(np.abs(plain.cpu().numpy().astype(np.float64).var(axis=0, ddof=1) / pca.explained_variance_ - 1.0) <= tol)


def test_transform_pads_with_exact_zeros(dev):
    from deephisto_amd.pca import PCA
    case = _planted(64, dev)
    pca = PCA(3).fit(case["xd"])
    z, wide = pca.transform(case["xd"]), pca.transform(case["xd"], width=64)
    assert tuple(wide.shape) == (1030, 64) and np.array_equal(_bits(wide[:, :3].contiguous()), _bits(z))
    assert not bool(wide[:, 3:].any()) and not bool(torch.signbit(wide[:, 3:]).any()), "exact +0 behind column K"
    for bad in (2, 6):
        with pytest.raises(ValueError, match="width"):
            pca.transform(case["xd"], width=bad)


# ---- reduce and k-means ------------------------------------------------------------------------------------------------------------------
def test_kmeans_on_the_reduced_rows_recovers_the_blobs(dev):
    from deephisto_amd.clustering import KMeans, cluster_map
    from deephisto_amd.pca import PCA
    x, which, centres = cr.blobs(D=128)
    n = len(x)
    P = 32
    origins = np.stack(np.divmod(np.arange(n), 32), axis=1).astype(np.int32) * P      # 33 rows of 32 tiles, the last row short
    emb = _emb(_t(x, dev), origins, np.arange(n), 33 * P, 32 * P, P, P, n_unique=n, n_padded=n)
    pca = PCA(8).fit(emb)
    red = pca.reduce(emb, width=64)
    assert tuple(red.features.shape) == (n, 64) and not bool(red.features[:, 8:].any())
    assert np.array_equal(red.origins, emb.origins) and np.array_equal(red.tile_index, emb.tile_index)
    assert (red.h, red.w, red.patch_size, red.stride, red.n_unique, red.n_padded) == (emb.h, emb.w, P, P, n, n)
    init = pca.transform(_t(centres, dev), width=64)
    # the float64 Lloyd over the very float32 rows the assign kernel reads asserts the margins a float32 run needs
    ref = cr.lloyd_ref(red.features.cpu().numpy(), init.cpu().numpy())
    km = KMeans(4, init=init, normalize=False).fit(red)
    assert km.converged_ and km.counts_.tolist() == list(cr.BLOB_SIZES)
    assert np.array_equal(km.labels_.cpu().numpy(), ref["labels"]) and np.array_equal(km.labels_.cpu().numpy(), which), \
        "the blobs' partition, exactly (sizes descend with the blob number, so the canonical numbers are the blobs')"
    cmap = cluster_map(red, km.labels_, 4, downscale=16).cpu().numpy()
    for i in (0, 17, 500, n - 1):   # tiles do not overlap: a tile's four cells carry its label
        y, xx = origins[i] // 16
        assert (cmap[y:y + 2, xx:xx + 2] == which[i]).all()


# ---- the colour map ------------------------------------------------------------------------------------------------------------------------
def test_colour_map_against_numpy(dev):
    from deephisto_amd import tiles
    from deephisto_amd.pca import PCA
    h, w, P, S, d = 160, 128, 32, 16, 16
    grid, n_unique = tiles.tile_grid(h, w, P, S, 1)
    grid = grid[:n_unique]
    rng = np.random.default_rng(8)
    keep = ~((grid[:, 0] < 64) & (grid[:, 1] < 48)) & (rng.random(n_unique) < 0.8)     # a corner gone whole, gaps elsewhere
    tile_index = np.flatnonzero(keep)
    origins = grid[tile_index]
    n = len(tile_index)
    x = (20.0 + rng.standard_normal((n, 4)) @ (rng.standard_normal((4, 64)) * np.array([[5.0], [3.0], [2.0], [1.0]]))
         + 0.1 * rng.standard_normal((n, 64))).astype(np.float32)
    emb = _emb(_t(x, dev), origins, tile_index, h, w, P, S)
    pca = PCA(3).fit(emb)
    z = pca.transform(emb).cpu().numpy().astype(np.float64)
    got = pca.colour_map(emb, downscale=d)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h // d, w // d, 3) and got.is_cuda
    want, hits = pr.colour_map_ref(z, origins, P, d, h, w)
    g = got.cpu().numpy().astype(np.int64)
    assert (hits[:3, :2] == 0).all() and (hits > 1).any(), "cells only missing tiles cover, and overlapping tiles elsewhere"
    assert np.all(np.abs(g - want.astype(np.int64)) <= 1), "within one grey level (the float32 affine can cross a rounding boundary)"
    print(f"colour map: {int((g != want).sum())} of {g.size} levels differ by one")
    assert (g[hits == 0] == 0).all() and g[hits > 0].any()
    # fewer components: the missing channels stay 0; another clip; a constant channel is 128 wherever a tile covers
    one = pca.colour_map(emb, downscale=d, components=(1,), clip=(0.0, 100.0)).cpu().numpy()
    want1, _ = pr.colour_map_ref(z[:, 1:2], origins, P, d, h, w, clip=(0.0, 100.0))
    assert np.all(np.abs(one.astype(np.int64) - want1.astype(np.int64)) <= 1) and not one[..., 1:].any()
    pca.components_[2].zero_()
    flat = pca.colour_map(emb, downscale=d).cpu().numpy()
    assert (flat[..., 2][hits > 0] == 128).all() and (flat[..., 2][hits == 0] == 0).all()
    assert np.array_equal(flat[..., :2], g[..., :2])
    with pytest.raises(ValueError, match="components"):
        pca.colour_map(emb, components=(0, 3))


# ---- refusals by name ------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from deephisto_amd.pca import PCA
    x = torch.randn((10, 64), dtype=torch.float32, device=dev)
    share = _emb(x, np.zeros((10, 2)), np.arange(10), 4096, 4096, 32, 32, n_unique=40, n_padded=40, row_range=(10, 20))
    with pytest.raises(ValueError, match="row_range"):
        PCA(2).fit(share)
    with pytest.raises(ValueError, match="row_range"):
        PCA(2).fit([x, share])
    with pytest.raises(ValueError, match="n >= 2"):
        PCA(1).fit(x[:1])
    with pytest.raises(ValueError, match="n_components"):
        PCA(65)
    with pytest.raises(RuntimeError, match="GPU memory"):
        PCA(2).fit(x.cpu())
    with pytest.raises(RuntimeError, match="GPU memory"):
        PCA(2).fit(x).transform(x.cpu())
    with pytest.raises(ValueError, match="all of them"):
        PCA(2).fit(x).colour_map(share, components=(0, 1))
