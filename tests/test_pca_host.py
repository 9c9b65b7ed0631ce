"""PCA of tile embeddings, host side (CPU only: no kernel runs): the argument checks of dh_embed_scatter / dh_embed_project before any GPU
call, the pure functions of deephisto_amd/pca.py (sign rule, colour levels), the .npz round trip, the CLI's refusals, and the
reference's own bounds for the planted spectrum that tests/test_gpu_pca.py holds the device to."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import pca_ref as pr  # noqa: E402


# ---- the C ABI, from null pointers ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name_before_any_gpu_call(built_lib):
    lib = built_lib
    err = lambda: lib.dh_last_error().decode()   # noqa: E731
    for D in (0, 32, 100, 4160, -64):
        assert lib.dh_embed_scatter(None, 4, D, None, None, None, None) == -22 and "dh_embed_scatter" in err() and f"D = {D}" in err()
        assert lib.dh_embed_scatter_work_size(4, D) == -1 and f"D = {D}" in err()
        assert lib.dh_embed_project(None, 4, D, None, None, 3, None, None, 4, None) == -22 and "dh_embed_project" in err() \
            and f"D = {D}" in err()
    for K in (0, 65):
        assert lib.dh_embed_project(None, 4, 512, None, None, K, None, None, 68, None) == -22 and f"K = {K}" in err()
    assert lib.dh_embed_scatter(None, -1, 512, None, None, None, None) == -22 and "n = -1" in err()
    assert lib.dh_embed_scatter_work_size(-1, 512) == -1 and "n = -1" in err()
    assert lib.dh_embed_project(None, -1, 512, None, None, 3, None, None, 4, None) == -22 and "n = -1" in err()
    assert lib.dh_embed_project(None, 4, 512, None, None, 5, None, None, 4, None) == -22 and "ld = 4" in err(), "ld < K"
    assert lib.dh_embed_project(None, 4, 512, None, None, 5, None, None, 6, None) == -22 and "ld = 6" in err(), "ld % 4 != 0"
    assert lib.dh_embed_project(None, 4, 512, None, None, 5, None, None, 4100, None) == -22 and "ld = 4100" in err()
    # good dimensions, null pointers: still refused on the host; n = 0 needs none
    assert lib.dh_embed_scatter(None, 4, 512, None, None, None, None) == -22 and "dh_embed_scatter" in err() and "null" in err()
    assert lib.dh_embed_project(None, 4, 512, None, None, 5, None, None, 8, None) == -22 and "dh_embed_project" in err() and "null" in err()
    assert lib.dh_embed_scatter(None, 0, 512, None, None, None, None) == 0
    assert lib.dh_embed_project(None, 0, 512, None, None, 5, None, None, 8, None) == 0
    odd, ok = C.c_void_p(4), C.c_void_p(64)
    assert lib.dh_embed_scatter(odd, 4, 512, ok, ok, None, None) == -22 and "aligned" in err()
    assert lib.dh_embed_scatter(ok, 4, 512, ok, odd, None, None) == -22 and "aligned" in err()
    assert lib.dh_embed_project(ok, 4, 512, odd, ok, 5, None, ok, 8, None) == -22 and "aligned" in err()
    assert lib.dh_embed_project(ok, 4, 512, ok, ok, 5, None, odd, 8, None) == -22 and "aligned" in err()
    # a matrix whose work size is not 0 needs the scratch it asks for
    assert lib.dh_embed_scatter(ok, 2000, 512, ok, ok, None, None) == -22 and "work_dev" in err()


def test_scatter_work_size(built_lib):
    """One 64 x 64 partial per tile of the triangle and chunk of a batch: a batch is all chunks, capped so that the scratch stays within
    2^26 floats and half the feature matrix; 0 where that leaves no batch of two chunks (a workgroup then walks the chunks itself)."""
    lib = built_lib
    assert lib.dh_embed_scatter_work_size(0, 512) == 0 and lib.dh_embed_scatter_work_size(1024, 512) == 0
    assert lib.dh_embed_scatter_work_size(1025, 64) == 2 * 1 * 4096
    assert lib.dh_embed_scatter_work_size(3100, 192) == 4 * 6 * 4096
    assert lib.dh_embed_scatter_work_size(1025, 512) == 0 and lib.dh_embed_scatter_work_size(2053, 2048) == 0
    assert lib.dh_embed_scatter_work_size(3100, 1024) == 2 * 136 * 4096, "four chunks in two batches"
    assert lib.dh_embed_scatter_work_size(198916, 512) == 195 * 36 * 4096, "every chunk in one batch"
    assert lib.dh_embed_scatter_work_size(198916, 2048) == 31 * 528 * 4096
    for n in (38416, 198916):
        for D in (512, 1024, 2048, 4096):
            assert 0 < lib.dh_embed_scatter_work_size(n, D) <= min(2 ** 26, n * D // 2)
    from deephisto_amd import embeddings
    assert embeddings.CHUNK_ROWS == pr.CHUNK_ROWS


# ---- pure Python ----------------------------------------------------------------------------------------------------------------
def test_sign_rule_on_a_hand_made_basis(built_lib):
    from deephisto_amd.pca import fix_signs, top_components
    v = np.array([[0.1, -0.9, 0.2], [0.5, 0.5, -0.5], [-0.5, 0.5, 0.5], [0.0, 0.3, 0.1]])
    got = fix_signs(v)
    assert np.array_equal(got[0], -v[0]), "the largest magnitude is negative: flipped"
    assert np.array_equal(got[1], v[1]), "a three-way tie: the FIRST index decides, and it is positive"
    assert np.array_equal(got[2], -v[2]), "a three-way tie whose first entry is negative: flipped"
    assert np.array_equal(got[3], v[3]) and np.array_equal(got, pr.fix_signs_ref(v))
    assert np.array_equal(v[0], [0.1, -0.9, 0.2]), "the input is not written"
    # a diagonal covariance: descending eigenvalues, unit vectors along the axes, positive
    lam, vec = top_components(np.diag([2.0, 7.0, 0.5, 3.0]), 3)
    assert lam.tolist() == [7.0, 3.0, 2.0] and np.array_equal(vec, np.eye(4)[[1, 3, 0]])


def test_colour_levels_against_hand_values(built_lib):
    from deephisto_amd.pca import colour_levels
    v = torch.tensor([-5.0, 0.0, 1.0, 2.5, 5.0, 9.999, 10.0, 40.0, 3.0], dtype=torch.float32)
    cov = torch.tensor([True] * 8 + [False])
    got = colour_levels(v, cov, 0.0, 10.0)
    # 255 * 0.1 + 0.5 = 26.0 -> 26; 255 * 0.25 + 0.5 = 64.25 -> 64; 255 * 0.5 + 0.5 = 128.0 -> 128; 255 * 0.9999 + 0.5 = 255.47 -> 255
    assert got.dtype == torch.uint8 and got.tolist() == [0, 0, 26, 64, 128, 255, 255, 255, 0]
    assert colour_levels(v, cov, 2.0, 2.0).tolist() == [128] * 8 + [0], "hi == lo: 128 wherever a tile covers, 0 elsewhere"
    assert colour_levels(v.reshape(3, 3), cov.reshape(3, 3), 0.0, 10.0).shape == (3, 3)


def test_pca_npz_round_trip(built_lib, tmp_path):
    from deephisto_amd.pca import PCA
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match="n_components"):
            PCA(bad)
    pca = PCA(3, whiten=True, normalize=True)
    with pytest.raises(ValueError):
        pca.save(tmp_path / "none.npz")
    with pytest.raises(ValueError, match="fit"):
        pca.transform(torch.zeros((2, 64)))
    pca.mean_ = torch.arange(64, dtype=torch.float32)
    pca.components_ = torch.arange(3 * 64, dtype=torch.float32).reshape(3, 64)
    pca.explained_variance_ = np.array([9.0, 4.0, 0.25])
    pca.explained_variance_ratio_ = np.array([0.5, 0.25, 0.0625])
    pca.n_samples_ = 1030
    pca.save(tmp_path / "pca.npz")
    with np.load(tmp_path / "pca.npz", allow_pickle=False) as z:
        assert set(z.files) == {"mean", "components", "explained_variance", "explained_variance_ratio", "meta"}
        assert z["meta"].dtype.kind == "U" and '"deephisto_amd.PCA/1"' in str(z["meta"])
    got = PCA.load(tmp_path / "pca.npz")
    assert (got.n_components, got.whiten, got.normalize, got.n_samples_) == (3, True, True, 1030)
    assert torch.equal(got.mean_, pca.mean_) and torch.equal(got.components_, pca.components_)
    assert got.explained_variance_.dtype == np.float64 and got.explained_variance_.tolist() == [9.0, 4.0, 0.25]
    assert got.explained_variance_ratio_.tolist() == [0.5, 0.25, 0.0625]
    np.savez(tmp_path / "other.npz", meta=np.array('{"format": "deephisto_amd.KMeans/1"}'), mean=np.zeros(4))
    with pytest.raises(ValueError, match="not a PCA file"):
        PCA.load(tmp_path / "other.npz")
    np.savez(tmp_path / "bare.npz", mean=np.zeros(4))
    with pytest.raises(ValueError, match="not a PCA file"):
        PCA.load(tmp_path / "bare.npz")


def test_cpu_tensors_are_refused(built_lib):
    from deephisto_amd.pca import PCA, centred_scatter, project
    x = torch.zeros((4, 64))
    with pytest.raises(RuntimeError, match="GPU memory"):
        centred_scatter(x, torch.zeros(64))
    with pytest.raises(RuntimeError, match="GPU memory"):
        project(x, torch.zeros(64), torch.zeros((2, 64)))
    with pytest.raises(RuntimeError, match="GPU memory"):
        PCA(2).fit(x)


# ---- the reference's own bounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_planted_reference_resolves_the_three_components(D):
    """The float64 PCA of the planted rows (n = 1030; standard deviations 10, 5, 2 over noise of 0.1, offset +20) finds the planted
    directions, and its Davis-Kahan bound 2 ||E||_F / gap_j is small enough to be a test.  ||E||_F is about (1024 + 2 + 6) u times the
    total variance (129 + noise: 7.3e-3 measured), whatever the directions are, so the bound is that over half the gap: below
    1e-3 for the first two components (gaps 80 and 21: 1.8e-4 and 7.1e-4 measured) and, with a gap of 4.1, 3.6e-3 for the third."""
    x, q = pr.planted(D=D)
    ref = pr.pca_ref(x, 3)
    bound = 2 * ref["E_fro"] / ref["gap"]
    print(f"D = {D}: eigenvalues {ref['lam'][:4]}, ||E||_F = {ref['E_fro']:.3e}, gaps {ref['gap']}, sin bound {bound}")
    assert np.all(bound[:2] < 1e-3) and bound[2] < 4e-3
    assert ref["E_fro"] < 1e-2 * ref["gap"].min(), "Weyl: the three eigenvalues stay apart"
    assert np.allclose(ref["lam"][:3], np.square(pr.STDS), rtol=0.15) and ref["lam"][3] < 0.03
    for j in range(3):   # the sample directions are the planted ones up to sampling error
        assert abs(float(ref["vec"][j] @ q[j])) > 0.99
    assert float(np.abs(ref["mean32"] - 20.0).max()) < 2.0, "the common offset dominates the mean"


# ---- the CLI's refusals ------------------------------------------------------------------------------------------------------------
BASE = ["--synthetic", "300", "300", "--weights", ""]


@pytest.mark.parametrize("other", [["--random_sampler"], ["--ondisk"], ["--tta", "flips"], ["--proba"]])
@pytest.mark.parametrize("flag", ["--pca", "--load_pca"])
def test_cli_refuses_pca_off_the_dense_resident_route(built_lib, tmp_path, capsys, flag, other):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    (tmp_path / "x.npz").write_bytes(b"")
    args = ap.parse_args(BASE + [flag, "3" if flag == "--pca" else str(tmp_path / "x.npz"), *other])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert flag in capsys.readouterr().err


def test_cli_pca_flag_combinations(built_lib, tmp_path, capsys):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    (tmp_path / "x.npz").write_bytes(b"")
    saved = str(tmp_path / "x.npz")
    for extra, word in ((["--pca", "0"], "1 .. 64"), (["--pca", "65"], "1 .. 64"), (["--save_pca", saved], "--save_pca needs --pca"),
                        (["--load_pca", str(tmp_path / "missing.npz")], "no such file"),
                        (["--load_pca", saved, "--pca", "3"], "belong to a fit"),
                        (["--load_pca", saved, "--save_pca", str(tmp_path / "y.npz")], "belong to a fit")):
        with pytest.raises(SystemExit):
            _check_args(ap, ap.parse_args(BASE + extra))
        assert word in capsys.readouterr().err, extra
    for extra in (["--pca", "1"], ["--pca", "64", "--save_pca", saved], ["--load_pca", saved], ["--pca", "3", "--clusters", "4"]):
        args = ap.parse_args(BASE + extra)
        _check_args(ap, args)
    plain = ap.parse_args(BASE)
    assert plain.pca is None and plain.save_pca is None and plain.load_pca is None
