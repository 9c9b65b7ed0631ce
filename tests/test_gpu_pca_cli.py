"""GPU: `--pca`, `--save_pca` and `--load_pca` through the CLI of examples/predict_full_patched.py, in process, on the --synthetic slide
and random weights of tests/test_gpu_cluster_cli.py."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--synthetic", "700", "900", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64", "--batch_size", "16",
        "--compute_dtype", "bf16"]
STEM = "synthetic_700x900"


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
    """Three runs shared by the tests below: plain, --pca 3 with --save_pca, --load_pca."""
    from deephisto_amd.examples.predict_full_patched import main
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("pca_cli")
    basis = root / "bases" / "basis.npz"
    plain = main(ARGS + ["--out_dir", str(root / "plain")])
    fit = main(ARGS + ["--out_dir", str(root / "fit"), "--pca", "3", "--save_pca", str(basis)])
    load = main(ARGS + ["--out_dir", str(root / "load"), "--load_pca", str(basis)])
    return dict(root=root, basis=basis, plain=plain, fit=fit, load=load)


def test_pca_writes_the_picture_the_summary_and_the_basis(runs):
    from PIL import Image
    root = runs["root"]
    jpg = root / "fit" / f"{STEM}_pca.jpg"
    assert jpg.is_file() and Image.open(jpg).size == (900 // 16, 700 // 16)
    doc = json.loads((root / "fit" / f"{STEM}_pca.json").read_text())
    assert doc["n_components"] == 3 and doc["n_tiles"] == doc["n_samples"] == 154 and doc["fitted_here"] is True
    var, ratio = doc["explained_variance"], doc["explained_variance_ratio"]
    assert len(var) == len(ratio) == 3 and var == sorted(var, reverse=True) and all(np.isfinite(var)) and var[0] > 0
    assert 0 < sum(ratio) <= 1.0
    for key in ("scatter_ms", "eigen_ms", "project_ms"):
        assert doc[key] >= 0 and np.isfinite(doc[key]), key
    assert runs["basis"].is_file()


def test_a_saved_basis_reproduces_the_picture(runs):
    from deephisto_amd.pca import PCA
    root = runs["root"]
    pca = PCA.load(runs["basis"])
    assert tuple(pca.components_.shape) == (3, 512) and tuple(pca.mean_.shape) == (512,) and pca.n_samples_ == 154
    assert (root / "load" / f"{STEM}_pca.jpg").read_bytes() == (root / "fit" / f"{STEM}_pca.jpg").read_bytes()
    a = json.loads((root / "fit" / f"{STEM}_pca.json").read_text())
    b = json.loads((root / "load" / f"{STEM}_pca.json").read_text())
    assert b["explained_variance"] == a["explained_variance"] and b["explained_variance_ratio"] == a["explained_variance_ratio"]
    assert b["fitted_here"] is False and b["scatter_ms"] is None and b["eigen_ms"] is None


def test_the_class_map_and_its_jpegs_do_not_change(runs):
    root = runs["root"]
    assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs["fit"]))
    assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs["load"]))
    plain = sorted(p.name for p in (root / "plain").iterdir())
    assert plain == sorted([f"{STEM}.jpg", f"{STEM}_mask.jpg", f"{STEM}_overlay.jpg"])
    for name in plain:
        assert (root / "plain" / name).read_bytes() == (root / "fit" / name).read_bytes(), name
    assert sorted(p.name for p in (root / "fit").iterdir()) == sorted(plain + [f"{STEM}_pca.jpg", f"{STEM}_pca.json"])


def test_flag_combinations_are_refused(built_lib, tmp_path):
    from deephisto_amd.examples.predict_full_patched import main
    for extra in (["--pca", "0"], ["--pca", "65"], ["--save_pca", str(tmp_path / "x.npz")], ["--pca", "3", "--proba"],
                  ["--pca", "3", "--tta", "flips"], ["--load_pca", str(tmp_path / "none.npz")]):
        with pytest.raises(SystemExit):
            main(ARGS + ["--out_dir", str(tmp_path), *extra])
