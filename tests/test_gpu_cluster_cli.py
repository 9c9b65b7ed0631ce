"""GPU: `--clusters`, `--save_clusters` and `--load_clusters` through the CLI of examples/predict_full_patched.py, in process, on the
--synthetic slide and random weights of tests/test_gpu_embed_cli.py."""
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
    """Three runs shared by the tests below: plain, --clusters 3 with --save_clusters and the region flags, --load_clusters."""
    from deephisto_amd.examples.predict_full_patched import main
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("cluster_cli")
    book = root / "books" / "codebook.npz"
    plain = main(ARGS + ["--out_dir", str(root / "plain")])
    fit = main(ARGS + ["--out_dir", str(root / "fit"), "--clusters", "3", "--cluster_seed", "4", "--save_clusters", str(book),
                       "--regions_json", str(root / "fit" / "regions.json"), "--export_anno", str(root / "fit" / "anno.json")])
    load = main(ARGS + ["--out_dir", str(root / "load"), "--load_clusters", str(book)])
    return dict(root=root, book=book, plain=plain, fit=fit, load=load)


def test_clusters_writes_the_map_and_the_summary(runs):
    root = runs["root"]
    jpg = root / "fit" / f"{STEM}_clusters.jpg"
    assert jpg.is_file() and jpg.stat().st_size > 1000
    doc = json.loads((root / "fit" / f"{STEM}_clusters.json").read_text())
    assert doc["n_clusters"] == 3 and len(doc["sizes"]) == 3 and sum(doc["sizes"]) == doc["n_tiles"] == 154, "every kept tile is in a cluster"
    assert doc["sizes"] == sorted(doc["sizes"], reverse=True) and doc["iterations"] >= 1 and isinstance(doc["converged"], bool)
    assert doc["inertia"] >= 0 and np.isfinite(doc["inertia"]) and doc["seed"] == 4 and doc["init"] == "kmeans++"
    assert list(doc["colors"]) == ["cluster_0", "cluster_1", "cluster_2"]


def test_the_class_map_and_its_jpegs_do_not_change(runs):
    root = runs["root"]
    assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs["fit"]))
    for name in (f"{STEM}_mask.jpg", f"{STEM}_overlay.jpg", f"{STEM}.jpg"):
        assert (root / "plain" / name).read_bytes() == (root / "fit" / name).read_bytes(), name
    assert not (root / "plain" / f"{STEM}_clusters.jpg").exists() and not (root / "plain" / f"{STEM}_clusters.json").exists()


def test_a_saved_codebook_reproduces_the_map(runs):
    from deephisto_amd.clustering import KMeans
    root = runs["root"]
    km = KMeans.load(runs["book"])
    assert km.centres_.shape == (3, 512) and int(km.counts_.sum()) == 154
    assert (root / "load" / f"{STEM}_clusters.jpg").read_bytes() == (root / "fit" / f"{STEM}_clusters.jpg").read_bytes()
    a = json.loads((root / "fit" / f"{STEM}_clusters.json").read_text())
    b = json.loads((root / "load" / f"{STEM}_clusters.json").read_text())
    assert b["sizes"] == a["sizes"] and b["inertia"] == a["inertia"], "a fit ends on an assignment to the centres it returns"
    assert b["fitted_here"] is False and a["fitted_here"] is True


def test_the_region_flags_describe_the_cluster_map(runs):
    root = runs["root"]
    doc = json.loads((root / "fit" / "regions.json").read_text())
    assert doc["n_regions"] >= 1 and {r["class"] for r in doc["regions"]} <= {"cluster_0", "cluster_1", "cluster_2"}
    anno = json.loads((root / "fit" / "anno.json").read_text())
    assert {r["class"] for r in anno} <= {"cluster_0", "cluster_1", "cluster_2"}


def test_flag_combinations_are_refused(built_lib, tmp_path):
    from deephisto_amd.examples.predict_full_patched import main
    for extra in (["--clusters", "0"], ["--clusters", "65"], ["--cluster_seed", "1"], ["--save_clusters", str(tmp_path / "x.npz")],
                  ["--clusters", "3", "--proba"], ["--clusters", "3", "--min_region", "4"], ["--load_clusters", str(tmp_path / "none.npz")]):
        with pytest.raises(SystemExit):
            main(ARGS + ["--out_dir", str(tmp_path), *extra])
