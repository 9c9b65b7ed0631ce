"""GPU: `--knn` / `--knn_bank` / `--knn_per_class` and `--similar_to` through the CLI of examples/predict_full_patched.py, in process,
on the --synthetic slide, random weights and annotation route of tests/test_gpu_embed_cli.py."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--synthetic", "700", "900", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64", "--batch_size", "16",
        "--compute_dtype", "bf16"]
STEM = "synthetic_700x900"
STANDARD = [f"{STEM}.jpg", f"{STEM}_mask.jpg", f"{STEM}_overlay.jpg"]
KNN = [f"{STEM}_knn.jpg", f"{STEM}_knn_overlay.jpg"]


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
    """Four runs shared by the tests below: plain; a fit on the annotation; a load of the fitted bank with the region flags; a
    retrieval."""
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.scoring import synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("knn_cli")
    anno = root / "anno.json"
    anno.write_text(json.dumps(synthetic_annotation(700, 900, 2, 24, list(KNOWN_COLORS), seed=36)))
    bank = root / "banks" / "bank.npz"
    plain = main(ARGS + ["--out_dir", str(root / "plain")])
    fit = main(ARGS + ["--out_dir", str(root / "fit"), "--anno", str(anno), "--knn", "3", "--knn_bank", str(bank)])
    load = main(ARGS + ["--out_dir", str(root / "load"), "--knn", "3", "--knn_bank", str(bank),
                        "--regions_json", str(root / "load" / "regions.json")])
    similar = main(ARGS + ["--out_dir", str(root / "similar"), "--no_visualizations", "--similar_to", "333,444", "--similar_k", "7"])
    return dict(root=root, anno=anno, bank=bank, plain=plain, fit=fit, load=load, similar=similar)


def test_the_fit_writes_the_bank_and_the_two_jpegs(runs):
    from PIL import Image
    from deephisto_amd.neighbours import KNNClassifier
    root = runs["root"]
    knn = KNNClassifier.load(runs["bank"])
    assert (knn.n_classes, knn.k, knn.normalize) == (5, 3, True) and tuple(knn.bank.shape) == (8, 512)
    assert knn.counts.tolist() == [0, 4, 4, 0, 0] and sorted(knn.labels.tolist()) == [1, 1, 1, 1, 2, 2, 2, 2]
    assert np.allclose(knn.bank.square().sum(1).numpy(), 1.0, atol=1e-5)
    for name in KNN:
        assert Image.open(root / "fit" / name).size == (900 // 16, 700 // 16), name
    assert sorted(p.name for p in (root / "fit").iterdir()) == sorted(STANDARD + KNN + [f"{STEM}_truth.jpg", f"{STEM}_errors.jpg"])


def test_the_loaded_bank_reproduces_the_map(runs):
    root = runs["root"]
    for name in KNN:
        assert (root / "load" / name).read_bytes() == (root / "fit" / name).read_bytes(), name
    doc = json.loads((root / "load" / "regions.json").read_text())   # the region flags describe the k-NN map: two classes only
    classes = {r["class"] for r in doc["regions"]}
    assert doc["n_regions"] == len(doc["regions"]) >= 1 and classes <= {"BG", "LP"}, classes   # the bank's classes 1 and 2


def test_the_class_map_and_its_jpegs_do_not_change(runs):
    root = runs["root"]
    for other in ("fit", "load", "similar"):
        assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs[other])), other
    assert sorted(p.name for p in (root / "plain").iterdir()) == sorted(STANDARD)
    for name in STANDARD:
        assert (root / "plain" / name).read_bytes() == (root / "fit" / name).read_bytes(), name
        assert (root / "plain" / name).read_bytes() == (root / "load" / name).read_bytes(), name


def test_knn_per_class_caps_the_bank(runs, tmp_path):
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.neighbours import KNNClassifier
    capped = tmp_path / "capped.npz"
    main(ARGS + ["--out_dir", str(tmp_path / "out"), "--no_visualizations", "--anno", str(runs["anno"]), "--knn", "1",
                 "--knn_bank", str(capped), "--knn_per_class", "2"])
    full, small = KNNClassifier.load(runs["bank"]), KNNClassifier.load(capped)
    assert small.counts.tolist() == [0, 2, 2, 0, 0] and small.k == 1
    for c in (1, 2):   # every second labelled tile of the class, in tile order, the first among them
        assert torch.equal(small.bank[small.labels == c], full.bank[full.labels == c][::2])


def test_similar_to_writes_the_neighbours_as_json(runs):
    doc = json.loads((runs["root"] / "similar" / f"{STEM}_similar.json").read_text())
    assert doc["pixel"] == [333, 444] and doc["k"] == 7 and doc["patch_size"] == 96
    qy, qx = doc["query_origin"]
    assert qy <= 333 < qy + 96 and qx <= 444 < qx + 96
    origins = doc["origins"]
    assert len(origins) == len(doc["rows"]) == len(doc["dist"]) == 7 and len({tuple(o) for o in origins}) == 7
    for y, x in origins:   # on the tile grid of the 700 x 900 slide, and not the query's tile
        assert (y % 64 == 0 or y == 700 - 96) and (x % 64 == 0 or x == 900 - 96) and 0 <= y <= 700 - 96 and 0 <= x <= 900 - 96
        assert [y, x] != doc["query_origin"]
    assert doc["query_row"] not in doc["rows"] and doc["dist"] == sorted(doc["dist"]) and doc["dist"][0] >= 0
    assert sorted(p.name for p in (runs["root"] / "similar").iterdir()) == [f"{STEM}_similar.json"]


def test_flag_combinations_are_refused(built_lib, runs, tmp_path):
    from deephisto_amd.embeddings import PrototypeClassifier
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.neighbours import KNNClassifier
    bank = str(runs["bank"])
    three = KNNClassifier.load(runs["bank"])
    three.n_classes, three.counts = 3, three.counts[:3]
    three.save(tmp_path / "three.npz")                                     # a bank of another class count
    narrow = KNNClassifier.load(runs["bank"])
    narrow.bank = narrow.bank[:, :64].contiguous()
    narrow.save(tmp_path / "narrow.npz")                                   # a bank of another width
    pc = PrototypeClassifier(5)
    pc.prototypes, pc.counts = torch.zeros((5, 512)), np.zeros(5, np.int64)
    pc.save(tmp_path / "protos.npz")                                       # not a bank at all
    for extra in (["--knn", "3"], ["--knn_bank", bank], ["--knn", "0", "--knn_bank", bank], ["--knn", "64", "--knn_bank", bank],
                  ["--knn", "3", "--knn_bank", str(tmp_path / "none.npz")], ["--knn", "3", "--knn_bank", bank, "--knn_per_class", "4"],
                  ["--knn", "3", "--knn_bank", bank, "--proba"], ["--knn", "3", "--knn_bank", bank, "--tta", "flips"],
                  ["--knn", "3", "--knn_bank", bank, "--clusters", "4"], ["--knn", "3", "--knn_bank", bank, "--min_region", "4"],
                  ["--knn", "3", "--knn_bank", str(tmp_path / "three.npz")], ["--knn", "3", "--knn_bank", str(tmp_path / "protos.npz")],
                  ["--knn", "3", "--knn_bank", bank, "--arch", "resnet50"], ["--knn", "3", "--knn_bank", str(tmp_path / "narrow.npz")],
                  ["--similar_to", "700,10"], ["--similar_to", "10,900"], ["--similar_to", "10"], ["--similar_k", "5"],
                  ["--similar_to", "10,10", "--similar_k", "0"], ["--similar_to", "10,10", "--fine"]):
        with pytest.raises(SystemExit):
            main(ARGS + ["--out_dir", str(tmp_path / "never"), *extra])
    assert not (tmp_path / "never").exists()
