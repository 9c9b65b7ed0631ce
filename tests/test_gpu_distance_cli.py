"""GPU: `--margin` / `--score_tolerance` / `--surface` / `--distance_json` through the CLI of examples/predict_full_patched.py, in
process, on the --synthetic slide, random weights and annotation route of tests/test_gpu_knn_cli.py."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--synthetic", "700", "900", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64", "--batch_size", "16",
        "--compute_dtype", "bf16"]
STEM = "synthetic_700x900"
STANDARD = [f"{STEM}.jpg", f"{STEM}_mask.jpg", f"{STEM}_overlay.jpg", f"{STEM}_truth.jpg", f"{STEM}_errors.jpg"]
D = 16
EDGES = [-48, 0, 32, 200]


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
    """Three runs shared by the tests below: with the annotation only; the same with the distance flags; the distance flags on the
    cleaned map."""
    from deephisto_amd.examples.predict_full_patched import main
    from deephisto_amd.scoring import synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("distance_cli")
    anno = root / "anno.json"
    anno.write_text(json.dumps(synthetic_annotation(700, 900, 4, 24, list(KNOWN_COLORS), seed=36)))
    label = _most_common_label(main(ARGS + ["--out_dir", str(root / "probe"), "--no_visualizations"]))
    common = ["--anno", str(anno)]
    flags = ["--margin", f"{label}:" + ",".join(str(e) for e in EDGES), "--score_tolerance", "16", "--surface"]
    plain = main(ARGS + common + ["--out_dir", str(root / "plain"), "--score_json", str(root / "plain" / "score.json")])
    full = main(ARGS + common + flags + ["--out_dir", str(root / "full"), "--score_json", str(root / "full" / "score.json"),
                                         "--distance_json", str(root / "full" / "distance.json")])
    clean = main(ARGS + common + flags + ["--out_dir", str(root / "clean"), "--no_visualizations", "--min_region", "6",
                                          "--distance_json", str(root / "clean" / "distance.json")])
    return dict(root=root, anno=anno, label=label, plain=plain, full=full, clean=clean)


def _most_common_label(pred) -> str:
    """The label of the class that holds most cells of the map: a margin around it has cells on both sides."""
    from deephisto_amd.visualize import KNOWN_COLORS
    counts = torch.bincount(torch.as_tensor(pred).flatten().clamp_min(0).cpu(), minlength=len(KNOWN_COLORS))
    return list(KNOWN_COLORS)[int(counts.argmax())]


def _expected(pred, anno_path, label, tmp_path):
    """The report the Python API gives for a class map, written by `save_distance_report` and read back."""
    from deephisto_amd import distance, scoring
    from deephisto_amd.anno.utils import AnnoDescription
    from deephisto_amd.visualize import KNOWN_COLORS
    dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
    labels = list(KNOWN_COLORS)
    pred = torch.as_tensor(pred).cuda()
    truth, _ = scoring.rasterize_annotation(json.loads(anno_path.read_text()), dsc, 1, 700, 900, D)
    bands = distance.margin_bands(pred, [labels.index(label)], EDGES, D)
    held = [k for k in range(len(labels)) if bool((truth == k).any())]
    path = distance.save_distance_report(
        tmp_path / "expected.json", D,
        margin=dict(label=label, edges_px=EDGES, class_labels=labels, counts=distance.band_composition(pred, bands, len(labels), len(EDGES) - 1)),
        tolerant=dict(tolerance_px=16, score=distance.tolerant_score(pred, truth, labels, 16, D)),
        surface={labels[k]: distance.surface_distances(pred, truth, k, D) for k in held})
    return json.loads(path.read_text()), bands, held


def test_the_report_is_what_the_api_returns_on_the_map(runs, tmp_path):
    doc = json.loads((runs["root"] / "full" / "distance.json").read_text())
    want, bands, held = _expected(runs["full"], runs["anno"], runs["label"], tmp_path)
    assert doc == want
    assert doc["downscale"] == D and doc["margin"]["label"] == runs["label"] and doc["margin"]["edges_px"] == EDGES
    counts = np.asarray(doc["margin"]["counts"])
    assert counts.shape == (3, 6) and counts.sum() == int((bands >= 0).sum())
    if len(torch.unique(torch.as_tensor(runs["full"]))) > 1:     # a map of one class has no border to measure from
        assert counts[0].sum() > 0 and counts[1].sum() > 0
    assert doc["tolerant"]["tolerance_px"] == 16 and doc["tolerant"]["score"]["n_cells"] == (700 // D) * (900 // D)
    plain_score = json.loads((runs["root"] / "plain" / "score.json").read_text())
    assert 0 < doc["tolerant"]["score"]["n_labelled"] < plain_score["n_labelled"]
    assert len(held) >= 1 and sorted(doc["surface"]) == sorted(plain_score["labels"][k] for k in held)
    assert all(set(v) == {"n_pred", "n_truth", "hausdorff", "hd95", "assd"} and v["n_truth"] > 0 for v in doc["surface"].values())


def test_the_margin_jpeg_is_written_beside_the_others(runs):
    from PIL import Image
    root = runs["root"]
    assert Image.open(root / "full" / f"{STEM}_margin.jpg").size == (900 // D, 700 // D)
    assert sorted(p.name for p in (root / "full").iterdir()) == sorted(STANDARD + [f"{STEM}_margin.jpg", "score.json", "distance.json"])
    assert sorted(p.name for p in (root / "plain").iterdir()) == sorted(STANDARD + ["score.json"])


def test_the_existing_outputs_do_not_change_by_a_byte(runs):
    root = runs["root"]
    assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs["full"]))
    assert torch.equal(torch.as_tensor(runs["plain"]), torch.as_tensor(runs["clean"]))
    for name in STANDARD + ["score.json"]:
        assert (root / "plain" / name).read_bytes() == (root / "full" / name).read_bytes(), name


def test_under_min_region_the_steps_run_on_the_cleaned_map(runs, tmp_path):
    from deephisto_amd import regions
    cleaned, _ = regions.clean_map(torch.as_tensor(runs["clean"]).cuda(), 6, 1, 5)
    doc = json.loads((runs["root"] / "clean" / "distance.json").read_text())
    assert doc == _expected(cleaned, runs["anno"], runs["label"], tmp_path)[0]
    assert sorted(p.name for p in (runs["root"] / "clean").iterdir()) == ["distance.json"]


def test_flag_combinations_are_refused(built_lib, runs, tmp_path):
    from deephisto_amd.examples.predict_full_patched import main
    anno = str(runs["anno"])
    for extra in (["--score_tolerance", "16"], ["--surface"], ["--margin", "XYZ:100", "--anno", anno], ["--margin", "TUM:100,50"],
                  ["--margin", "TUM:5,5"], ["--margin", "TUM"], ["--distance_json", str(tmp_path / "d.json")],
                  ["--anno", anno, "--score_tolerance", "-1"], ["--margin", "TUM:100", "--clusters", "3"]):
        with pytest.raises(SystemExit):
            main(ARGS + ["--out_dir", str(tmp_path / "never"), *extra])
    assert not (tmp_path / "never").exists()
