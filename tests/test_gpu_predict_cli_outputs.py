"""GPU: what `main` of examples/predict_full_patched.py prints, writes and returns for five composite command lines that between
them reach every rank-0 reporter of deephisto_amd/cli, against tests/golden/predict_cli_outputs.json: the record that
tests/helpers/predict_cli_outputs.py (run as a program) took on an MI355X from the commit before the CLI was split into one
module per flag group.  The record holds the printed lines (the seconds after `traced in` masked), the names of the files,
every JSON without its three timing keys, and the SHA-256 of the returned class maps and of every .npy / .npz array; JPEG bytes
depend on the imaging library's build and are not in it."""
import json
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "predict_cli_outputs.json").read_text())


@pytest.fixture(scope="module")
def root(built_lib, tmp_path_factory):
    import predict_cli_outputs as helper
    assert torch.cuda.is_available()
    root = tmp_path_factory.mktemp("predict_cli_outputs")
    helper.write_annotation(root / "anno.json")
    return root


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_a_composite_command_line_leaves_what_it_left_before_the_split(root, name):
    import predict_cli_outputs as helper
    from deephisto_amd.examples.predict_full_patched import main
    want = GOLDEN[name]
    got = helper.run_case(main, helper.cases(root, root / "anno.json")[name], root / name, root)
    assert got["lines"] == want["lines"]
    assert got["files"] == want["files"]
    assert got["class_maps"] == want["class_maps"]
    for path in want["json"]:
        assert json.dumps(got["json"][path], sort_keys=True) == json.dumps(want["json"][path], sort_keys=True), path   # NaN == NaN as text
    assert sorted(got["json"]) == sorted(want["json"]) and got["sha256"] == want["sha256"]


def test_the_cases_reach_every_reporter():
    import predict_cli_outputs as helper
    flags = {a for argvs in helper.cases(Path("r"), Path("a")).values() for argv in argvs for a in argv if a.startswith("--")}
    assert flags >= {"--tissue", "--min_sharpness", "--quality_json", "--proba", "--heat", "--save_proba", "--anno", "--score_json",
                     "--regions_json", "--min_region", "--export_anno", "--margin", "--score_tolerance", "--surface", "--distance_json",
                     "--stain", "--save_stain_fit", "--pyramid", "--tta", "--prototypes", "--knn", "--knn_bank", "--knn_per_class",
                     "--similar_to", "--pca", "--save_pca", "--load_pca", "--save_embeddings", "--clusters", "--save_clusters",
                     "--load_clusters", "--fine"}
