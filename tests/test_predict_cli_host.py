"""Host: the command line of examples/predict_full_patched.py (deephisto_amd/cli) answers as it did before it was split into
one module per flag group: the `--help` text and a table of refusals and derived values, both recorded from the commit before the
split by tools/record_cli_refusals.py.  `_check_args` runs before any GPU call, so none is touched."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
ROWS = json.loads((GOLDEN / "predict_cli_refusals.json").read_text())


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("record_cli_refusals", REPO / "tools" / "record_cli_refusals.py")
    table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(table)
    tmp = tmp_path_factory.mktemp("cli_refusals")
    table.make_files(tmp)
    return table, tmp


def test_help_text_is_byte_equal(monkeypatch):
    from deephisto_amd.examples import predict_full_patched as pfp
    monkeypatch.setenv("COLUMNS", "80")   # argparse wraps to the terminal
    ap = pfp._build_parser()
    ap.prog = "predict_full_patched"
    assert ap.format_help() == (GOLDEN / "predict_cli_help.txt").read_text()


def test_the_table_covers_what_it_should():
    refused = [r for r in ROWS if r["error"] is not None]
    assert len({r["error"] for r in refused}) >= 100 and len(ROWS) - len(refused) >= 20
    for argv in (["--clusters", "0"], ["--pca", "0"], ["--knn", "64"], ["--fine", "--tta", "d4", "--clusters", "3"],
                 ["--knn", "5", "--clusters", "3", "--min_region", "4"], ["--margin", "X:5", "--clusters", "2"],
                 ["--quality_fill", "TUM", "--tissue", "otsu", "--tissue_fill", "BG", "--ondisk"]):
        assert any(" ".join(argv) in " ".join(r["argv"]) for r in refused), argv


@pytest.mark.parametrize("row", ROWS, ids=[" ".join(r["argv"][10:]) or "base" for r in ROWS])
def test_check_args_answers_as_recorded(table, row):
    from deephisto_amd.examples import predict_full_patched as pfp
    module, tmp = table
    assert module.replay(pfp, row["argv"], tmp, row["foreign_model"]) == row


def test_reexported_checkers_are_the_package_s_objects():
    from deephisto_amd import cli
    from deephisto_amd.cli import common, filters, routes, scoring
    from deephisto_amd.examples import predict_full_patched as pfp
    from deephisto_amd.models.patch_cls_simple import model
    assert pfp._check_args is cli.check_args and pfp._tissue_from_args is filters.tissue_from_args
    assert pfp._anno_from_args is scoring.anno_from_args and pfp._proba_from_args is routes.proba_from_args
    assert pfp._regions_from_args is cli.regions.check and pfp._dense_resident_only is common.dense_resident_only
    assert (pfp.ARCHS, pfp.detect_arch, pfp.resolve_arch) == (model.ARCHS, model.detect_arch, model.resolve_arch)
    assert len(cli.FLAGS) == 8 and len(cli.CHECKS) == 9
