"""Records what the flag checks of the predict CLI answer to a table of command lines, without a GPU:

    python tools/record_cli_refusals.py MODULE OUT.json [HELP.txt]

MODULE (e.g. deephisto_amd.examples.predict_full_patched) is imported from the current directory first, so the table can be
recorded from a worktree of another commit.  Every entry of OUT.json holds the argv, the last line the parser wrote to stderr
(null where the checks pass) and, for a passing row, the values the checks leave on the namespace.  HELP.txt gets the parser's
help text.  Paths below the scratch folder are spelled {tmp}.  tests/test_predict_cli_host.py replays the stored table through
`make_files` and `replay` of this file."""
import contextlib
import importlib
import io
import json
import sys
import tempfile
from pathlib import Path

PROG = "predict_full_patched"
BASE = ["--synthetic", "300", "420", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64"]
T = "{tmp}/"

SINGLE = [   # one broken rule each, in the order of the checks
    ["--clean_rounds", "2"], ["--min_region", "0"], ["--min_region", "4", "--clean_rounds", "0"],
    ["--pyramid", "--ondisk"],
    ["--stain_target", T + "fit.json"], ["--save_stain_fit", T + "fit.json"], ["--stain", "macenko", "--ondisk"],
    ["--stain", "macenko", "--stain_target", T + "missing.json"], ["--stain", "macenko", "--stain_target", T + "garbage.txt"],
    ["--tissue", "otsu", "--random_sampler"], ["--tissue", "otsu", "--ondisk"], ["--tissue", "otsu", "--tissue_fill", "XX"],
    ["--tissue", "foo"], ["--tissue", "300"], ["--tissue", "otsu", "--tissue_min_fraction", "2"],
    ["--quality_json", T + "q.json"], ["--min_sharpness", "5", "--random_sampler"], ["--max_ink", "0.5", "--ondisk"],
    ["--quality_fill", "XX"], ["--min_sharpness", "-1"], ["--max_ink", "2"], ["--min_sharpness", "5", "--patch_size", "2048"],
    ["--tissue", "otsu", "--tissue_fill", "BG", "--quality_fill", "TUM"],
    ["--tta", "d4", "--ondisk"],
    ["--score_json", T + "s.json"], ["--anno", T + "missing.json"], ["--anno", T + "garbage.txt"], ["--anno", T + "no_class.json"],
    ["--anno", T + "number.json"], ["--anno", T + "unknown.json"],
    ["--heat", "TUM"], ["--save_proba", T + "p"], ["--proba", "--heat", "TUM", "XX"],
    ["--knn", "5"], ["--knn_bank", T + "bank.npz"], ["--knn_per_class", "3"], ["--similar_k", "4"], ["--similar_json", T + "s.json"],
    ["--save_embeddings", T + "e.npz", "--random_sampler"], ["--prototypes", T + "exists", "--ondisk"], ["--clusters", "3", "--tta", "d4"],
    ["--load_clusters", T + "exists", "--proba"], ["--pca", "3", "--proba"], ["--load_pca", T + "exists", "--tta", "flips"],
    ["--knn", "5", "--knn_bank", T + "good.npz", "--proba"], ["--similar_to", "1,1", "--random_sampler"], ["--similar_to", "1,1", "--ondisk"],
    ["--prototypes", T + "missing.npz"],
    ["--clusters", "0"], ["--clusters", "65"], ["--load_clusters", T + "exists", "--save_clusters", T + "s.npz"],
    ["--load_clusters", T + "exists", "--cluster_seed", "0"], ["--load_clusters", T + "exists", "--cluster_init", "maximin"],
    ["--load_clusters", T + "missing.npz"], ["--save_clusters", T + "s.npz"], ["--cluster_seed", "0"], ["--cluster_init", "maximin"],
    ["--clusters", "3", "--min_region", "4"], ["--load_clusters", T + "exists", "--min_region", "4"],
    ["--pca", "0"], ["--pca", "65"], ["--load_pca", T + "exists", "--pca", "3"], ["--load_pca", T + "exists", "--save_pca", T + "s.npz"],
    ["--load_pca", T + "missing.npz"], ["--save_pca", T + "s.npz"],
    ["--knn", "0", "--knn_bank", T + "good.npz"], ["--knn", "64", "--knn_bank", T + "good.npz"],
    ["--knn", "5", "--knn_bank", T + "good.npz", "--knn_per_class", "10"],
    ["--anno", T + "good.json", "--knn", "5", "--knn_bank", T + "new.npz", "--knn_per_class", "0"],
    ["--knn", "5", "--knn_bank", T + "good.npz", "--clusters", "3"], ["--knn", "5", "--knn_bank", T + "good.npz", "--load_clusters", T + "exists"],
    ["--knn", "5", "--knn_bank", T + "good.npz", "--min_region", "4"], ["--knn", "5", "--knn_bank", T + "missing.npz"],
    ["--knn", "5", "--knn_bank", T + "other_format.npz"], ["--knn", "5", "--knn_bank", T + "three.npz"],
    ["--knn", "5", "--knn_bank", T + "narrow.npz"], ["--knn", "5", "--knn_bank", T + "good.npz", "--arch", "resnet50"],
    ["--knn", "5", "--knn_bank", T + "three.npz", "--weights", T + "some.pth"],
    ["--similar_to", "12"], ["--similar_to", "a,b"], ["--similar_to", "300,10"], ["--similar_to", "10,420"], ["--similar_to=-1,10"],
    ["--similar_to=-1,10", "--pyramid"], ["--similar_to", "10,10", "--similar_k", "64"], ["--similar_to", "10,10", "--similar_k", "0"],
    ["--fine", "--random_sampler"], ["--fine", "--ondisk"], ["--fine", "--tta", "d4"], ["--fine", "--save_embeddings", T + "e.npz"],
    ["--fine", "--prototypes", T + "exists"], ["--fine", "--clusters", "3"], ["--fine", "--load_clusters", T + "exists"], ["--fine", "--pca", "3"],
    ["--fine", "--load_pca", T + "exists"], ["--fine", "--knn", "5", "--knn_bank", T + "good.npz"], ["--fine", "--similar_to", "10,10"],
    ["--fine", "--patch_size", "100"],
    ["--score_tolerance", "4"], ["--surface"], ["--anno", T + "good.json", "--score_tolerance", "-1"], ["--distance_json", T + "d.json"],
    ["--margin", "TUM:5", "--clusters", "2"], ["--anno", T + "good.json", "--surface", "--load_clusters", T + "exists"],
    ["--anno", T + "good.json", "--score_tolerance", "3", "--clusters", "2"],
    ["--margin", "TUM"], ["--margin", "TUM:"], ["--margin", "XYZ:5"], ["--margin", "TUM:a"], ["--margin", "TUM:5,b"], ["--margin", "TUM:0"],
    ["--margin", "TUM:-5"], ["--margin", "TUM:5,5"], ["--margin", "TUM:100,50"],
]

DOUBLE = [   # two broken rules of different groups: the order of the checks decides the message
    ["--fine", "--tta", "d4", "--clusters", "3"], ["--knn", "5", "--clusters", "3", "--min_region", "4"],
    ["--margin", "X:5", "--clusters", "2"], ["--quality_fill", "TUM", "--tissue", "otsu", "--tissue_fill", "BG", "--ondisk"],
    ["--clean_rounds", "2", "--pyramid", "--ondisk"], ["--min_region", "0", "--stain_target", T + "fit.json"],
    ["--pyramid", "--ondisk", "--stain", "macenko"], ["--stain_target", T + "fit.json", "--tissue", "foo"],
    ["--tissue", "otsu", "--random_sampler", "--quality_json", T + "q.json"], ["--quality_json", T + "q.json", "--tta", "d4", "--ondisk"],
    ["--tta", "d4", "--ondisk", "--score_json", T + "s.json"], ["--score_json", T + "s.json", "--heat", "TUM"], ["--heat", "TUM", "--knn", "5"],
    ["--save_proba", T + "p", "--fine", "--patch_size", "100"], ["--clusters", "0", "--fine"], ["--fine", "--patch_size", "100", "--margin", "TUM"],
    ["--pca", "0", "--surface"], ["--knn", "64", "--knn_bank", T + "good.npz", "--distance_json", T + "d.json"], ["--similar_to", "12", "--fine"],
    ["--save_pca", T + "s.npz", "--margin", "XYZ:5"], ["--clusters", "3", "--proba", "--heat", "XX"],
    ["--save_embeddings", T + "e.npz", "--tta", "d4", "--fine"], ["--min_sharpness", "-1", "--anno", T + "missing.json"],
    ["--stain", "macenko", "--ondisk", "--tissue", "otsu"], ["--load_clusters", T + "missing.npz", "--load_pca", T + "missing.npz"],
    ["--knn_per_class", "3", "--similar_k", "4"], ["--anno", T + "unknown.json", "--min_region", "0"],
    ["--pca", "3", "--random_sampler", "--tissue", "otsu"], ["--margin", "TUM:5,5", "--pca", "65"],
    # an out-of-range count beside a refused route: --clusters 0 counts as off and reaches its range check, the others do not
    ["--clusters", "0", "--tta", "d4"], ["--clusters", "0", "--random_sampler"], ["--clusters", "0", "--proba"], ["--pca", "0", "--tta", "d4"],
    ["--knn", "0", "--knn_bank", T + "good.npz", "--proba"], ["--clusters", "65", "--ondisk"],
]

WHOLE = [["--pyramid", "--image", "slide.psi", "--weights", ""]]   # without BASE: a slide that is not --synthetic
FOREIGN = [["--tta", "flips", "--random_sampler"]]   # with a module that is no ResNetHIP injected into main

PASSING = [
    [], ["--margin", "TUM:5"], ["--margin", "BG:-10,0,20,300"], ["--similar_to", "10,20"], ["--similar_to", "299,419", "--similar_k", "63"],
    ["--tta", "flips"], ["--tta", "d4", "--random_sampler"], ["--tissue", "40", "--tissue_min_fraction", "0.5"],
    ["--tissue", "otsu", "--tissue_fill", "BG", "--min_sharpness", "100", "--max_ink", "0.5", "--quality_fill", "BG", "--quality_json", T + "q.json"],
    ["--quality_fill", "-1"], ["--stain", "macenko", "--save_stain_fit", T + "fit.json"], ["--pyramid", "--layer", "2", "--similar_to", "900,10"],
    ["--anno", T + "good.json", "--score_json", T + "s.json", "--knn", "5", "--knn_bank", T + "new.npz", "--knn_per_class", "3"],
    ["--anno", T + "good.json", "--prototypes", T + "new.npz", "--score_tolerance", "0", "--surface", "--distance_json", T + "d.json"],
    ["--clusters", "1"], ["--clusters", "64", "--cluster_seed", "3", "--cluster_init", "maximin", "--save_clusters", T + "s.npz"],
    ["--pca", "64", "--save_pca", T + "s.npz"], ["--knn", "63", "--knn_bank", T + "good.npz"], ["--load_pca", T + "exists"],
    ["--load_clusters", T + "exists", "--regions_json", T + "r.json"], ["--fine", "--proba", "--heat", "TUM", "--min_region", "4", "--clean_rounds", "2"],
    ["--prototypes", T + "exists", "--save_embeddings", T + "e.npz"],
]


def make_files(tmp: Path) -> None:
    """The files the table's command lines name below {tmp}; what they call missing or new is not made."""
    import numpy as np
    import torch

    from deephisto_amd.neighbours import KNNClassifier
    square = [[10, 10], [10, 200], [200, 200], [200, 10]]
    (tmp / "good.json").write_text(json.dumps([dict({"class": "TUM"}, vertices=square), dict({"class": "other"}, vertices=square)]))
    (tmp / "unknown.json").write_text(json.dumps([dict({"class": "other"}, vertices=square)]))
    (tmp / "no_class.json").write_text(json.dumps([dict(vertices=square)]))
    (tmp / "number.json").write_text("5")
    (tmp / "garbage.txt").write_text("nope")
    (tmp / "exists").write_text("")
    for name, n_classes, width in (("good.npz", 5, 512), ("three.npz", 3, 512), ("narrow.npz", 5, 64)):
        knn = KNNClassifier(n_classes)
        knn.bank, knn.labels, knn.counts = torch.zeros((2, width)), torch.zeros(2, dtype=torch.int32), np.zeros(n_classes, np.int64)
        knn.save(tmp / name)
    with open(tmp / "other_format.npz", "wb") as f:
        np.savez(f, meta=np.array(json.dumps(dict(format="something else"))))


def _plain(obj):
    """The scalar attributes of a filter, or None."""
    return None if obj is None else {k: v for k, v in sorted(vars(obj).items()) if isinstance(v, (bool, int, float, str, type(None)))}


def replay(module, argv: list[str], tmp: Path, foreign_model: bool = False) -> dict:
    """One row of the table: the argv through `_build_parser` and `_check_args` of `module`."""
    import torch
    spelled = [a.replace("{tmp}", str(tmp)) for a in argv]
    model = torch.nn.Identity() if foreign_model else None
    ap = module._build_parser()
    ap.prog = PROG
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            args = ap.parse_args(spelled)
            module._check_args(ap, args, model)
    except SystemExit:
        return dict(argv=argv, foreign_model=foreign_model, error=err.getvalue().replace(str(tmp), "{tmp}").splitlines()[-1], values=None)
    values = dict(margin_spec=args.margin_spec and [args.margin_spec[0], list(args.margin_spec[1])],
                  similar_yx=args.similar_yx and list(args.similar_yx), tta_is_none=args.tta_aug is None,
                  stain_is_none=args.stain_norm is None, n_anno_records=None if args.anno_records is None else len(args.anno_records),
                  tissue_filter=_plain(args.tissue_filter), quality_filter=_plain(args.quality_filter))
    return dict(argv=argv, foreign_model=foreign_model, error=None, values=values)


if __name__ == "__main__":
    import os
    sys.path.insert(0, "")
    os.environ["COLUMNS"] = "80"   # argparse wraps the help text to the terminal
    module = importlib.import_module(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        make_files(Path(tmp))
        rows = [replay(module, BASE + extra, Path(tmp)) for extra in SINGLE + DOUBLE + PASSING]
        rows += [replay(module, argv, Path(tmp)) for argv in WHOLE] + [replay(module, BASE + extra, Path(tmp), True) for extra in FOREIGN]
    Path(sys.argv[2]).write_text(json.dumps(rows, indent=1) + "\n")
    ap = module._build_parser()
    ap.prog = PROG
    if len(sys.argv) > 3:
        Path(sys.argv[3]).write_text(ap.format_help())
    print(f"{len(rows)} rows, {sum(r['error'] is not None for r in rows)} refused, {len({r['error'] for r in rows}) - 1} different messages; "
          f"help text of {len(ap.format_help())} characters")
