"""GPU: scoring a class map against a polygon annotation against the NumPy restatements `rasterize_np` and
`confusion_np` of tests/test_score_host.py.  Nothing here carries a tolerance: label maps, confusion matrices and outcome maps are
compared cell for cell and count for count."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_score_host import LABELS, _dsc, _pack, confusion_np, packed_cases, rasterize_np  # noqa: E402
from test_gpu_proba import CONFIGS, _model, _sampler, painted  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rings_of(records, layer):
    rings = [np.asarray(r["vertices"], np.float64) / layer for r in records]
    return _pack(rings, [LABELS.index(r["class"]) for r in records])


def _differs(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} cells differ, first at {bad[:5].tolist()}"


# ---- 1. the rasteriser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(packed_cases()))
def test_rasteriser_equals_the_restatement_on_the_host_cases(dev, name):
    from deephisto_amd import scoring
    xy, start, cls, n_cls, dh, dw, d = packed_cases()[name]
    want = rasterize_np(xy, start, cls, n_cls, dh, dw, d)
    got = scoring.rasterize_rings(xy, start, cls, n_cls, dh, dw, d, dev)
    assert got.dtype == torch.int32 and tuple(got.shape) == (dh, dw) and got.is_cuda
    got = got.cpu().numpy()
    assert np.array_equal(got, want), _differs(got, want)
    again = scoring.rasterize_rings(xy, start, cls, n_cls, dh, dw, d, dev).cpu().numpy()   # the kept plan
    assert np.array_equal(again, want)


def test_rasteriser_slide_scale_many_rings_per_bin_and_empty_bins(dev):
    """200 seeded rings of 1 000 non-integer vertices on a 3125 x 3125 canvas (a 50 000^2 layer at d = 16)."""
    from deephisto_amd import scoring
    h = w = 50000
    d = 16
    xy, start, cls = _rings_of(scoring.synthetic_annotation(h, w, 200, 1000, LABELS, seed=11), 1)
    assert len(cls) == 200 and len(xy) == 200_000
    want = rasterize_np(xy, start, cls, 5, h // d, w // d, d)
    got = scoring.rasterize_rings(xy, start, cls, 5, h // d, w // d, d, dev).cpu().numpy()
    assert np.array_equal(got, want), _differs(got, want)
    # what the case claims: bins of 32 x 32 cells that many rings reach, bins none reaches, overlaps of two classes
    rings = [xy[start[r]:start[r + 1]] / d for r in range(200)]
    x0, x1 = np.array([r[:, 0].min() for r in rings]), np.array([r[:, 0].max() for r in rings])
    y0, y1 = np.array([r[:, 1].min() for r in rings]), np.array([r[:, 1].max() for r in rings])
    bins = np.arange(0, 3125, 32)
    reach = ((x0[:, None, None] < bins[None, None, :] + 32) & (x1[:, None, None] > bins[None, None, :])
             & (y0[:, None, None] < bins[None, :, None] + 32) & (y1[:, None, None] > bins[None, :, None])).sum(axis=0)
    assert reach.max() >= 4 and (reach == 0).sum() >= 10
    labelled = (want >= 0).sum()
    assert 0.1 * want.size < labelled < 0.9 * want.size and len(np.unique(want)) == 6


@pytest.mark.parametrize("layer,h,w,d", [(2, 3000, 4100, 16), (2, 999, 1237, 10), (1, 2047, 1531, 7)])
def test_rasteriser_float_vertices_through_the_annotation_parser(dev, layer, h, w, d, tmp_path):
    """Non-integer float64 vertices scaled by the layer: only the shared float64 rule decides.  The device reads the parser's rings."""
    from deephisto_amd import scoring
    records = scoring.synthetic_annotation(h, w, 40, 257, LABELS + ["OTHER"], seed=h, layer=layer)
    path = tmp_path / "anno.json"
    path.write_text(json.dumps(records))
    xy, start, cls, info = scoring.annotation_rings(records, _dsc(), layer, h, w)
    assert info["skipped_class"] > 0 and info["failed"] == 0 and info["n_rings"] == len(cls) > 20
    assert (xy != np.rint(xy)).mean() > 0.9
    want = rasterize_np(xy, start, cls, 5, h // d, w // d, d)
    got, info2 = scoring.rasterize_annotation(path, _dsc(), layer, h, w, d, dev)
    assert info2 == info
    got = got.cpu().numpy()
    assert np.array_equal(got, want), _differs(got, want)
    assert (want >= 0).any() and (want == -1).any()


def test_rasteriser_without_rings_is_all_unlabelled(dev):
    from deephisto_amd import scoring
    got = scoring.rasterize_rings(np.zeros((0, 2)), [0], [], 5, 77, 130, 16, dev)
    assert tuple(got.shape) == (77, 130) and (got == -1).all()
    got, info = scoring.rasterize_annotation([{"class": "NOPE", "vertices": [[0, 0], [50, 0], [50, 50]]}], _dsc(), 1, 640, 640, 16, dev)
    assert (got == -1).all() and info == dict(n_rings=0, n_regions=0, skipped_class=1, failed=0)


# ---- 2. the confusion matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cls", [1, 5, 64])
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (1000, 2049), (3125, 3125)])
def test_confusion_equals_the_restatement(dev, n_cls, shape):
    from deephisto_amd import scoring
    rng = np.random.default_rng(n_cls * 1000 + shape[1])
    truth = rng.integers(-1, n_cls, shape).astype(np.int32)
    pred = rng.integers(-1, n_cls, shape).astype(np.int64)
    if shape[0] > 100:   # patches of one pair, as class maps have them, and a run of unlabelled cells
        truth[: shape[0] // 2, : shape[1] // 3] = n_cls - 1
        pred[: shape[0] // 3] = 0
        truth[-7:] = -1
    want, want_outcome = confusion_np(pred, truth, n_cls)
    got, outcome = scoring.confusion(torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev), n_cls, return_outcome=True)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n_cls, n_cls + 1)
    assert np.array_equal(got.numpy(), want), (got.numpy() - want)
    assert outcome.dtype == torch.int64 and np.array_equal(outcome.cpu().numpy(), want_outcome)
    assert int(got.sum()) == int((truth >= 0).sum())
    only = scoring.confusion(torch.from_numpy(pred).to(dev), torch.from_numpy(truth).to(dev), n_cls)
    assert np.array_equal(only.numpy(), want)


def test_confusion_all_unlabelled_and_out_of_range(dev):
    from deephisto_amd import scoring
    from deephisto_amd._lib import DeephistoHipError
    pred = torch.randint(-1, 5, (123, 457), device=dev)
    none = torch.full((123, 457), -1, dtype=torch.int32, device=dev)
    counts, outcome = scoring.confusion(pred, none, 5, return_outcome=True)
    assert not counts.any() and (outcome == -1).all()
    truth = torch.randint(-1, 5, (123, 457), device=dev).to(torch.int32)
    for bad in (5, -2, 1 << 40):
        p = pred.clone()
        p[77, 300] = bad
        with pytest.raises(DeephistoHipError, match=r"1 predictions outside \[-1, 5\)"):
            scoring.confusion(p, truth, 5)
    p = pred.clone()
    p[0, 0] = 7
    with pytest.raises(DeephistoHipError, match="outside"):   # refused where the truth is unlabelled as well: not a silent drop
        scoring.confusion(p, none, 5)
    want, _ = confusion_np(pred.cpu().numpy(), truth.cpu().numpy(), 5)
    assert np.array_equal(scoring.confusion(pred, truth, 5).numpy(), want)   # usable after the refusals


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def _check(score, pred, truth_want, what):
    want, _ = confusion_np(pred.cpu().numpy() if isinstance(pred, torch.Tensor) else pred, truth_want, 5)
    assert np.array_equal(score.confusion, want), what
    assert score.labels == LABELS and score.n_cells == truth_want.size and score.n_labelled == int((truth_want >= 0).sum())
    return want


@pytest.mark.parametrize("arch,dtype", CONFIGS)
def test_score_prediction_end_to_end(dev, arch, dtype):
    from deephisto_amd import scoring, tiles
    from deephisto_amd.examples.predict_full_patched import predict_full_patched, predict_random_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    from deephisto_amd.tissue import TissueFilter
    h, w, d, P, S, B, layer = 1100, 1300, 16, 224, 112, 16, 2
    records = scoring.synthetic_annotation(h, w, 30, 120, LABELS, seed=5, layer=layer)
    xy, start, cls, _ = scoring.annotation_rings(records, _dsc(), layer, h, w)
    truth_want = rasterize_np(xy, start, cls, 5, h // d, w // d, d)
    assert (truth_want >= 0).sum() > 500
    model = _model(arch, dtype, dev)
    smp = _sampler(painted(h, w, 7), P, S, B, dev)
    cmap, proba = predict_full_patched(smp, model, 5, downscale=d, return_proba=True)
    score, truth, outcome, info = scoring.score_prediction(cmap, records, _dsc(), layer, h, w, d, return_maps=True)
    assert np.array_equal(truth.cpu().numpy(), truth_want) and info["n_rings"] == len(cls)
    want = _check(score, cmap, truth_want, "dense")
    assert score.n_unclassified == 0 and want.sum() > 0
    assert np.array_equal(outcome.cpu().numpy(), confusion_np(cmap.cpu().numpy(), truth_want, 5)[1])
    plain = scoring.score_prediction(cmap.cpu().numpy(), records, _dsc(), layer, h, w, d)   # process()'s NumPy map
    assert np.array_equal(plain.confusion, want) and plain.to_dict() == score.to_dict()
    # a SlideProbabilities: its class map (the argmax of the mean probability) is what is scored
    _check(scoring.score_prediction(proba, records, _dsc(), layer, h, w, d), proba.class_map, truth_want, "proba")
    # the tissue filter leaves labelled cells without a prediction: the last column
    cmap_t = predict_full_patched(smp, model, 5, downscale=d, tissue=TissueFilter("otsu", fill_class=-1))
    score_t = scoring.score_prediction(cmap_t, records, _dsc(), layer, h, w, d)
    _check(score_t, cmap_t, truth_want, "tissue")
    assert score_t.n_unclassified > 0 and score_t.n_unclassified == int(((cmap_t.cpu().numpy() == -1) & (truth_want >= 0)).sum())
    # the random sampler's map
    rnd = FullImageRndSampler(tiles.synth_slide(h, w, 4, dev), layer=1, patch_size=P, batch_size=32, dense_level=1, speedup=d,
                              index_logic="device")
    np.random.seed(17)
    cmap_r = predict_random_patched(rnd, model, 5, d)
    _check(scoring.score_prediction(cmap_r, records, _dsc(), layer, h, w, d), cmap_r, truth_want, "random")
    with pytest.raises(ValueError, match="the class map is"):
        scoring.score_prediction(cmap[:, :-1], records, _dsc(), layer, h, w, d)


def test_cli_scores_and_leaves_the_class_map_alone(dev, tmp_path, capsys):
    from PIL import Image

    from deephisto_amd import scoring
    from deephisto_amd.examples.predict_full_patched import main
    h, w = 1500, 1300
    records = scoring.synthetic_annotation(h, w, 25, 90, LABELS + ["OTHER"], seed=2, layer=2)
    anno = tmp_path / "anno.json"
    anno.write_text(json.dumps(records))
    args = ["--synthetic", str(h), str(w), "--weights", "", "--patch_size", "224", "--stride", "112", "--batch_size", "16",
            "--compute_dtype", "bf16"]
    pred0 = main(args + ["--out_dir", str(tmp_path / "plain")])
    capsys.readouterr()
    pred1 = main(args + ["--out_dir", str(tmp_path / "scored"), "--anno", str(anno), "--score_json", str(tmp_path / "scored" / "s.json")])
    printed = capsys.readouterr().out
    assert torch.equal(pred1, pred0)
    stem = f"synthetic_{h}x{w}"
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted([f"{stem}.jpg", f"{stem}_mask.jpg", f"{stem}_overlay.jpg"])
    for f in (f"{stem}_truth.jpg", f"{stem}_errors.jpg"):
        with Image.open(tmp_path / "scored" / f) as im:
            assert im.size == (w // 16, h // 16) and im.mode == "RGB", f
    want = scoring.score_prediction(pred0, records, _dsc(), 2, h, w, 16)
    saved = json.loads((tmp_path / "scored" / "s.json").read_text())
    assert saved["confusion"] == want.confusion.tolist() and saved["labels"] == LABELS and want.n_labelled > 0
    assert saved["annotation"]["skipped_class"] > 0 and saved["annotation"]["n_rings"] > 0
    assert {k: v for k, v in saved.items() if k != "annotation"} == want.to_dict()
    assert str(want) in printed and "accuracy" in printed
    # the truth picture holds the class colours where the label map has a class, black elsewhere (JPEG: approximately)
    truth, _ = scoring.rasterize_annotation(records, _dsc(), 2, h, w, 16, dev)
    with Image.open(tmp_path / "scored" / f"{stem}_truth.jpg") as im:
        rgb = np.asarray(im).astype(np.int64)
    assert (rgb.sum(axis=2) > 60).mean() == pytest.approx((truth >= 0).float().mean().item(), abs=0.05)
