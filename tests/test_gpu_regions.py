"""GPU: regions of a class map against the NumPy restatement `regions_np` of tests/test_regions_host.py
(`label_np`, `table_np`, `clean_np`).  Nothing here carries a tolerance: label maps, K, every table column including the
quantised confidence sum, cleaned maps and changed-cell counts are compared bit for bit."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_regions_host import CANVASES, LABELS, _dsc, blob_map, canvas, clean_round_np, label_np, table_np  # noqa: E402
from test_gpu_proba import _free_port, _model, _sampler, painted  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SHAPES = [(1, 1), (1, 4097), (4097, 1), (37, 53), (1000, 2049), (3125, 3125)]   # on and off multiples of the 64-cell tile
COLUMNS = ("cls", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x", "first")


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _differs(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} cells differ, first at {bad[:5].tolist()}"


def _confidence(shape, seed):
    """float32 in [0, 1] with values whose product with 2^32 has a fraction, exact halves, 0 and 1."""
    rng = np.random.default_rng(seed)
    c = rng.random(shape, dtype=np.float32)
    flat = c.reshape(-1)
    flat[::7] *= np.float32(2.0 ** -20)
    flat[::11] = np.float32(2.0 ** -33) * rng.integers(0, 8, flat[::11].shape).astype(np.float32)   # k / 2 after scaling
    flat[::13] = 1.0
    flat[::17] = 0.0
    return c


def _same_table(got, want, conf):
    for name in COLUMNS:
        g, w = getattr(got, name), want[name]
        assert g.dtype == w.dtype and np.array_equal(g, w), f"column {name}: {int((g != w).sum())} rows differ"
    if conf:
        assert got.conf_q.dtype == np.uint64 and np.array_equal(got.conf_q, want["conf_q"]), "conf_q differs"
    else:
        assert got.conf_q is None


# ---- 1. labels, K, table ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", CANVASES)
def test_labels_count_and_table_equal_the_restatement(dev, kind, shape):
    from deephisto_amd import regions
    m, n_cls = canvas(kind, shape)
    conf = _confidence(shape, 3)
    want, want_k = label_np(m)
    pred = torch.from_numpy(m).to(dev)
    labels, k = regions.label_components(pred, n_cls)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == shape and labels.is_cuda
    got = labels.cpu().numpy()
    assert k == want_k, (k, want_k)
    assert np.array_equal(got, want), _differs(got, want)
    table = regions.region_table(pred, labels, k, torch.from_numpy(conf).to(dev))
    ref = table_np(m, want, want_k, conf)
    assert len(table) == k and table.shape == shape
    _same_table(table, ref, True)
    assert int(table.area.sum()) == int((m >= 0).sum())
    _same_table(regions.region_table(pred, labels, k), ref, False)
    again, k2 = regions.label_components(pred)       # the default class range, the scratch reused
    assert k2 == k and torch.equal(again, labels)
    assert torch.equal(pred.cpu(), torch.from_numpy(m))


# ---- 2. cleanup ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", CANVASES)
def test_cleanup_equals_the_restatement(dev, kind, shape):
    from deephisto_amd import regions
    m, n_cls = canvas(kind, shape)
    pred = torch.from_numpy(m).to(dev)
    for min_cells in (2, 9, 200):
        cur, total, after = m, 0, {}
        for r in (1, 2, 3):                           # the restatement round by round: rounds = 1 is the first of rounds = 3
            out, changed = clean_round_np(cur, min_cells)
            if changed:
                cur, total = out, total + changed
            after[r] = (cur, total)
            if not changed:
                after.update({q: (cur, total) for q in range(r, 4)})
                break
        for rounds in (1, 3):
            got, n_changed = regions.clean_map(pred, min_cells, rounds, n_cls)
            want, want_changed = after[rounds]
            assert got.dtype == torch.int64 and got.data_ptr() != pred.data_ptr()
            assert n_changed == want_changed, (min_cells, rounds, n_changed, want_changed)
            g = got.cpu().numpy()
            assert np.array_equal(g, want), f"min_cells {min_cells} rounds {rounds}: " + _differs(g, want)
            assert np.array_equal((g == -1), (m == -1))
    assert torch.equal(pred.cpu(), torch.from_numpy(m)), "clean_map modified its input"


@pytest.mark.timeout(120)
def test_min_cells_one_returns_the_input_and_the_vote_width_defaults_to_the_map(dev):
    from deephisto_amd import regions
    m, n_cls = canvas("noise5_gaps", (300, 411))
    pred = torch.from_numpy(m).to(dev)
    same, changed = regions.clean_map(pred, 1, 3)
    assert changed == 0 and torch.equal(same, pred) and same.data_ptr() != pred.data_ptr()
    want, want_changed = clean_round_np(m, 4)
    got, n_changed = regions.clean_map(pred, 4)       # n_classes from the map
    assert n_changed == want_changed > 0 and np.array_equal(got.cpu().numpy(), want)
    got, n_changed = regions.clean_map(m, 4, n_classes=64)   # a NumPy map is uploaded
    assert n_changed == want_changed and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.timeout(120)
def test_out_of_range_class_is_refused(dev):
    from deephisto_amd import regions
    from deephisto_amd._lib import DeephistoHipError
    m, n_cls = canvas("patch7", (200, 333))
    want, want_k = label_np(m)
    for bad in (5, -2, 1 << 40):
        p = torch.from_numpy(m).to(dev)
        p[64, 128] = bad                               # on a tile border, among cells of its own kind
        p[65, 128] = bad
        with pytest.raises(DeephistoHipError, match=r"code -22.*2 cells hold a class outside \[-1, 5\)"):
            regions.label_components(p, n_cls)
        with pytest.raises(DeephistoHipError, match="outside"):
            regions.clean_map(p, 4, 1, n_cls)
    p = torch.from_numpy(m).to(dev)
    p[0, 0] = 64
    with pytest.raises(DeephistoHipError, match="outside"):
        regions.label_components(p)
    labels, k = regions.label_components(torch.from_numpy(m).to(dev), n_cls)   # usable after the refusals
    assert k == want_k and np.array_equal(labels.cpu().numpy(), want)
    with pytest.raises(ValueError, match="labels must be int32"):
        regions.region_table(torch.from_numpy(m).to(dev), labels.long(), k)
    with pytest.raises(ValueError, match="confidence must be float32"):
        regions.region_table(torch.from_numpy(m).to(dev), labels, k, torch.zeros((200, 333), dtype=torch.float64, device=dev))


# ---- 3. polygons back through the merged rasteriser --------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("layer,d,shape,seed", [(2, 16, (200, 260), 1), (1, 10, (411, 333), 2), (3, 7, (96, 120), 3)])
def test_exported_rings_rasterise_back_to_the_class_map(dev, tmp_path, layer, d, shape, seed):
    from deephisto_amd import regions, scoring
    m = blob_map(shape[0], shape[1], seed)
    res = regions.extract_regions(torch.from_numpy(m).to(dev), _dsc(), layer, d)
    assert res.k >= 8 and res.n_changed == 0 and res.trace_s > 0 and sorted(res.polygons) == list(range(1, res.k + 1))
    for outer, holes in res.polygons.values():        # the precondition: hole-free, no ring that touches itself
        assert holes == [] and len({tuple(v) for v in outer}) == len(outer)
    path = regions.export_annotation(tmp_path / "pred.json", res.regions, res.polygons, _dsc())
    h, w = shape[0] * d + d // 2, shape[1] * d + d - 1   # the canvas is h // d x w // d
    xy, start, cls, info = scoring.annotation_rings(path, _dsc(), layer, h, w)
    assert info == dict(n_rings=res.k, n_regions=res.k, skipped_class=0, failed=0)
    back = scoring.rasterize_rings(xy, start, cls, 5, shape[0], shape[1], d, dev).cpu().numpy()
    assert np.array_equal(back[m >= 0], m[m >= 0]) and (back[m < 0] == -1).all(), _differs(back, m)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("with_tissue", [False, True])
def test_extract_regions_after_predict_full_patched(dev, with_tissue):
    from deephisto_amd import regions
    from deephisto_amd.examples.predict_full_patched import extract_regions, predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    h, w, d, P, S, B, layer = 1100, 1300, 16, 224, 112, 16, 2
    model = _model("resnet18", "bf16", dev)
    smp = _sampler(painted(h, w, 7), P, S, B, dev)
    tissue = TissueFilter("otsu", fill_class=-1) if with_tissue else None
    pred, proba = predict_full_patched(smp, model, 5, downscale=d, tissue=tissue, return_proba=True)
    before = pred.clone()
    m = pred.cpu().numpy()
    assert ((m == -1).any()) == with_tissue
    res = extract_regions(pred, _dsc(), layer, d, confidence=proba.confidence)
    want, want_k = label_np(m)
    assert res.k == want_k and np.array_equal(res.labels.cpu().numpy(), want) and torch.equal(res.class_map, pred)
    _same_table(res.regions, table_np(m, want, want_k, proba.confidence.cpu().numpy()), True)
    assert int(res.regions.area.sum()) == int((m >= 0).sum())
    conf = res.regions.mean_confidence
    assert np.all((conf >= 0) & (conf <= 1))
    # a SlideProbabilities: its own class map and confidence
    res_p = extract_regions(proba, _dsc(), layer, d, polygons=False)
    mp = proba.class_map.cpu().numpy()
    lab_p, k_p = label_np(mp)
    assert res_p.polygons is None and res_p.k == k_p
    _same_table(res_p.regions, table_np(mp, lab_p, k_p, proba.confidence.cpu().numpy()), True)
    # cleaned
    res_c = extract_regions(pred, _dsc(), layer, d, min_cells=6, rounds=3)
    cur, total = m, 0
    for _ in range(3):
        out, changed = clean_round_np(cur, 6)
        if not changed:
            break
        cur, total = out, total + changed
    assert res_c.n_changed == total and np.array_equal(res_c.class_map.cpu().numpy(), cur)
    assert res_c.k == label_np(cur)[1] <= res.k
    assert torch.equal(pred, before)
    assert json.loads(json.dumps(res_c.records(_dsc(), d, layer)))[0]["class"] in LABELS


def _bytes(folder):
    return {p.name: p.read_bytes() for p in sorted(Path(folder).iterdir())}


@pytest.mark.timeout(1500)
def test_cli_region_flags_leave_the_map_alone_and_two_ranks_equal_one(dev, tmp_path):
    from deephisto_amd import scoring
    from deephisto_amd.examples.predict_full_patched import main
    h, w = 1500, 1300
    args = ["--synthetic", str(h), str(w), "--weights", "", "--patch_size", "224", "--stride", "112", "--batch_size", "16",
            "--compute_dtype", "bf16"]
    stem = f"synthetic_{h}x{w}"
    pred0 = main(args + ["--out_dir", str(tmp_path / "plain")])

    def with_dir(folder):
        return ["--out_dir", str(folder), "--regions_json", str(folder / "r.json"), "--min_region", "5", "--clean_rounds", "2",
                "--export_anno", str(folder / "a.json")]

    pred1 = main(args + with_dir(tmp_path / "one"))
    assert torch.equal(pred1, pred0)
    plain, one = _bytes(tmp_path / "plain"), _bytes(tmp_path / "one")
    assert sorted(plain) == sorted([f"{stem}.jpg", f"{stem}_mask.jpg", f"{stem}_overlay.jpg"])
    assert sorted(one) == sorted([*plain, f"{stem}_clean_mask.jpg", f"{stem}_clean_overlay.jpg", "r.json", "a.json"])
    for f in plain:
        assert one[f] == plain[f], f"{f} changed with the region flags"
    m = pred0.cpu().numpy()
    cur = m
    total = 0
    for _ in range(2):
        out, changed = clean_round_np(cur, 5)
        if not changed:
            break
        cur, total = out, total + changed
    lab, k = label_np(cur)
    table = json.loads(one["r.json"])
    assert table["n_regions"] == k == len(table["regions"]) and table["shape"] == list(m.shape) and table["n_changed"] == total
    assert sum(r["area_cells"] for r in table["regions"]) == int((m >= 0).sum())
    anno = json.loads(one["a.json"])
    assert len(anno) == k and all(set(a) >= {"class", "vertices", "holes"} and a["class"] in LABELS for a in anno)
    assert [a["class"] for a in anno] == [r["class"] for r in table["regions"]]
    # with --anno: the uncleaned map's score first, the cleaned map's second
    (tmp_path / "truth.json").write_text(json.dumps(scoring.synthetic_annotation(h, w, 25, 90, LABELS, seed=2, layer=2)))
    # two ranks sharing cuda:0 over gloo write the single-process files
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}", DH_DIST_BACKEND="gloo", DH_SHARE_GPU="1")
    (tmp_path / "run2.py").write_text("import sys\nfrom examples.predict_full_patched import main\nmain(sys.argv[1:])\n")
    cmd = ["timeout", "-k", "10", "840", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "run2.py"), *args,
           *with_dir(tmp_path / "two"), "--anno", str(tmp_path / "truth.json")]
    r = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    two = _bytes(tmp_path / "two")
    assert sorted(two) == sorted([*one, f"{stem}_truth.jpg", f"{stem}_errors.jpg"])
    for f in one:
        assert two[f] == one[f], f"{f}: two ranks differ from one process"
    assert r.stdout.count("accuracy") == 2 and "cleaned map:" in r.stdout and f"regions: {k}" in r.stdout
