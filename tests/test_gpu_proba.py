"""GPU: whole-slide probability maps against the NumPy restatement `proba_np` of tests/test_proba_host.py.

Only the softmax carries a tolerance (a multiple of torch-CPU float32's own error against float64).  Sums, counts and the finish
are compared bit for bit: the device's own softmax rows are read back and fed to the float32 NumPy loop.  End to end the device is
held to a multiple of the float32 restatement's error against the float64 one."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_proba_host import brute_count, proba_np  # noqa: E402

from oracle import random_sampler, synth, tiling  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
CONFIGS = [("resnet18", "f32"), ("resnet18", "bf16"), ("resnet50", "bf16")]
# name: h, w, patch, stride, batch, downscale
GRIDS = {
    "4096_224_112_b64": (4096, 4096, 224, 112, 64, 16),        # 48 padding duplicates of the corner
    "4096_256_256_b64": (4096, 4096, 256, 256, 64, 16),
    "1000x1300_256_256_b16": (1000, 1300, 256, 256, 16, 16),
    "999x1237_64_48_b7_d10": (999, 1237, 64, 48, 7, 10),       # d divides nothing: footprints of 6 and 7 cells
}
# the dense grids cover every cell of the h//d x w//d canvas (the clamped last row and column reach it), so the count == 0 cells and
# the fill class at d = 10 come from a thinned list: every third tile of the grid above
NAMES = [*GRIDS, "999x1237_64_48_b7_d10_every_third", "random"]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _origins(name, dedupe):
    if name == "random":
        np.random.seed(5)
        h, w, P, d = 1024, 1280, 128, 16
        o = np.concatenate([b for b, _ in random_sampler.random_batches(h, w, P, 16, dense_level=2, speedup=d)])
        return h, w, P, d, o
    h, w, P, S, B, d = GRIDS[name.replace("_every_third", "")]
    o = tiling.batched_origins(h, w, P, S, B).reshape(-1, 2)
    if dedupe:
        o = o[:len(tiling.tile_origins(h, w, P, S))]
    return h, w, P, d, np.ascontiguousarray(o[::3] if name.endswith("_every_third") else o)


def _logits(n, n_cls, seed, scale):
    return (np.random.default_rng(seed).standard_normal((n, n_cls)) * scale).astype(np.float32)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    """Every field of a SlideProbabilities bit-identical to a proba_np dict or to another SlideProbabilities."""
    if not isinstance(want, dict):
        want = dict(proba=want.proba, count=want.count, class_map=want.class_map, confidence=want.confidence)
    for k in ("count", "proba", "class_map", "confidence"):
        g, w_ = _bits(getattr(got, k)), _bits(want[k])
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, w_.dtype, g.shape, w_.shape)
        assert np.array_equal(g, w_), f"{what}: {k} differs in {int((g != w_).sum())} places"


# ---- 1. softmax rows --------------------------------------------------------------------------------------------------------
def test_softmax_rows_within_the_cpu_softmax_error(dev):
    """Bound: 4 x E_ref, E_ref = max |torch-CPU float32 softmax - float64 softmax| on the same float32 logits (the device differs
    from the CPU only in expf's last bits); rows sum to 1 within that bound times n_cls."""
    from deephisto_amd import tiles
    n_cls = 5
    rows = [_logits(4096, n_cls, seed, scale) for seed in range(5) for scale in (3.0, 0.05)]
    spread = _logits(512, n_cls, 9, 1.0)
    spread[:, 0] += 80.0
    spread[:, 1] -= 80.0
    rows += [spread, np.roll(spread, 2, axis=1), np.repeat(_logits(256, 1, 10, 30.0), n_cls, axis=1),
             np.zeros((8, n_cls), np.float32)]
    x = np.concatenate(rows)
    want = torch.softmax(torch.from_numpy(x).double(), dim=1).numpy()
    e_ref = float(np.abs(torch.softmax(torch.from_numpy(x), dim=1).numpy().astype(np.float64) - want).max())
    got = tiles.softmax_rows(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    sum_err = float(np.abs(got.sum(axis=1) - 1.0).max())
    print(f"softmax rows: device error {err:.3e}, E_ref {e_ref:.3e}, |row sum - 1| {sum_err:.3e}")
    assert np.isfinite(got).all()
    assert 0 < e_ref < 1e-6
    assert err <= 4 * e_ref
    assert sum_err <= 4 * e_ref * n_cls
    equal = tiles.softmax_rows(torch.full((3, 4), 7.5, device=dev)).cpu().numpy()
    assert np.array_equal(equal, np.full((3, 4), 0.25, np.float32))


# ---- 2. sums, counts, finish: bit-exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedupe", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_sums_counts_finish_bit_exact(dev, name, dedupe):
    from deephisto_amd import tiles
    h, w, P, d, o = _origins(name, dedupe)
    n_cls, fill = 5, (-1 if dedupe else 2)
    logits = torch.from_numpy(_logits(len(o), n_cls, len(o), 3.0)).to(dev)
    probs = tiles.softmax_rows(logits).cpu().numpy()
    ref = proba_np(h, w, n_cls, d, [(P, o, probs)], softmax=False, fill=fill)
    if name == "4096_224_112_b64":
        assert ref["count"].max() == (9 if dedupe else 57) and ref["count"].min() == 1
    if name == "999x1237_64_48_b7_d10_every_third":
        assert (ref["count"] == 0).any() and (ref["class_map"] == fill).any()
    # unfused: sums and counts, then the finish in place
    st = tiles.accumulate_probabilities(logits, o, P, d, h, w, finish=False)
    assert not st.finished and st.class_map is None and st.confidence is None
    assert st.count.dtype == torch.int32 and st.proba.dtype == torch.float32
    assert np.array_equal(_bits(st.proba), _bits(ref["sum"])), "sums differ"
    assert np.array_equal(_bits(st.count), ref["count"]), "counts differ"
    st.finish(fill)
    _same(st, ref, "dh_finish_mean")
    assert st.class_map.dtype == torch.int64
    # fused: one pass
    _same(tiles.accumulate_probabilities(logits, o, P, d, h, w, fill_class=fill), ref, "fused")


@pytest.mark.parametrize("n_cls", [1, 3, 64])
def test_other_class_counts_bit_exact(dev, n_cls):
    """256 / n_cls cells per pass: 256, 85 and 4."""
    from deephisto_amd import tiles
    h, w, P, d, o = _origins("999x1237_64_48_b7_d10", False)
    logits = torch.from_numpy(_logits(len(o), n_cls, n_cls, 3.0)).to(dev)
    ref = proba_np(h, w, n_cls, d, [(P, o, tiles.softmax_rows(logits).cpu().numpy())], softmax=False)
    _same(tiles.accumulate_probabilities(logits, o, P, d, h, w), ref, "fused")
    _same(tiles.accumulate_probabilities(logits, o, P, d, h, w, finish=False).finish(), ref, "unfused")


def test_continuation_and_empty_list(dev):
    from deephisto_amd import tiles
    h, w, d, n_cls = 1000, 1300, 16, 5
    o1 = tiling.batched_origins(h, w, 224, 112, 64).reshape(-1, 2)
    o2 = tiling.batched_origins(h, w, 96, 160, 7).reshape(-1, 2)   # stride > patch: the second run leaves gaps
    l1 = torch.from_numpy(_logits(len(o1), n_cls, 1, 3.0)).to(dev)
    l2 = torch.from_numpy(_logits(len(o2), n_cls, 2, 0.05)).to(dev)
    runs = [(224, o1, tiles.softmax_rows(l1).cpu().numpy()), (96, o2, tiles.softmax_rows(l2).cpu().numpy())]
    ref = proba_np(h, w, n_cls, d, runs, softmax=False)
    st = tiles.accumulate_probabilities(l1, o1, 224, d, h, w, finish=False)
    st = tiles.accumulate_probabilities(l2, o2, 96, d, h, w, state=st)
    _same(st, ref, "two runs chained")
    # a run that starts where nothing is covered yet, continued: order of the runs matters and is kept
    ref = proba_np(h, w, n_cls, d, runs[::-1], softmax=False, fill=4)
    st = tiles.accumulate_probabilities(l2, o2, 96, d, h, w, finish=False)
    assert (st.count == 0).any()
    _same(tiles.accumulate_probabilities(l1, o1, 224, d, h, w, state=st, fill_class=4), ref, "chained, reversed")
    # an empty tile list: all fill
    empty = tiles.accumulate_probabilities(torch.empty((0, n_cls), device=dev), np.zeros((0, 2), np.int32), 224, d, h, w,
                                           fill_class=3)
    assert tuple(empty.proba.shape) == (h // d, w // d, n_cls) and not empty.proba.any() and not empty.count.any()
    assert (empty.class_map == 3).all() and not empty.confidence.any()
    # an empty list on top of a state: the finish of what the state held
    st = tiles.accumulate_probabilities(l2, o2, 96, d, h, w, finish=False)
    st = tiles.accumulate_probabilities(torch.empty((0, n_cls), device=dev), np.zeros((0, 2), np.int32), 224, d, h, w, state=st)
    _same(st, proba_np(h, w, n_cls, d, runs[1:], softmax=False), "empty list on a state")


# ---- 3. against float64 end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedupe", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_against_float64(dev, name, dedupe):
    """proba within 4 x E_mean_ref (the float32 restatement's own error against the float64 one); class_map equal wherever the
    float64 top-two gap exceeds 8 x E_mean_ref; at most 0.1 % of the covered cells may fall below that gap."""
    from deephisto_amd import tiles
    h, w, P, d, o = _origins(name, dedupe)
    n_cls = 5
    for seed, scale in ((0, 3.0), (1, 0.05)):
        x = _logits(len(o), n_cls, seed, scale)
        r64 = proba_np(h, w, n_cls, d, [(P, o, x.astype(np.float64))], dtype=np.float64)
        r32 = proba_np(h, w, n_cls, d, [(P, o, x)], dtype=np.float32)
        e_mean = float(np.abs(r32["proba"].astype(np.float64) - r64["proba"]).max())
        covered = r64["count"] > 0
        top = np.sort(r64["proba"], axis=2)
        gap = top[..., -1] - top[..., -2]
        left_out = covered & (gap <= 8 * e_mean)
        assert 0 < e_mean < 1e-5
        assert left_out.sum() <= 1e-3 * covered.sum(), f"{int(left_out.sum())} of {int(covered.sum())} cells below the gap"
        got = tiles.accumulate_probabilities(torch.from_numpy(x).to(dev), o, P, d, h, w)
        err = float(np.abs(got.proba.cpu().numpy().astype(np.float64) - r64["proba"]).max())
        print(f"{name} dedupe={dedupe} scale={scale}: device error {err:.3e}, E_mean_ref {e_mean:.3e}, "
              f"smallest gap {gap[covered].min():.3e}, left out {int(left_out.sum())}")
        assert err <= 4 * e_mean
        assert np.array_equal(got.count.cpu().numpy(), r64["count"])
        cmap = got.class_map.cpu().numpy()
        keep = covered & ~left_out
        assert np.array_equal(cmap[keep], r64["class_map"][keep])
        assert (cmap[~covered] == -1).all()
        conf = got.confidence.cpu().numpy().astype(np.float64)
        assert np.abs(conf - r64["confidence"])[keep].max() <= 4 * e_mean and not conf[~covered].any()


# ---- 4. through the predict functions ------------------------------------------------------------------------------------------
GREY = (200, 196, 198)   # chroma 4


def painted(h, w, seed):
    """Synthetic tissue with a seeded glass pattern: white columns and blocks over about half the area, a grey band."""
    host = synth.synth_slide(h, w, seed)
    rng = np.random.default_rng(seed)
    host[:, : int(w * rng.uniform(0.25, 0.35))] = 255
    for _ in range(4):
        y0, x0 = rng.integers(0, h - 100), rng.integers(0, w - 100)
        host[y0:y0 + rng.integers(50, h // 3), x0:x0 + rng.integers(50, w // 3)] = 255
    y0 = int(h * 0.6)
    host[y0:y0 + h // 8] = GREY
    return host


def _model(arch, dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(0)
    return get_model(5, dtype, arch=arch).to(dev).eval()


def _sampler(host, P, S, B, dev, **kw):
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    return FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev, **kw)


@pytest.mark.parametrize("arch,dtype", CONFIGS)
def test_predict_full_patched_return_proba(dev, arch, dtype):
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    h, w, d, P, S, B = 1100, 1300, 16, 224, 112, 16
    host = painted(h, w, 7)
    model = _model(arch, dtype, dev)
    smp = _sampler(host, P, S, B, dev)
    n_unique, origins = smp.n_tiles, smp.origins
    assert len(origins) > n_unique
    cmap0, logits0 = predict_full_patched(smp, model, 5, downscale=d, return_logits=True)
    cmap1, logits1, pr = predict_full_patched(smp, model, 5, downscale=d, return_logits=True, return_proba=True)
    assert torch.equal(cmap1, cmap0) and torch.equal(logits1, logits0)
    assert isinstance(pr, tiles.SlideProbabilities) and pr.proba.is_cuda and pr.finished
    _same(pr, tiles.accumulate_probabilities(logits1, origins, P, d, h, w), "padded list")
    _same(pr, proba_np(h, w, 5, d, [(P, origins, tiles.softmax_rows(logits1).cpu().numpy())], softmax=False), "restatement")
    cmap2, pr2 = predict_full_patched(smp, model, 5, downscale=d, return_proba=True)
    assert torch.equal(cmap2, cmap0)
    _same(pr2, pr, "without return_logits")
    cmap3, pr3 = predict_full_patched(smp, model, 5, downscale=d, dedupe_padding=True, return_proba=True)
    assert torch.equal(cmap3, predict_full_patched(smp, model, 5, downscale=d, dedupe_padding=True))
    _same(pr3, tiles.accumulate_probabilities(logits1[:n_unique].contiguous(), origins[:n_unique], P, d, h, w), "dedupe_padding")
    assert int(pr.count.max()) > int(pr3.count.max())   # the corner's duplicates are counted by default
    # tissue: the kept tiles only; uncovered cells have count 0 and the fill class
    for dedupe in (False, True):
        filt, info = TissueFilter("otsu", fill_class=3), {}
        cmap_t, logits_t, pr_t = predict_full_patched(smp, model, 5, downscale=d, return_logits=True, tissue=filt,
                                                      tissue_info=info, return_proba=True, dedupe_padding=dedupe)
        assert torch.equal(cmap_t, predict_full_patched(smp, model, 5, downscale=d, tissue=filt, dedupe_padding=dedupe))
        keep = info["kept"]
        assert 0 < len(keep) < n_unique and torch.isnan(logits_t).any()
        rows = list(keep)
        if not dedupe and keep[-1] == n_unique - 1:
            rows += list(range(n_unique, len(origins)))
        probs = tiles.softmax_rows(logits0[torch.tensor(rows, device=dev)].contiguous()).cpu().numpy()
        ref = proba_np(h, w, 5, d, [(P, origins[rows], probs)], softmax=False, fill=3)
        _same(pr_t, ref, f"tissue dedupe={dedupe}")
        assert (ref["count"] == 0).any() and not torch.isnan(pr_t.proba).any()
        assert (pr_t.class_map[pr_t.count == 0] == 3).all()


def test_all_glass_gives_all_fill_and_runs_no_forward(dev):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    white = np.full((700, 900, 3), 255, np.uint8)
    model = _model("resnet18", "bf16", dev)
    calls = []
    fwd, name = model.tiles_entry()
    model.tiles_entry = lambda: ((lambda *a: calls.append(1) or fwd(*a)), name)
    smp = _sampler(white, 224, 112, 8, dev)
    cmap, pr = predict_full_patched(smp, model, 5, downscale=16, tissue=TissueFilter("otsu", fill_class=2), return_proba=True)
    assert calls == []
    assert tuple(pr.proba.shape) == (700 // 16, 900 // 16, 5) and not pr.proba.any() and not pr.count.any()
    assert (pr.class_map == 2).all() and (cmap == 2).all() and not pr.confidence.any()
    predict_full_patched(smp, model, 5, downscale=16, return_proba=True)
    assert calls


@pytest.mark.parametrize("arch,dtype", [("resnet18", "f32"), ("resnet50", "bf16")])
def test_predict_random_patched_return_proba(dev, arch, dtype):
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import ImagePredictorPatched, predict_random_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    h, w, P, B, d = 1200, 1536, 224, 32, 16
    slide = tiles.synth_slide(h, w, 4, dev)
    m = _model(arch, dtype, dev)

    def smp():
        return FullImageRndSampler(slide, layer=1, patch_size=P, batch_size=B, dense_level=1, speedup=d, index_logic="device")

    np.random.seed(17)
    cmap, canvas, pr = predict_random_patched(smp(), m, 5, d, return_canvas=True, return_proba=True)
    np.random.seed(17)
    cmap0, canvas0 = predict_random_patched(smp(), m, 5, d, return_canvas=True)
    assert torch.equal(cmap, cmap0) and torch.equal(canvas, canvas0)
    np.random.seed(17)
    origins = np.concatenate([np.array([(p.pos_y, p.pos_x) for p in patches], np.int32) for patches, _ in smp().generator()])
    assert np.array_equal(pr.count.cpu().numpy(), brute_count(h, w, d, P, origins))
    assert int(pr.count.min()) >= 1 and int(pr.count.max()) > 4

    def cb(patches):
        o = torch.from_numpy(np.array([(p.pos_y, p.pos_x) for p in patches], np.int32)).to(dev)
        return m.forward_tiles(slide, o, P)

    np.random.seed(17)
    predictor = ImagePredictorPatched((h, w), smp().generator(), cb, 5, layer=1, downscale=d, device=dev)
    _same(predictor.process_proba(), pr, "callback route")
    np.testing.assert_array_equal(predictor.process(), cmap.cpu().numpy())   # the same pass serves the class map


def test_streamed_equals_resident(dev):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import SamplerExecutionMode
    h, w, P, S, B, d = 900, 1000, 224, 112, 16, 16
    host = synth.synth_slide(h, w, 2)
    m = _model("resnet18", "bf16", dev)
    cmap, pr = predict_full_patched(_sampler(host, P, S, B, dev), m, 5, downscale=d, return_proba=True)
    disk = _sampler(host, P, S, B, dev, mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    cmap2, pr2 = predict_full_patched(disk, m, 5, downscale=d, return_proba=True, streams=1)
    assert torch.equal(cmap2, cmap)
    _same(pr2, pr, "streamed")


def test_process_proba_without_patches(dev):
    from deephisto_amd.examples.predict_full_patched import ImagePredictorPatched
    pr = ImagePredictorPatched((320, 480), iter(()), lambda patches: None, 5, layer=1, downscale=16, device=dev).process_proba(4)
    assert tuple(pr.proba.shape) == (20, 30, 5) and (pr.class_map == 4).all() and not pr.count.any()


# ---- 5. two ranks equal one process; 6. the CLI's files ------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_proba_two_ranks_equal_single_process(dev, tmp_path):
    """`--proba --heat --save_proba` through the CLI: JPEGs and arrays written by rank 0; two ranks sharing cuda:0 over gloo save
    the single-process arrays."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import main, predict_full_patched
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    args = ["--synthetic", "1500", "1300", "--weights", "", "--patch_size", "224", "--stride", "112", "--batch_size", "16",
            "--proba", "--heat", "TUM", "BG"]
    pred1 = main(args + ["--out_dir", str(tmp_path / "one"), "--save_proba", str(tmp_path / "one" / "p.npy")])
    proba1, count1 = np.load(tmp_path / "one" / "p.npy"), np.load(tmp_path / "one" / "p_count.npy")
    assert proba1.dtype == np.float16 and proba1.shape == (1500 // 16, 1300 // 16, 5)
    assert count1.dtype == np.int32 and count1.shape == proba1.shape[:2] and count1.min() >= 1
    stem = "synthetic_1500x1300"
    for f in (f"{stem}_mask.jpg", f"{stem}.jpg", f"{stem}_overlay.jpg", f"{stem}_confidence.jpg", f"{stem}_heat_TUM.jpg",
              f"{stem}_heat_BG.jpg"):
        assert (tmp_path / "one" / f).stat().st_size > 0, f
    # the library call with the CLI's model and sampler gives the saved arrays, and the CLI's map is the default one
    torch.manual_seed(0)
    model = get_model(5, "f32").to(dev).eval()
    smp = FullImageDenseSampler(tiles.synth_slide(1500, 1300, 0, dev), layer=2, patch_size=224, batch_size=16, stride=112, device=dev)
    cmap, pr = predict_full_patched(smp, model, 5, downscale=16, return_proba=True)
    assert np.array_equal(pred1.cpu().numpy(), cmap.cpu().numpy())
    assert np.array_equal(proba1, pr.proba.cpu().numpy().astype(np.float16)) and np.array_equal(count1, pr.count.cpu().numpy())
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}", DH_DIST_BACKEND="gloo", DH_SHARE_GPU="1")
    (tmp_path / "run2.py").write_text("import sys\nfrom examples.predict_full_patched import main\nmain(sys.argv[1:])\n")
    cmd = ["timeout", "-k", "10", "840", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(tmp_path / "run2.py"), *args,
           "--out_dir", str(tmp_path / "two"), "--save_proba", str(tmp_path / "two" / "p")]
    r = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "two" / "p.npy"), proba1)
    assert np.array_equal(np.load(tmp_path / "two" / "p_count.npy"), count1)
    assert (tmp_path / "two" / f"{stem}_confidence.jpg").stat().st_size > 0
    assert sorted(p.name for p in (tmp_path / "two").glob("*.npy")) == ["p.npy", "p_count.npy"]   # rank 0 only


def heat_np(img, field, col, alpha):
    return (img * alpha + (np.float64(field)[..., None] * col) * (1 - alpha)).astype(np.uint8)


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
def test_heatmap_blend_bit_identical(dev, alpha):
    from deephisto_amd import tiles
    h, w, n_cls = 123, 217, 5
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    logits = _logits(h * w, n_cls, 4, 3.0)
    proba = tiles.softmax_rows(torch.from_numpy(logits).to(dev)).view(h, w, n_cls)
    proba[:10] = 0.0                 # count == 0 cells
    proba[10:20, :, 2] = 1.0         # the edge values
    proba[10:20, :, 0] = 0.0
    host = proba.cpu().numpy()
    img_dev = torch.from_numpy(img).to(dev)
    for k, col in ((2, (33, 67, 156)), (0, (245, 119, 34)), (4, (255, 255, 255))):
        got = tiles.heatmap_blend(img_dev, proba[..., k], col, alpha)   # a strided view: read in place
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), heat_np(img, host[..., k], col, alpha)), (k, alpha)
    conf = proba.amax(dim=2)
    got = tiles.heatmap_blend(img_dev, conf, (255, 255, 255), alpha)
    assert np.array_equal(got.cpu().numpy(), heat_np(img, conf.cpu().numpy(), (255, 255, 255), alpha))
    got = tiles.heatmap_blend(img_dev, proba.permute(1, 0, 2).contiguous().permute(1, 0, 2)[..., 1], (64, 170, 72), alpha)
    assert np.array_equal(got.cpu().numpy(), heat_np(img, host[..., 1], (64, 170, 72), alpha))   # a view that needs a copy


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument(dev):
    from deephisto_amd import tiles
    from deephisto_amd._lib import DeephistoHipError
    h, w, P, d = 640, 800, 128, 16
    o = tiling.tile_origins(h, w, P, P)
    lg = torch.zeros((len(o), 5), device=dev)
    with pytest.raises(ValueError, match="n_cls = 65"):
        tiles.accumulate_probabilities(torch.zeros((len(o), 65), device=dev), o, P, d, h, w)
    with pytest.raises(DeephistoHipError, match="n_cls=65"):
        tiles.softmax_rows(torch.zeros((4, 65), device=dev))
    with pytest.raises(ValueError, match="7 origins"):
        tiles.accumulate_probabilities(lg, o[:7], P, d, h, w)
    good = tiles.accumulate_probabilities(lg, o, P, d, h, w, finish=False)

    def state(proba=None, count=None):
        return tiles.SlideProbabilities(good.proba if proba is None else proba, good.count if count is None else count)

    with pytest.raises(ValueError, match="state.proba must be contiguous"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=state(proba=torch.zeros((h // d, w // d, 10), device=dev)[..., ::2]))
    with pytest.raises(ValueError, match="state.proba must be float32"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=state(proba=good.proba.double()))
    with pytest.raises(ValueError, match="state.count must be int32"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=state(count=good.count.long()))
    with pytest.raises(ValueError, match=r"state.proba must be float32\[20, 25, 5\]"):
        tiles.accumulate_probabilities(lg, o, P, 32, h, w, state=good)      # another canvas
    with pytest.raises(ValueError, match=r"state.count must be int32\[40, 50\]"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=state(count=good.count[:, :49].contiguous()))
    with pytest.raises(ValueError, match="state.proba must live in GPU memory"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=state(proba=good.proba.cpu()))
    done = tiles.accumulate_probabilities(lg, o, P, d, h, w)
    with pytest.raises(ValueError, match="state is already finished"):
        tiles.accumulate_probabilities(lg, o, P, d, h, w, state=done)
    with pytest.raises(ValueError, match="already finished"):
        done.finish()
    img = torch.zeros((h // d, w // d, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="field must be a float32"):
        tiles.heatmap_blend(img, done.confidence[:, :10], (255, 255, 255))
    with pytest.raises(ValueError, match="color must be three integers"):
        tiles.heatmap_blend(img, done.confidence, (255, 300, 0))
    with pytest.raises(DeephistoHipError, match="alpha=2"):
        tiles.heatmap_blend(img, done.confidence, (255, 255, 255), 2.0)
    # the state is still usable after the refusals
    again = tiles.accumulate_probabilities(lg, o, P, d, h, w, state=good)
    assert torch.equal(again.count, 2 * done.count) and torch.equal(again.class_map, done.class_map)
