"""FullImageRndSampler's device index logic (csrc/coverage.hip + deephisto_amd/coverage.py) on the GPU.

The device path must reproduce the reference's sampler exactly: origins, filled ratios, the final hit-count map and
the global NumPy RNG stream (oracle/random_sampler.py, pinned to the reference by the committed fixtures), and the
batched random-branch prediction must give the callback path's class map and canvas bit for bit."""
import time

import numpy as np
import pytest
import torch

from oracle import random_sampler, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _sampler(slide, P, B, dl, d, **kw):
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    return FullImageRndSampler(slide, layer=1, patch_size=P, batch_size=B, dense_level=dl, speedup=d, **kw)


def _oracle_accum(h, w, P, d, origins):
    acc = np.zeros((h // d, w // d), np.float32)
    for o in origins:
        for y, x in o:
            acc[y // d:(y + P) // d, x // d:(x + P) // d] += 1
    return acc


GEOMETRIES = [   # h, w, patch, batch, dense_level, speedup, np seed
    (4096, 4096, 224, 64, 2, 16, 0),
    (3000, 5000, 96, 7, 3, 8, 1),
    (512, 640, 96, 4, 1, 16, 1),
    (12800, 12800, 224, 64, 2, 16, 5),
]


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}_{g[2]}_{g[3]}_dl{g[4]}_{g[5]}")
def test_device_path_matches_oracle_to_full_coverage(dev, geom):
    h, w, P, B, dl, d, seed = geom
    np.random.seed(seed)
    want = list(random_sampler.random_batches(h, w, P, B, dl, d))
    nxt = np.random.random_sample()
    slide = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    np.random.seed(seed)
    smp = _sampler(slide, P, B, dl, d, index_logic="device")
    assert smp.index_logic == "device"
    got = [(np.array([(p.pos_y, p.pos_x) for p in patches], np.int32), f) for patches, f in smp.generator()]
    assert np.random.random_sample() == nxt
    assert len(got) == len(want)
    for i, ((o_w, f_w), (o_g, f_g)) in enumerate(zip(want, got)):
        np.testing.assert_array_equal(o_g, o_w, err_msg=f"batch {i}")
        assert f_g == f_w, i
    assert smp._filled_ratio == [f for _, f in want]
    acc = smp._accum
    assert acc.dtype == np.float32 and acc.shape == (h // d, w // d)
    np.testing.assert_array_equal(acc, _oracle_accum(h, w, P, d, [o for o, _ in want]))
    if geom[0] == 512:
        assert smp.planner.stats.forced_batches > 0


def test_auto_selects_device_and_numpy_path_agrees(dev):
    h, w, P, B, dl, d = 1600, 2400, 128, 16, 2, 16
    slide = synth.synth_slide(h, w, 3)
    runs = {}
    for logic in ("auto", "numpy"):
        np.random.seed(42)
        smp = _sampler(slide, P, B, dl, d, index_logic=logic, device=dev)
        runs[logic] = ([(f.cpu(), c.cpu(), r) for f, c, r in smp.generator_torch()], np.random.random_sample(), smp)
    assert runs["auto"][2].index_logic == "device" and runs["numpy"][2].index_logic == "numpy"
    a, b = runs["auto"], runs["numpy"]
    assert a[1] == b[1] and len(a[0]) == len(b[0]) > 3
    for (fa, ca, ra), (fb, cb, rb) in zip(a[0], b[0]):
        assert torch.equal(fa, fb) and torch.equal(ca, cb) and ra == rb
    np.testing.assert_array_equal(a[2]._accum, b[2]._accum)
    assert a[2]._filled_ratio == b[2]._filled_ratio
    # a non-integer dense_level or a CPU device keeps the NumPy logic under "auto"
    assert _sampler(slide, P, B, 1.5, d, device=dev).index_logic == "numpy"
    assert _sampler(slide, P, B, 2, d, device="cpu").index_logic == "numpy"
    with pytest.raises(ValueError):
        _sampler(slide, P, B, 1.5, d, device=dev, index_logic="device")


def test_generator_device_yields_device_origins(dev):
    from deephisto_amd._lib import DH_LAYOUT_NCHW
    from oracle import tiling
    h, w, P, B = 900, 1100, 96, 8
    host = synth.synth_slide(h, w, 9)
    np.random.seed(8)
    want = list(random_sampler.random_batches(h, w, P, B, 2, 16))
    np.random.seed(8)
    smp = _sampler(torch.from_numpy(host).to(dev), P, B, 2, 16, index_logic="device")
    n = 0
    for (t, o, f), (o_w, f_w) in zip(smp.generator_device(DH_LAYOUT_NCHW, torch.float32), want):
        assert o.is_cuda and o.dtype == torch.int32 and tuple(o.shape) == (B, 2)
        np.testing.assert_array_equal(o.cpu().numpy(), o_w)
        assert f == f_w and tuple(t.shape) == (B, 3, P, P)
        np.testing.assert_array_equal(t.cpu().numpy(), tiling.gather_u8(host, o_w, P).astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255))
        n += 1
    assert n == len(want)


def test_reference_fixtures_through_the_device_path(dev, golden_meta, golden_vectors):
    from deephisto_amd.patch_samplers.full_samplers import SamplerExecutionMode
    for name, r in golden_meta["random_sampler"].items():
        host = synth.synth_slide(r["h"], r["w"], r["seed"])
        for gen in ("generator", "generator_torch"):
            np.random.seed(r["np_seed"])
            smp = _sampler(host, r["patch"], r["batch"], r["dense_level"], r["speedup"], device=dev,
                           mode=SamplerExecutionMode.INMEMORY_SINGLEPROC, index_logic="device")
            n = 0
            for i, item in enumerate(getattr(smp, gen)()):
                if gen == "generator":
                    got = np.array([(p.pos_y, p.pos_x) for p in item[0]], np.int32)
                else:
                    got = item[1].cpu().numpy().astype(np.int32)
                np.testing.assert_array_equal(got, golden_vectors[name + "_origins"][i])
                assert item[-1] == golden_vectors[name + "_ratios"][i]
                n += 1
            assert n == r["n_batches"]


def test_ondisk_device_path_equals_resident(dev, tmp_path):
    from deephisto_amd.patch_samplers.full_samplers import SamplerExecutionMode
    host = synth.synth_slide(800, 900, 12)
    path = tmp_path / "slide.npy"
    np.save(path, host)
    kw = dict(layer=1, patch_size=96, batch_size=8, dense_level=2, speedup=16, device=dev, index_logic="device")
    from deephisto_amd.patch_samplers.full_samplers import FullImageRndSampler
    np.random.seed(4)
    a = list(FullImageRndSampler(host, mode=SamplerExecutionMode.INMEMORY_SINGLEPROC, **kw).generator_torch())
    np.random.seed(4)
    b = list(FullImageRndSampler(path, mode=SamplerExecutionMode.ONDISK_MULTIPROC, **kw).generator_torch())
    assert len(a) == len(b) > 3
    for (fa, ca, ra), (fb, cb, rb) in zip(a, b):
        assert torch.equal(fa, fb) and torch.equal(ca, cb) and ra == rb


def test_device_path_refuses_a_map_smaller_than_the_batch(dev):
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="smaller than the batch"):
        _sampler(slide, 64, 64, 2, 16, index_logic="device")


# ---- kernels against NumPy on crafted maps ---------------------------------------------------------------------------

def _map(dev, h, w, P, d, dl, B):
    from deephisto_amd import tiles
    return tiles.CoverageMap(h, w, P, d, dl, B, device=dev)


def _step(cm, idx, explicit, jit):
    o = torch.full((len(idx), 2), -1, dtype=torch.int32, device=cm.device)
    cm.step(np.asarray(idx), explicit, np.asarray(jit), o.data_ptr(), host_origins=True)
    f, e, oh = cm.counters()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(o.cpu().numpy(), oh)
    return oh, f, e


def test_hit_update_duplicates_and_clamped_edges(dev):
    from deephisto_amd.coverage import NumpyCoverageMap
    h, w, P, d, dl = 1000, 1400, 96, 16, 3
    cm = _map(dev, h, w, P, d, dl, 16)
    ref = NumpyCoverageMap(h, w, P, d, dl)
    dh, dw = h // d, w // d
    corners = [0, dw - 1, (dh - 1) * dw, dh * dw - 1, 0, 0, dh * dw - 1, 5 * dw + 7, 5 * dw + 7, 3, (dh // 2) * dw]
    rs = np.random.RandomState(0)
    for rnd in range(4):
        jit = rs.randint(0, d, size=(len(corners), 2)).astype(np.int32)
        o, f, e = _step(cm, corners, True, jit)
        o_ref, f_ref, e_ref = ref.step(corners, True, jit)
        np.testing.assert_array_equal(o, o_ref)
        assert o[:, 0].min() == 0 and o[:, 0].max() == h - P and o[:, 1].min() == 0 and o[:, 1].max() == w - P
        assert (f, e) == (ref.filled, ref.eligible)
        np.testing.assert_array_equal(cm.read_map().cpu().numpy(), ref.accum.astype(np.float32))


def test_rank_to_cell_across_rows_and_chunks(dev):
    """Ranks among the eligible cells -> cells, on maps whose eligible cells straddle row and 1024-cell chunk
    boundaries, including the first and the last eligible cell."""
    h, w, P, d, dl = 70 * 16, 3000 * 16, 32, 16, 2           # 70 x 3000 cells: rows longer than a chunk
    cm = _map(dev, h, w, P, d, dl, 64)
    rs = np.random.RandomState(3)
    for density in (0.97, 0.4, 0.01):
        counts = np.where(rs.rand(70, 3000) < density, 0, rs.randint(dl, dl + 3, size=(70, 3000))).astype(np.int32)
        counts.ravel()[[1023, 1024, 2047, 3000, 2999]] = 0      # chunk and row edges eligible
        cm.set_map(counts)
        elig = np.flatnonzero(counts.ravel() < dl)
        assert cm.eligible == elig.size and cm.filled == np.count_nonzero(counts)
        picks = sorted(set([0, elig.size - 1] + list(np.searchsorted(elig, [1023, 1024, 2047, 2999, 3000]))
                           + rs.choice(elig.size, 40, replace=False).tolist()))[:64]
        jit = np.zeros((len(picks), 2), np.int32)
        o, _, _ = _step(cm, picks, False, jit)
        cells = elig[picks]
        pd2 = P // d // 2
        want_y = np.clip((cells // 3000 - pd2) * d, 0, h - P)
        want_x = np.clip((cells % 3000 - pd2) * d, 0, w - P)
        np.testing.assert_array_equal(o, np.stack([want_y, want_x], 1))


def test_eligible_cells_compaction(dev):
    h, w, P, d, dl = 50 * 8, 3000 * 8, 16, 8, 2
    cm = _map(dev, h, w, P, d, dl, 64)
    counts = np.full((50, 3000), dl, np.int32)
    rs = np.random.RandomState(9)
    pick = np.sort(np.concatenate([[0, 1023, 1024, 50 * 3000 - 1], rs.choice(50 * 3000, 40, replace=False)]))
    pick = np.unique(pick)
    counts.ravel()[pick] = rs.randint(0, dl, size=pick.size)
    cm.set_map(counts)
    assert cm.eligible == pick.size
    np.testing.assert_array_equal(cm.eligible_cells(), pick)


def test_step_argument_errors_before_any_gpu_call(dev):
    from deephisto_amd import _lib
    cm = _map(dev, 512, 512, 64, 16, 2, 8)
    with pytest.raises(_lib.DeephistoHipError, match="rank"):
        cm.step(np.array([1024] * 8), False, np.zeros((8, 2), np.int32))
    with pytest.raises(_lib.DeephistoHipError, match="jitter"):
        cm.step(np.arange(8), False, np.full((8, 2), 16, np.int32))
    with pytest.raises(_lib.DeephistoHipError, match="outside"):
        cm.step(np.arange(9), False, np.zeros((9, 2), np.int32))
    import ctypes as C
    h = C.c_void_p()
    assert _lib.lib().dh_coverage_create(C.byref(h), 100, 100, 64, 16, 0, 4, None) == -22
    assert b"dense_level" in _lib.lib().dh_last_error()


# ---- batched random-branch prediction ----------------------------------------------------------------------------------

def _callback_path(sampler, model, n_cls, d, dev):
    """The reference's loop: batch_predictor per sampler batch, then the ordered accumulation."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import batch_predictor
    origins, logits = [], []
    for patches, _ in sampler.generator():
        logits.append(torch.from_numpy(batch_predictor(patches, model, dev)))
        origins.append(np.array([(p.pos_y, p.pos_x) for p in patches], np.int32))
    return tiles.accumulate_logits(torch.cat(logits).to(dev).contiguous(), np.concatenate(origins), sampler.patch_size,
                                   d, sampler.h, sampler.w)


@pytest.mark.parametrize("dtype,dl,mb", [("bf16", 2, None), ("f32", 2, None), ("bf16", 1, 256), ("f32", 1, 128)])
def test_predict_random_patched_equals_callback_path(dev, dtype, dl, mb):
    from deephisto_amd.examples.predict_full_patched import ImagePredictorPatched, batch_predictor, predict_random_patched
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from deephisto_amd import tiles
    h = w = 2048
    P, B, d = 224, 64, 16
    slide = tiles.synth_slide(h, w, 4, dev)
    torch.manual_seed(1)
    model = get_model(5, dtype).to(dev).eval()
    np.random.seed(17)
    cmap, canvas = predict_random_patched(_sampler(slide, P, B, dl, d, index_logic="device"), model, 5, d, micro_batch=mb,
                                          return_canvas=True)
    np.random.seed(17)
    canvas_cb, cmap_cb = _callback_path(_sampler(slide, P, B, dl, d, index_logic="device"), model, 5, d, dev)
    assert torch.equal(canvas, canvas_cb) and torch.equal(cmap, cmap_cb)
    np.random.seed(17)
    smp = _sampler(slide, P, B, dl, d, index_logic="numpy")
    pred = ImagePredictorPatched((h, w), smp.generator(), lambda p: batch_predictor(p, model, dev), 5, layer=1, downscale=d).process()
    np.testing.assert_array_equal(cmap.cpu().numpy(), pred)


def test_main_random_sampler_uses_batched_path(dev, tmp_path, monkeypatch):
    from deephisto_amd.examples import predict_full_patched as pfp
    from deephisto_amd.models.patch_cls_simple.model import get_model
    calls = []
    real = pfp.predict_random_patched
    monkeypatch.setattr(pfp, "predict_random_patched", lambda *a, **k: calls.append(1) or real(*a, **k))
    args = ["--random_sampler", "--synthetic", "1200", "1500", "--weights", "", "--patch_size", "224", "--batch_size", "16",
            "--compute_dtype", "bf16", "--no_visualizations", "--out_dir", str(tmp_path)]
    np.random.seed(23)
    pred = pfp.main(args)
    assert calls == [1]
    from deephisto_amd import tiles
    torch.manual_seed(0)
    model = get_model(n_classes=5, compute_dtype="bf16").to(dev).eval()
    np.random.seed(23)
    smp = _sampler(tiles.synth_slide(1200, 1500, 0, dev), 224, 16, 2, 16)
    want = pfp.ImagePredictorPatched((1200, 1500), smp.generator(), lambda p: pfp.batch_predictor(p, model, dev), 5, layer=2,
                                     downscale=16).process()
    np.testing.assert_array_equal(np.asarray(pred), want)


def test_full_size_slide_reaches_coverage_quickly(dev):
    """The reference's geometry: 50 000^2 slide, patch 224, batch 64, dense_level 2, speedup 16 (3 125^2 cells).  The
    device path reaches full coverage well inside the step limit; its first 10 batches equal the oracle's."""
    h = w = 50000
    P, B, dl, d = 224, 64, 2, 16
    np.random.seed(31)
    want = []
    for i, item in enumerate(random_sampler.random_batches(h, w, P, B, dl, d)):
        want.append(item)
        if i == 9:
            break
    slide = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)   # 7.5 GB in HBM; only the geometry matters here
    np.random.seed(31)
    smp = _sampler(slide, P, B, dl, d)
    assert smp.index_logic == "device"
    t0 = time.time()
    n, filled = 0, 0.0
    for _, o_host, filled in smp._device_origin_batches(host_origins=True):
        if n < 10:
            np.testing.assert_array_equal(o_host, want[n][0])
            assert filled == want[n][1]
        n += 1
    dt = time.time() - t0
    assert filled == 1.0 and smp._filled_ratio[-1] == 1.0
    assert dt < 60, f"{n} batches took {dt:.1f} s"
    print(f"50000^2: {n} batches, {n * B} tiles, {dt:.2f} s, {n * B / dt:.0f} patches/s (sampler only)")
