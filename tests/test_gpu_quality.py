"""GPU: the tile quality filter of whole-slide prediction against the NumPy restatement in
tests/helpers/quality_ref.py.

The per-tile sums (n_t, S1, S2, n_ink) equal the restatement bit for bit at every size, origin and threshold; the flags equal
the Python-int rule; a filter that keeps every tile changes no bit; on a painted slide the filtered class map equals the
UNFILTERED run's logits accumulated over the kept rows in grid order (float32 +=), argmax, uncovered cells filled."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import synth

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import quality_ref as Q  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
CONFIGS = [("resnet18", "f32"), ("resnet18", "bf16"), ("resnet50", "bf16")]
THRESHOLDS = (-1, 0, 37, 255)
MIN_SHARPNESS, MAX_INK = 200, 0.1        # between a blurred tile's ~12 and a sharp tile's ~2 600; pink noise has no ink pixel


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _filter(**kw):
    from deephisto_amd.quality import QualityFilter
    return QualityFilter(**kw)


def _origins(h, w, P, seed, n_random=6):
    """The four corners plus seeded random origins, at least one with odd x (when the slide leaves room for one)."""
    rng = np.random.default_rng(seed)
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(n_random)]
    if w - P >= 1:
        o.append((int(rng.integers(0, h - P + 1)), 2 * int(rng.integers(0, (w - P + 1) // 2)) + 1))
        assert o[-1][1] % 2 == 1 and o[-1][1] <= w - P
    return np.array(o, np.int32)


def _stats(host_or_dev, o, P, t, dev, filt=None, host_check=True):
    from deephisto_amd import quality
    slide = host_or_dev if isinstance(host_or_dev, torch.Tensor) else torch.from_numpy(host_or_dev).to(dev)
    got = quality.tile_quality_stats(slide, torch.from_numpy(o).to(dev), P, t, filt or _filter(), o if host_check else None)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(o), 4)
    return got.cpu().numpy()


# ---- kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "painted"])
@pytest.mark.parametrize("h,w,P", [(8, 8, 8), (17, 33, 8), (17, 33, 17), (67, 93, 16), (67, 93, 31), (67, 93, 64),
                                   (300, 333, 224), (300, 333, 256)])
def test_stats_equal_restatement(dev, h, w, P, kind):
    host = synth.synth_slide(h, w, h * w + P) if kind == "noise" else Q.painted(h, w, h + P)[0]
    o = _origins(h, w, P, P)
    for t in THRESHOLDS:
        np.testing.assert_array_equal(_stats(host, o, P, t, dev), Q.tile_stats(host, o, P, t), err_msg=f"t={t}")
    # the ink rule's constants reach the kernel; origins that live on the device only give the same sums
    ink = dict(ink_chroma=5, ink_margin=0, dark_max=-1)
    np.testing.assert_array_equal(_stats(host, o, P, 37, dev, _filter(**ink), host_check=False), Q.tile_stats(host, o, P, 37, **ink))


def test_unaligned_slide_view(dev):
    h, w, P = 40, 61, 16
    host = synth.synth_slide(h, w, 3)
    flat = torch.from_numpy(host.reshape(-1)).to(dev)
    buf = torch.empty(flat.numel() + 5, dtype=torch.uint8, device=dev)
    buf[5:] = flat
    view = buf[5:].view(h, w, 3)   # contiguous, 5 bytes past a 16-byte boundary
    assert view.data_ptr() % 16 == 5
    o = _origins(h, w, P, 1)
    for t in (-1, 37):
        np.testing.assert_array_equal(_stats(view, o, P, t, dev), Q.tile_stats(host, o, P, t))


def test_extremes_checkerboard_at_the_largest_patch(dev):
    """0 / 255 checkerboard, 1030 x 1027 at P = 1024: every interior L is +-1020, so S2 is as large as a tile's can be."""
    from deephisto_amd import quality
    from deephisto_amd._lib import DeephistoHipError
    h, w, P = 1030, 1027, 1024
    yy, xx = np.mgrid[:h, :w]
    host = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    o = np.array([[0, 0], [6, 3], [3, 2], [1, 1]], np.int32)
    got = _stats(host, o, P, -1, dev)
    np.testing.assert_array_equal(got, Q.tile_stats(host, o, P, -1))
    n_t, s1, s2, _ = (int(v) for v in got[3])            # the tile at (1, 1) touches no border of the slide
    assert n_t == P * P and s2 == P * P * 1020 * 1020 and s1 == 0
    stats_dev = torch.from_numpy(got).to(dev)
    for ms in (0, 1, 1040399, 1040400):
        reason, keep = quality.quality_flags(stats_dev, _filter(min_sharpness=ms), P)
        want_r, want_k = Q.flags(got, ms, P * P)
        np.testing.assert_array_equal(reason.cpu().numpy(), want_r)
        np.testing.assert_array_equal(keep.cpu().numpy(), want_k)
    assert keep.cpu().numpy()[3] == 1                    # variance exactly 1 040 400 is not below it
    slide = torch.from_numpy(host).to(dev)
    with pytest.raises(DeephistoHipError, match="patch 1025 above 1024"):
        quality.tile_quality_stats(slide, torch.from_numpy(o[:1]).to(dev), 1025, -1, _filter())
    with pytest.raises(ValueError, match="patch size"):
        quality.score_quality(slide, torch.from_numpy(o[:1]).to(dev), 1025, -1, _filter())


def test_offsets_past_2_31(dev):
    """26 001 x 28 003 x 3 = 2.18e9 bytes (> 2^31): tiles at the far end and the bottom-right corner against the restatement
    applied to the downloaded window plus halo."""
    from deephisto_amd import tiles
    h, w, P = 26001, 28003, 224
    assert h * w * 3 > 2 ** 31
    slide = tiles.synth_slide(h, w, 5, dev)
    o = np.array([[h - P, w - P], [h - P, 0], [h - P - 1, w - P - 1], [25700, 27001], [25600, 13], [0, w - P], [0, 0]], np.int32)
    assert (o[:5, 0].astype(np.int64) * w * 3 > 2 ** 31).all()
    for t in (-1, 37):
        got = _stats(slide, o, P, t, dev)
        for (y, x), row in zip(o.tolist(), got):
            top, bottom, left, right = y > 0, y + P < h, x > 0, x + P < w
            win = slide[y - top:y + P + bottom, x - left:x + P + right].cpu().numpy()
            np.testing.assert_array_equal(row, Q.window_stats(win, P, t, top, bottom, left, right), err_msg=f"({y}, {x}) t={t}")
    del slide
    torch.cuda.empty_cache()


def test_flags_equal_python_int_rule(dev):
    """dh_quality_flags on a hand-made stats tensor (no slide involved): random rows within a P <= 1024 tile's bounds plus the
    boundary rows of the host test."""
    from deephisto_amd import quality
    rng = np.random.default_rng(0)
    P, m = 1024, 1020 * 1020
    n_t = rng.integers(0, P * P + 1, 3000)
    rows = np.stack([n_t, (rng.uniform(-1, 1, 3000) * 1020 * n_t).astype(np.int64), (rng.uniform(0, 1, 3000) * m * n_t).astype(np.int64),
                     rng.integers(0, P * P + 1, 3000)], 1).astype(np.int64)
    small = rng.integers(0, 50, (500, 4)).astype(np.int64)          # small sums: equalities and near-equalities happen here
    small[:, 2] = small[:, 2] * small[:, 0]
    cases = Q.boundary_cases()
    for ms, frac in ((0, 1.0), (1, 0.0), (5, 1.0 / P / P), (200, 0.1), (m - 1, 1.0 - 1.0 / P / P), (m, 0.5)):
        filt = _filter(min_sharpness=ms, max_ink_fraction=frac)
        mi = Q.max_ink_pixels(frac, P)
        assert mi == filt.max_ink_pixels(P)
        bound = np.array([c[:4] for c in cases if c[4] == ms], np.int64)
        stats = np.concatenate([rows, small, bound])
        reason, keep = quality.quality_flags(torch.from_numpy(stats).to(dev), filt, P)
        assert reason.dtype == torch.uint8 and keep.dtype == torch.int32
        want_r, want_k = Q.flags(stats, ms, mi)
        np.testing.assert_array_equal(reason.cpu().numpy(), want_r)
        np.testing.assert_array_equal(keep.cpu().numpy(), want_k)
    assert len(bound) and set(want_r.tolist()) == {0, Q.BLUR, Q.INK, Q.BLUR | Q.INK}


def test_score_quality_compacts_in_grid_order(dev):
    from deephisto_amd import quality, tiles
    h, w, P, S = 300, 333, 64, 48
    host, _ = Q.painted(h, w, 2)
    o_all, n_unique = tiles.tile_grid(h, w, P, S, 7)
    o = np.ascontiguousarray(o_all[:n_unique])
    filt = _filter(min_sharpness=MIN_SHARPNESS, max_ink_fraction=MAX_INK)
    idx, yx, info = quality.score_quality(torch.from_numpy(host).to(dev), torch.from_numpy(o).to(dev), P, -1, filt, o)
    stats = Q.tile_stats(host, o, P, -1)
    want_r, want_k = Q.flags(stats, MIN_SHARPNESS, Q.max_ink_pixels(MAX_INK, P))
    keep = np.flatnonzero(want_k)
    assert 0 < len(keep) < n_unique
    np.testing.assert_array_equal(idx.cpu().numpy(), keep)
    np.testing.assert_array_equal(yx.cpu().numpy(), o[keep])
    np.testing.assert_array_equal(info["stats"], stats)
    np.testing.assert_array_equal(info["reason"], want_r)
    assert (info["threshold"], info["min_sharpness"], info["max_ink_pixels"]) == (-1, MIN_SHARPNESS, 409)
    assert (info["n_tiles"], info["n_kept"]) == (n_unique, len(keep))
    assert info["rejected_blur"] == int((want_r & Q.BLUR != 0).sum()) and info["rejected_ink"] == int((want_r & Q.INK != 0).sum())
    sharp = quality.sharpness(info["stats"])
    want = np.array([(n * s2 - s1 * s1) / (n * n) if n else np.nan for n, s1, s2, _ in stats.tolist()])
    np.testing.assert_array_equal(sharp, want)


# ---- prediction ---------------------------------------------------------------------------------------------------------------
def _model(arch, dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(0)
    return get_model(5, dtype, arch=arch).to(dev).eval()


def _sampler(host, P, S, B, dev):
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    return FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev)


H, W, D = 700, 900, 16


@pytest.fixture(scope="module")
def painted_slide():
    return Q.painted(H, W, 7)


@pytest.mark.parametrize("arch,dtype", CONFIGS)
@pytest.mark.parametrize("P,S", [(224, 112), (256, 256)])
def test_painted_slide_matches_oracle(dev, painted_slide, arch, dtype, P, S):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    host, areas = painted_slide
    model = _model(arch, dtype, dev)
    smp = _sampler(host, P, S, 7, dev)
    n_unique, origins = smp.n_tiles, smp.origins
    assert len(origins) > n_unique                        # the corner's padding duplicates are in play
    grid = origins[:n_unique]
    cmap0, logits0_dev = predict_full_patched(smp, model, 5, downscale=D, return_logits=True)
    logits0 = logits0_dev.cpu().numpy()

    # the default filter keeps every tile and changes no bit
    info: dict = {}
    cmap1, logits1 = predict_full_patched(smp, model, 5, downscale=D, return_logits=True, quality=_filter(), quality_info=info)
    assert info["n_kept"] == info["n_tiles"] == n_unique and info["rejected_blur"] == info["rejected_ink"] == 0
    np.testing.assert_array_equal(info["kept"], np.arange(n_unique))
    assert torch.equal(cmap1, cmap0) and torch.equal(logits1, logits0_dev)

    stats = Q.tile_stats(host, grid, P, -1)
    np.testing.assert_array_equal(info["stats"], stats)
    where = {k: Q.inside(grid, P, a, H, W) for k, a in areas.items()}
    assert all(m.any() for m in where.values())
    for filt, mb in ((_filter(min_sharpness=MIN_SHARPNESS, max_ink_fraction=MAX_INK), None),
                     (_filter(max_ink_fraction=MAX_INK, fill_class=3), 32),
                     (_filter(min_sharpness=MIN_SHARPNESS), None)):
        want_r, want_k = Q.flags(stats, filt.min_sharpness, Q.max_ink_pixels(filt.max_ink_fraction, P))
        keep = np.flatnonzero(want_k)
        assert 0 < len(keep) < n_unique
        info = {}
        cmap, logits = predict_full_patched(smp, model, 5, downscale=D, micro_batch=mb, return_logits=True, quality=filt,
                                            quality_info=info)
        assert info["kept"].dtype == np.int64
        np.testing.assert_array_equal(info["kept"], keep)
        np.testing.assert_array_equal(info["reason"], want_r)
        np.testing.assert_array_equal(info["stats"], stats)
        assert info["threshold"] == -1 and info["n_kept"] == len(keep) and info["n_tiles"] == n_unique
        np.testing.assert_array_equal(cmap.cpu().numpy(), Q.filtered_map(logits0, origins, n_unique, keep, P, D, H, W, filt.fill_class))
        lg = logits.cpu().numpy()
        assert lg.shape == logits0.shape
        rejected = np.setdiff1d(np.arange(n_unique), keep)
        np.testing.assert_array_equal(lg[keep], logits0[keep])
        assert np.isnan(lg[rejected]).all()
        # what the painted areas must come out as: a flat tile has variance 0, so with a sharpness test it is blurred as well
        r = info["reason"]
        blur_bit = Q.BLUR if filt.min_sharpness else 0
        ink_bit = Q.INK if filt.max_ink_fraction < 1 else 0
        assert (r[where["sharp"]] == 0).all() and (r[where["blur"]] == blur_bit).all()
        assert (r[where["blue"]] == (blur_bit | ink_bit)).all() and (r[where["black"]] == (blur_bit | ink_bit)).all()
    # with the ink test alone the blue and the black tiles carry reason 4, with the sharpness test alone the blurred ones carry 2
    assert ink_bit == 0 and (r[where["blur"]] == 2).all()
    cmap = predict_full_patched(smp, model, 5, downscale=D, dedupe_padding=True,
                                quality=_filter(min_sharpness=MIN_SHARPNESS, max_ink_fraction=MAX_INK))
    keep = np.flatnonzero(Q.flags(stats, MIN_SHARPNESS, Q.max_ink_pixels(MAX_INK, P))[1])
    np.testing.assert_array_equal(cmap.cpu().numpy(), Q.filtered_map(logits0, origins, n_unique, keep, P, D, H, W, -1, dedupe=True))

    # both filters: the tissue stage first (the black quarter is glass at chroma <= 20), the quality stage over its survivors
    # with the tissue filter's threshold; tissue_info is what it is without the quality filter
    tf = TissueFilter(20, 0.5, fill_class=2)
    qf = _filter(min_sharpness=MIN_SHARPNESS, max_ink_fraction=MAX_INK, fill_class=2)
    t_alone: dict = {}
    predict_full_patched(smp, model, 5, downscale=D, tissue=tf, tissue_info=t_alone)
    t_info, q_info = {}, {}
    cmap, logits = predict_full_patched(smp, model, 5, downscale=D, return_logits=True, tissue=tf, tissue_info=t_info,
                                        quality=qf, quality_info=q_info)
    counts = np.array([int(Q.tissue_mask(host[y:y + P, x:x + P], 20).sum()) for y, x in grid.tolist()])
    first = np.flatnonzero(counts >= tf.min_pixels(P))
    assert 0 < len(first) < n_unique
    assert sorted(t_info) == sorted(t_alone)
    for k in t_alone:
        np.testing.assert_array_equal(t_info[k], t_alone[k])
    np.testing.assert_array_equal(t_info["kept"], first)
    stats20 = Q.tile_stats(host, grid[first], P, 20)
    final = first[np.flatnonzero(Q.flags(stats20, MIN_SHARPNESS, Q.max_ink_pixels(MAX_INK, P))[1])]
    assert 0 < len(final) < len(first)
    np.testing.assert_array_equal(q_info["stats"], stats20)
    np.testing.assert_array_equal(q_info["kept"], final)
    assert q_info["threshold"] == 20 and q_info["n_tiles"] == len(first) and q_info["n_kept"] == len(final)
    np.testing.assert_array_equal(cmap.cpu().numpy(), Q.filtered_map(logits0, origins, n_unique, final, P, D, H, W, 2))
    lg = logits.cpu().numpy()
    np.testing.assert_array_equal(lg[final], logits0[final])
    assert np.isnan(lg[np.setdiff1d(np.arange(n_unique), final)]).all()


def test_slide_blurred_everywhere_runs_no_forward(dev, painted_slide):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    host = Q.box_blur(painted_slide[0][:350, :450], 5)    # the sharp quarter, blurred
    model = _model("resnet18", "bf16", dev)
    calls = []
    fwd, name = model.tiles_entry()
    model.tiles_entry = lambda: ((lambda *a: calls.append(1) or fwd(*a)), name)
    smp = _sampler(host, 224, 112, 8, dev)
    info: dict = {}
    filt = _filter(min_sharpness=MIN_SHARPNESS, fill_class=2)
    cmap, logits = predict_full_patched(smp, model, 5, downscale=D, return_logits=True, quality=filt, quality_info=info)
    assert info["n_kept"] == 0 and len(info["kept"]) == 0 and info["rejected_blur"] == info["n_tiles"] == smp.n_tiles
    assert cmap.shape == (350 // D, 450 // D) and (cmap == 2).all()
    assert torch.isnan(logits).all()
    assert calls == []
    predict_full_patched(smp, model, 5, downscale=D)
    assert calls   # the wrapper does count launches


def test_refusals(dev, tmp_path):
    from deephisto_amd import quality
    from deephisto_amd._lib import DeephistoHipError
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import (FullImageDenseSampler, FullImageRndSampler,
                                                            SamplerExecutionMode)
    from deephisto_amd.tissue import TissueFilter, select_tiles
    host = synth.synth_slide(500, 600, 1)
    path = tmp_path / "slide.npy"
    np.save(path, host)
    model = _model("resnet18", "f32", dev)
    disk = FullImageDenseSampler(path, layer=1, patch_size=128, batch_size=8, stride=128, device=dev,
                                 mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    with pytest.raises(ValueError, match="quality filter needs an HBM-resident"):
        predict_full_patched(disk, model, 5, quality=_filter())
    rnd = FullImageRndSampler(host, layer=1, patch_size=128, batch_size=8, device=dev, index_logic="device")
    with pytest.raises(ValueError, match="random sampler"):
        predict_full_patched(rnd, model, 5, quality=_filter())
    smp = _sampler(host, 128, 128, 8, dev)
    with pytest.raises(ValueError, match="fill_class"):
        predict_full_patched(smp, model, 5, tissue=TissueFilter(fill_class=1), quality=_filter(fill_class=2))
    slide = torch.from_numpy(host).to(dev)
    o = np.array([[0, 0], [400, 480]], np.int32)   # 480 + 128 > 600
    o_dev = torch.from_numpy(o).to(dev)
    with pytest.raises(DeephistoHipError, match=r"origin 1 \(400, 480\) outside"):
        quality.tile_quality_stats(slide, o_dev, 128, 10, _filter(), o)
    stats = quality.tile_quality_stats(slide, o_dev, 128, 10, _filter())   # device-only origins: flagged, not read
    assert stats.cpu().numpy()[1].tolist() == [-1, -1, -1, -1]
    reason, keep = quality.quality_flags(stats, _filter(), 128)
    assert keep.cpu().numpy().tolist() == [1, -1] and reason.cpu().numpy()[1] == 255
    with pytest.raises(DeephistoHipError, match="1 origins lie outside"):
        select_tiles(keep, o_dev, 1)
    with pytest.raises(DeephistoHipError, match="threshold 300"):
        quality.tile_quality_stats(slide, o_dev[:1], 128, 300, _filter())
    with pytest.raises(DeephistoHipError, match="larger than"):
        quality.tile_quality_stats(slide, o_dev[:1], 512, 10, _filter())
    with pytest.raises(ValueError, match="uint8"):
        quality.tile_quality_stats(slide.float(), o_dev[:1], 128, 10, _filter())
    with pytest.raises(ValueError, match="GPU memory"):
        quality.tile_quality_stats(torch.from_numpy(host), o_dev[:1], 128, 10, _filter())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_quality_two_ranks_equal_single_process(built_lib, tmp_path):
    """`--min_sharpness / --max_ink` through the CLI: two ranks sharing cuda:0 over gloo score the same kept list and give the
    single-process map; --quality_json holds the restatement's counts."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import main
    h, w, P, S = 900, 1000, 224, 112
    # the closed-form slide is uniform noise: sharpness about 16 050 and an ink share about 0.423 in every tile, so these two
    # thresholds each cut through the middle of the list
    args = ["--synthetic", str(h), str(w), "--weights", "", "--patch_size", str(P), "--stride", str(S), "--batch_size", "16",
            "--min_sharpness", "16050", "--max_ink", "0.4235", "--quality_fill", "BG", "--no_visualizations"]
    pred1 = main(args + ["--out_dir", str(tmp_path / "one"), "--quality_json", str(tmp_path / "q1.json")]).cpu().numpy()
    assert pred1.shape == (h // 16, w // 16)
    host = tiles.synth_slide(h, w, 0, "cuda:0").cpu().numpy()
    o_all, n_unique = tiles.tile_grid(h, w, P, S, 16)
    stats = Q.tile_stats(host, o_all[:n_unique], P, -1)
    want_r, want_k = Q.flags(stats, 16050, Q.max_ink_pixels(0.4235, P))
    assert 0 < want_k.sum() < n_unique and (want_r & Q.BLUR).any() and (want_r & Q.INK).any()
    doc = json.loads((tmp_path / "q1.json").read_text())
    assert (doc["n_tiles"], doc["n_kept"]) == (n_unique, int(want_k.sum()))
    assert (doc["rejected_blur"], doc["rejected_ink"]) == (int((want_r & Q.BLUR != 0).sum()), int((want_r & Q.INK != 0).sum()))
    assert (doc["min_sharpness"], doc["max_ink_fraction"], doc["max_ink_pixels"]) == (16050, 0.4235, Q.max_ink_pixels(0.4235, P))
    assert (doc["ink_chroma"], doc["ink_margin"], doc["dark_max"], doc["fill_class"], doc["threshold"]) == (40, 16, 40, 1, -1)
    sharp = np.array([(n * s2 - s1 * s1) / (n * n) for n, s1, s2, _ in stats.tolist()])
    five = doc["sharpness"]
    assert five["n"] == n_unique
    np.testing.assert_allclose([five["min"], five["q1"], five["median"], five["q3"], five["max"]],
                               np.percentile(sharp, [0, 25, 50, 75, 100]), rtol=1e-12)
    (tmp_path / "run2.py").write_text(
        "import os, sys, numpy as np\n"
        "from examples.predict_full_patched import main\n"
        "pred = main(sys.argv[1:])\n"
        "np.save(f'pred_{os.environ.get(\"RANK\", \"0\")}.npy', pred.cpu().numpy())\n")
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}", DH_DIST_BACKEND="gloo", DH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(tmp_path / "run2.py"), *args, "--out_dir", str(tmp_path / "two"),
           "--quality_json", str(tmp_path / "q2.json")]
    r = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("quality: ") == 1 and f"quality: {int(want_k.sum())} of {n_unique} tiles pass" in r.stdout, r.stdout[-2000:]
    assert json.loads((tmp_path / "q2.json").read_text()) == doc
    for k in range(2):
        assert np.array_equal(np.load(tmp_path / f"pred_{k}.npy"), pred1), f"rank {k}"
