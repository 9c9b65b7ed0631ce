"""GPU: the tissue filter of whole-slide prediction against a NumPy oracle in this file.

The histogram equals np.bincount of the chroma; per-tile counts equal a summed-area table of the tissue mask; the kept list is
np.flatnonzero order; a filter that keeps every tile changes no bit; on a painted slide the masked class map equals the
UNMASKED run's logits accumulated over the kept rows in grid order (float32 +=), argmax, uncovered cells filled."""
import math
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
GREY = (200, 196, 198)   # chroma 4: glass for t >= 4, tissue for t <= 3
CONFIGS = [("resnet18", "f32"), ("resnet18", "bf16"), ("resnet50", "bf16")]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- oracle ---------------------------------------------------------------------------------------------------------------
def chroma_np(host):
    return (host.max(axis=2).astype(np.int16) - host.min(axis=2)).astype(np.uint8)


def counts_np(host, origins, P, t):
    m = (chroma_np(host) > t).astype(np.int64)
    s = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int64)
    s[1:, 1:] = m.cumsum(0).cumsum(1)
    y, x = origins[:, 0].astype(np.int64), origins[:, 1].astype(np.int64)
    return s[y + P, x + P] - s[y, x + P] - s[y + P, x] + s[y, x]


def otsu_np(host):
    from deephisto_amd.tissue import otsu_threshold
    return otsu_threshold(np.bincount(chroma_np(host).ravel(), minlength=256))


def masked_map_np(logits_unmasked, origins, n_unique, kept, P, d, h, w, fill, dedupe=False):
    """Unmasked logits, kept rows only, grid order (the corner's padding duplicates follow the corner), float32 +=, argmax, fill."""
    n_cls = logits_unmasked.shape[1]
    rows = list(kept)
    if not dedupe and len(kept) and kept[-1] == n_unique - 1:
        rows += list(range(n_unique, len(origins)))
    canvas = np.zeros((h // d, w // d, n_cls), np.float32)
    cover = np.zeros((h // d, w // d), bool)
    for i in rows:
        y, x = int(origins[i, 0]), int(origins[i, 1])
        canvas[y // d:(y + P) // d, x // d:(x + P) // d] += logits_unmasked[i]
        cover[y // d:(y + P) // d, x // d:(x + P) // d] = True
    out = np.argmax(canvas, axis=2).astype(np.int64)
    out[~cover] = fill
    return out


def painted(h, w, seed):
    """Synthetic tissue with a seeded glass pattern: white (255) columns and blocks over about half the area, a grey band."""
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


def _sampler(host, P, S, B, dev):
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    return FullImageDenseSampler(host, layer=1, patch_size=P, batch_size=B, stride=S, device=dev)


# ---- kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (1, 21), (17, 33), (257, 1001), (999, 1237)])
def test_histogram_equals_bincount(dev, h, w):
    from deephisto_amd import tissue
    host = painted(h, w, h + w) if min(h, w) > 300 else synth.synth_slide(h, w, h * w)
    hist = tissue.chroma_histogram(torch.from_numpy(host).to(dev))
    assert hist.dtype == np.uint64 and hist.shape == (256,)
    np.testing.assert_array_equal(hist, np.bincount(chroma_np(host).ravel(), minlength=256))


def test_unaligned_slide_view_is_handled(dev):
    from deephisto_amd import tissue
    host = synth.synth_slide(40, 61, 3)
    flat = torch.from_numpy(host.reshape(-1)).to(dev)
    buf = torch.empty(flat.numel() + 5, dtype=torch.uint8, device=dev)
    buf[5:] = flat
    view = buf[5:].view(40, 61, 3)   # contiguous, 5 bytes past a 16-byte boundary
    np.testing.assert_array_equal(tissue.chroma_histogram(view), np.bincount(chroma_np(host).ravel(), minlength=256))


def test_slide_past_2_31_bytes(dev):
    """26 001 x 28 003 x 3 = 2.18e9 bytes (> 2^31), h*w % 16 = 3: histogram and tile counts with 64-bit offsets."""
    from deephisto_amd import tiles, tissue
    h, w, P = 26001, 28003, 224
    assert h * w * 3 > 2 ** 31 and (h * w) % 16 == 3
    slide = tiles.synth_slide(h, w, 5, dev)
    slide[:, :9000] = 255
    slide[20000:21000] = torch.tensor(GREY, dtype=torch.uint8, device=dev)
    c = (slide.amax(2) - slide.amin(2)).cpu().numpy()
    np.testing.assert_array_equal(tissue.chroma_histogram(slide), np.bincount(c.ravel(), minlength=256))
    rng = np.random.default_rng(0)
    o = np.stack([rng.integers(0, h - P + 1, 300), rng.integers(0, w - P + 1, 300)], 1).astype(np.int32)
    o = np.concatenate([o, [[h - P, w - P], [h - P, 0], [0, w - P], [19900, 8900], [25000, 27000]]]).astype(np.int32)
    for t in (3, 4, 60):
        got = tissue.tile_tissue_counts(slide, torch.from_numpy(o).to(dev), P, t, o).cpu().numpy()
        m = (c > t)
        want = np.array([int(m[y:y + P, x:x + P].sum()) for y, x in o])
        np.testing.assert_array_equal(got, want)
    del slide
    torch.cuda.empty_cache()


@pytest.mark.parametrize("P,S", [(256, 256), (224, 112), (64, 48)])
def test_counts_and_selection_on_dense_grids(dev, P, S):
    from deephisto_amd import tiles, tissue
    h, w = 1000, 1337
    host = painted(h, w, P + S)
    slide = torch.from_numpy(host).to(dev)
    o_all, n_unique = tiles.tile_grid(h, w, P, S, 7)
    o = np.ascontiguousarray(o_all[:n_unique])
    assert (o[:, 0] == h - P).any() and (o[:, 1] == w - P).any()   # the clamped edge tiles are in the list
    o_dev = torch.from_numpy(o).to(dev)
    for t in (3, 4, otsu_np(host)):
        want = counts_np(host, o, P, t)
        counts = tissue.tile_tissue_counts(slide, o_dev, P, t)
        np.testing.assert_array_equal(counts.cpu().numpy(), want)
        for frac in (0.0, 0.25, 0.6, 1.0):
            mp = math.ceil(frac * P * P)
            idx, yx = tissue.select_tiles(counts, o_dev, mp)
            keep = np.flatnonzero(want >= mp)
            np.testing.assert_array_equal(idx.cpu().numpy(), keep)
            np.testing.assert_array_equal(yx.cpu().numpy(), o[keep])
    # a long list: several rounds of the compaction's block scan
    big = np.tile(o, (40, 1))
    counts = tissue.tile_tissue_counts(slide, torch.from_numpy(big).to(dev), P, 4, big)
    mp = math.ceil(0.25 * P * P)
    idx, _ = tissue.select_tiles(counts, torch.from_numpy(big).to(dev), mp)
    np.testing.assert_array_equal(idx.cpu().numpy(), np.flatnonzero(np.tile(counts_np(host, o, P, 4), 40) >= mp))


def test_fill_uncovered_matches_footprints(dev):
    from deephisto_amd import tissue
    h, w, P, d = 900, 1300, 224, 16
    rng = np.random.default_rng(1)
    o = np.stack([rng.integers(0, h - P + 1, 7), rng.integers(0, w - P + 1, 7)], 1).astype(np.int32)
    cmap = torch.arange((h // d) * (w // d), dtype=torch.int64, device=dev).view(h // d, w // d)
    want = cmap.cpu().numpy().copy()
    cover = np.zeros_like(want, bool)
    for y, x in o:
        cover[y // d:(y + P) // d, x // d:(x + P) // d] = True
    want[~cover] = -7
    tissue.fill_uncovered(cmap, torch.from_numpy(o).to(dev), P, d, h, w, -7)
    np.testing.assert_array_equal(cmap.cpu().numpy(), want)
    tissue.fill_uncovered(cmap, torch.empty((0, 2), dtype=torch.int32, device=dev), P, d, h, w, 2)
    assert (cmap == 2).all()


# ---- prediction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,dtype", CONFIGS)
def test_filter_that_keeps_every_tile_changes_no_bit(dev, arch, dtype):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    host = synth.synth_slide(800, 1000, 3)
    model = _model(arch, dtype, dev)
    smp = _sampler(host, 224, 112, 16, dev)
    assert len(smp.origins) > smp.n_tiles   # the corner's padding duplicates are in play
    cmap0, logits0 = predict_full_patched(smp, model, 5, downscale=16, return_logits=True)
    for filt in (TissueFilter("otsu", min_fraction=0.0), TissueFilter(0)):
        info: dict = {}
        cmap1, logits1 = predict_full_patched(smp, model, 5, downscale=16, return_logits=True, tissue=filt, tissue_info=info)
        assert info["n_kept"] == info["n_tiles"] == smp.n_tiles
        np.testing.assert_array_equal(info["kept"], np.arange(smp.n_tiles))
        assert torch.equal(cmap1, cmap0) and torch.equal(logits1, logits0)
    cmap2 = predict_full_patched(smp, model, 5, downscale=16, dedupe_padding=True, tissue=TissueFilter(min_fraction=0.0))
    assert torch.equal(cmap2, predict_full_patched(smp, model, 5, downscale=16, dedupe_padding=True))


@pytest.mark.parametrize("arch,dtype", CONFIGS)
@pytest.mark.parametrize("P,S", [(224, 112), (256, 256)])
def test_painted_slide_matches_oracle(dev, arch, dtype, P, S):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    h, w, d = 1100, 1300, 16
    host = painted(h, w, 7)
    model = _model(arch, dtype, dev)
    smp = _sampler(host, P, S, 16, dev)
    n_unique, origins = smp.n_tiles, smp.origins
    _, logits0 = predict_full_patched(smp, model, 5, downscale=d, return_logits=True)
    logits0 = logits0.cpu().numpy()
    t = otsu_np(host)
    counts = counts_np(host, origins[:n_unique], P, t)
    for filt, mb in ((TissueFilter("otsu"), None), (TissueFilter(t, 0.5, fill_class=3), 32)):
        keep = np.flatnonzero(counts >= math.ceil(filt.min_fraction * P * P))
        assert 0 < len(keep) < n_unique
        info: dict = {}
        cmap, logits = predict_full_patched(smp, model, 5, downscale=d, micro_batch=mb, return_logits=True, tissue=filt,
                                            tissue_info=info)
        assert info["threshold"] == t and info["n_kept"] == len(keep) and info["n_tiles"] == n_unique
        assert info["kept"].dtype == np.int64
        np.testing.assert_array_equal(info["kept"], keep)
        if filt.threshold == "otsu":
            np.testing.assert_array_equal(info["histogram"], np.bincount(chroma_np(host).ravel(), minlength=256))
        else:
            assert "histogram" not in info
        want = masked_map_np(logits0, origins, n_unique, keep, P, d, h, w, filt.fill_class)
        np.testing.assert_array_equal(cmap.cpu().numpy(), want)
        lg = logits.cpu().numpy()
        assert lg.shape == logits0.shape
        rejected = np.setdiff1d(np.arange(n_unique), keep)
        np.testing.assert_array_equal(lg[keep], logits0[keep])
        assert np.isnan(lg[rejected]).all()
    cmap = predict_full_patched(smp, model, 5, downscale=d, dedupe_padding=True, tissue=TissueFilter("otsu"))
    keep = np.flatnonzero(counts >= math.ceil(0.25 * P * P))
    np.testing.assert_array_equal(cmap.cpu().numpy(), masked_map_np(logits0, origins, n_unique, keep, P, d, h, w, -1, dedupe=True))


def test_all_glass_runs_no_forward(dev):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.tissue import TissueFilter
    white = np.full((700, 900, 3), 255, np.uint8)
    grey = white.copy()
    grey[100:300, 100:300] = GREY   # chroma 4: Otsu would split 0 | 4 here, a fixed threshold of 4 rejects it
    model = _model("resnet18", "bf16", dev)
    calls = []
    fwd, name = model.tiles_entry()
    model.tiles_entry = lambda: ((lambda *a: calls.append(1) or fwd(*a)), name)
    for host, filt in ((white, TissueFilter("otsu", fill_class=-1)), (grey, TissueFilter(4, fill_class=2))):
        smp = _sampler(host, 224, 112, 8, dev)
        info: dict = {}
        cmap, logits = predict_full_patched(smp, model, 5, downscale=16, return_logits=True, tissue=filt, tissue_info=info)
        assert info["n_kept"] == 0 and len(info["kept"]) == 0
        assert cmap.shape == (700 // 16, 900 // 16) and (cmap == filt.fill_class).all()
        assert torch.isnan(logits).all()
    assert calls == []
    predict_full_patched(smp, model, 5, downscale=16)
    assert calls   # the wrapper does count launches


def test_refusals(dev, tmp_path):
    from deephisto_amd import tissue
    from deephisto_amd._lib import DeephistoHipError
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import (FullImageDenseSampler, FullImageRndSampler,
                                                            SamplerExecutionMode)
    host = synth.synth_slide(500, 600, 1)
    path = tmp_path / "slide.npy"
    np.save(path, host)
    model = _model("resnet18", "f32", dev)
    disk = FullImageDenseSampler(path, layer=1, patch_size=128, batch_size=8, stride=128, device=dev,
                                 mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    with pytest.raises(ValueError, match="resident"):
        predict_full_patched(disk, model, 5, tissue=tissue.TissueFilter())
    rnd = FullImageRndSampler(host, layer=1, patch_size=128, batch_size=8, device=dev, index_logic="device")
    with pytest.raises(ValueError, match="random sampler"):
        predict_full_patched(rnd, model, 5, tissue=tissue.TissueFilter())
    slide = torch.from_numpy(host).to(dev)
    o = np.array([[0, 0], [400, 480]], np.int32)   # 480 + 128 > 600
    with pytest.raises(DeephistoHipError, match=r"origin 1 \(400, 480\) outside"):
        tissue.tile_tissue_counts(slide, torch.from_numpy(o).to(dev), 128, 10, o)
    counts = tissue.tile_tissue_counts(slide, torch.from_numpy(o).to(dev), 128, 10)   # device-only origins: flagged, not read
    assert counts.cpu().numpy()[1] == -1
    with pytest.raises(DeephistoHipError, match="1 origins lie outside"):
        tissue.select_tiles(counts, torch.from_numpy(o).to(dev), 10)
    with pytest.raises(DeephistoHipError, match="threshold 300"):
        tissue.tile_tissue_counts(slide, torch.from_numpy(o[:1]).to(dev), 128, 300)
    with pytest.raises(DeephistoHipError, match="larger than"):
        tissue.tile_tissue_counts(slide, torch.from_numpy(o[:1]).to(dev), 512, 10)
    with pytest.raises(ValueError, match="uint8"):
        tissue.chroma_histogram(slide.float())
    with pytest.raises(ValueError, match="GPU memory"):
        tissue.chroma_histogram(torch.from_numpy(host))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cli_tissue_two_ranks_equal_single_process(built_lib, tmp_path):
    """`--tissue otsu` through the CLI: two ranks sharing cuda:0 over gloo score the same kept list and give the single-process map."""
    from deephisto_amd.examples.predict_full_patched import main
    args = ["--synthetic", "1500", "1300", "--weights", "", "--patch_size", "224", "--stride", "112", "--batch_size", "16",
            "--tissue", "otsu", "--tissue_min_fraction", "0.6", "--tissue_fill", "BG", "--no_visualizations"]
    pred1 = main(args + ["--out_dir", str(tmp_path / "one")]).cpu().numpy()
    assert pred1.shape == (1500 // 16, 1300 // 16)
    (tmp_path / "run2.py").write_text(
        "import os, sys, numpy as np\n"
        "from examples.predict_full_patched import main\n"
        "pred = main(sys.argv[1:])\n"
        "np.save(f'pred_{os.environ.get(\"RANK\", \"0\")}.npy', pred.cpu().numpy())\n")
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}", DH_DIST_BACKEND="gloo", DH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(tmp_path / "run2.py"), *args, "--out_dir", str(tmp_path / "two")]
    r = subprocess.run(cmd, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("kept ") == 1 and " of 143 tiles, threshold " in r.stdout, r.stdout[-2000:]
    for k in range(2):
        assert np.array_equal(np.load(tmp_path / f"pred_{k}.npy"), pred1), f"rank {k}"
