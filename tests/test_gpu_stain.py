"""GPU: Macenko stain normalisation against the NumPy restatement in tests/helpers/stain_ref.py.

Every device result -- the ten moments, the angle histogram, the two concentration histograms, the applied slide -- is an integer
function of the bytes and is compared bit for bit.  With `stain=` the prediction functions and the region samplers give exactly
what they give over the normalised slide.  The largest slide here has 8.4e6 pixels; the four passes over 1.4e9 pixels (offsets past 2^32
bytes, the counters at slide scale) are held by tests/test_gpu_slide_scale.py."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import stain_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# fixed-point operands with mixed signs, so that every quadrant and both clamps of every pass are reached whatever the content
E_FIX = np.array([[9000, -12000, 5000], [-7000, 3000, 11000]], np.int32)
P_FIX = np.array([[9000, -3000, -1500], [-5200, 7000, 800]], np.int32)
M_FIX = np.array([[5000, -900, 300], [-2000, 6000, 100], [700, -400, 3500]], np.int32)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def content(kind, h, w, seed=0):
    if kind == "he":
        return R.synth_he(h, w, seed + 1, glass=0.4)
    if kind == "glass":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    assert kind == "random"
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def check_fixed(host, slide, norm):
    """The four passes with the fixed operands; returns the moments."""
    from deephisto_amd import stain as S
    mom = R.moments(host, norm.vmax)
    np.testing.assert_array_equal(S.stain_moments(slide, norm.vmax), mom)
    np.testing.assert_array_equal(S.angle_histogram(slide, norm.vmax, E_FIX), R.angle_hist(host, norm.vmax, E_FIX))
    np.testing.assert_array_equal(S.conc_histogram(slide, norm.vmax, P_FIX), R.conc_hist(host, norm.vmax, P_FIX))
    np.testing.assert_array_equal(S.apply_fixed(slide, M_FIX).cpu().numpy(), R.apply_fixed(host, M_FIX))
    return mom


def check_passes(host, slide, norm):
    """Moments, both histograms (the fitted operands when the slide has a plane, fixed ones always), the fit and the applied
    slide of `slide` (device) equal the restatement's on `host`."""
    from deephisto_amd import stain as S
    mom = check_fixed(host, slide, norm)
    want = R.fit(host, norm)
    got = norm.fit(slide)
    assert got.to_json() == want.to_json()          # every number of the fit: same integers in, same host math
    if not want.identity:
        evec_q, _ = S.plane_from_moments(mom)
        np.testing.assert_array_equal(S.angle_histogram(slide, norm.vmax, evec_q), R.angle_hist(host, norm.vmax, evec_q))
        pinv_q = S.quantize_coef(S.pinv32(want.HE), "pinv")
        np.testing.assert_array_equal(S.conc_histogram(slide, norm.vmax, pinv_q), R.conc_hist(host, norm.vmax, pinv_q))
    np.testing.assert_array_equal(norm.apply(slide, got).cpu().numpy(), R.apply(host, norm, want))
    return got


@pytest.mark.parametrize("kind", ["he", "glass", "black", "random"])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 53), (64, 64)])
def test_passes_equal_the_restatement(dev, h, w, kind):
    """1 x 1; 3 x 5 (tail only, no full group); 37 x 53 (h*w % 16 = 9); 64 x 64 (full groups only).  All glass: identity fit,
    output unchanged.  All black: the accumulators' worst case per pixel.  Uniform random bytes: every bin busy."""
    from deephisto_amd.stain import StainNormalizer
    host = content(kind, h, w, seed=h * w)
    slide = torch.from_numpy(host).to(dev)
    norm = StainNormalizer()
    fit = check_passes(host, slide, norm)
    assert torch.equal(slide.cpu(), torch.from_numpy(host))          # the slide itself is untouched
    if kind in ("glass", "black") or h * w < 16:
        assert fit.identity and fit.HE is None
        assert torch.equal(norm.normalize(slide), slide)
    if kind == "glass":
        assert fit.n_stained == 0
    if kind == "black":
        assert fit.n_stained == h * w and fit.moments[4] == h * w * 22713 ** 2
    if kind in ("he", "random") and h * w >= 37 * 53:
        assert not fit.identity


def test_unaligned_view_goes_through_the_clone(dev):
    """300 x 517 as a contiguous view 5 bytes past a 16-byte boundary: every entry clones it; out= an unaligned tensor too."""
    from deephisto_amd.stain import StainNormalizer
    host = content("he", 300, 517, 7)
    buf = torch.empty(host.size + 5, dtype=torch.uint8, device=dev)
    buf[5:] = torch.from_numpy(host.reshape(-1)).to(dev)
    view = buf[5:].view(300, 517, 3)
    assert view.data_ptr() % 16 and view.is_contiguous()
    norm = StainNormalizer()
    fit = check_passes(host, view, norm)
    want = R.apply(host, norm, fit)
    assert norm.apply(view, fit, out=view) is view                    # in place on the unaligned view
    np.testing.assert_array_equal(view.cpu().numpy(), want)


def test_grid_stride_loop_runs_twice(dev):
    """The grid is capped at 2 048 workgroups of 256 lanes, 16 pixels per lane and sweep: 8 388 608 pixels.  2 900 x 2 901 =
    8 412 900 pixels (% 16 = 4) is just past it, so the first lanes take a second group.  The four passes with the fixed operands
    (the restatement of this size is what takes the seconds)."""
    from deephisto_amd.stain import StainNormalizer
    cap = 2048 * 256 * 16
    h, w = 2900, 2901
    assert cap < h * w < cap + cap // 256 and (h * w) % 16 == 4
    host = content("random", h, w, 3)
    host[:700] = 255                                                  # a glass band: long runs with no bin
    host[700:1400] = np.tile(R.synth_he(70, w, 5), (10, 1, 1))        # and real clusters
    check_fixed(host, torch.from_numpy(host).to(dev), StainNormalizer())


def test_exactly_the_minimum_of_stained_pixels(dev):
    from deephisto_amd.stain import MIN_STAINED, StainNormalizer
    norm = StainNormalizer()
    he = R.synth_he(64, 64, 9, glass=0.0).reshape(-1, 3)
    he = he[he.max(1) <= norm.vmax]
    for n, identity in ((MIN_STAINED, False), (MIN_STAINED - 1, True)):
        host = np.full((37, 53, 3), 255, np.uint8)
        host.reshape(-1, 3)[np.arange(n) * 97 + 11] = he[:n]
        fit = check_passes(host, torch.from_numpy(host).to(dev), norm)
        assert fit.n_stained == n and fit.identity == identity


def test_in_place_equals_out_of_place(dev):
    from deephisto_amd.stain import StainNormalizer
    host = content("he", 301, 211, 4)
    slide = torch.from_numpy(host).to(dev)
    norm = StainNormalizer()
    fit = norm.fit(slide)
    out = norm.apply(slide, fit)
    assert out.data_ptr() != slide.data_ptr() and torch.equal(slide.cpu(), torch.from_numpy(host))
    other = torch.empty_like(slide)
    assert norm.apply(slide, fit, out=other) is other and torch.equal(other, out)
    assert norm.apply(slide, fit, out=slide) is slide and torch.equal(slide, out)
    np.testing.assert_array_equal(out.cpu().numpy(), R.apply(host, norm, fit))


def test_target_from_another_slide(dev):
    from deephisto_amd.stain import StainFit, StainNormalizer
    a, b = content("he", 200, 260, 1), np.clip(content("he", 180, 333, 2).astype(np.int32) * 3 // 4 + 30, 0, 255).astype(np.uint8)
    fit_a = StainNormalizer().fit(torch.from_numpy(a).to(dev))
    fit_a = StainFit.from_json(fit_a.to_json())
    to_a = StainNormalizer(target=fit_a)
    info = {}
    got = to_a.normalize(torch.from_numpy(b).to(dev), info)
    want, fit_b = R.normalize(b, to_a)
    assert info["fit"].to_json() == fit_b.to_json() and not fit_b.identity
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, R.normalize(b, StainNormalizer())[0])   # the target matters


def test_refusals(dev):
    from deephisto_amd import stain as S
    from deephisto_amd._lib import DeephistoHipError, lib
    slide = torch.from_numpy(content("he", 20, 20)).to(dev)
    with pytest.raises(ValueError, match="uint8"):
        S.stain_moments(slide.float(), 219)
    with pytest.raises(ValueError, match="GPU memory"):
        S.stain_moments(slide.cpu(), 219)
    with pytest.raises(DeephistoHipError, match="eigenvector component"):
        S.angle_histogram(slide, 219, E_FIX * 4)
    with pytest.raises(DeephistoHipError, match="matrix entry"):
        S.apply_fixed(slide, M_FIX * 1000)
    with pytest.raises(DeephistoHipError, match="must be the slide itself or not overlap"):
        flat = torch.zeros(20 * 20 * 3 + 48, dtype=torch.uint8, device=dev)
        S.apply_fixed(flat[:1200].view(20, 20, 3), M_FIX, out=flat[48:].view(20, 20, 3))
    assert lib().dh_stain_max_pixels() == S.MAX_PIXELS >= 50_000 ** 2
    od = S.od_table()
    import ctypes as C
    rc = lib().dh_stain_moments(slide.data_ptr(), 1 << 20, 1 << 20, slide.data_ptr(), od.ctypes.data_as(C.c_void_p), 219,
                                slide.data_ptr(), None)     # refused by name before any launch
    assert rc == -22 and b"max_pixels" in lib().dh_last_error()


# ---- through the public interface ---------------------------------------------------------------------------------------------
def _model(dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(0)
    return get_model(5, dtype, arch="resnet18").to(dev).eval()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b)) if a.is_floating_point() else torch.equal(a, b)


@pytest.fixture(scope="module")
def slide600(dev):
    host = R.synth_he(600, 600, 12, glass=0.5)
    host[:, 380:] = 255                       # a glass margin, so the tissue filter rejects tiles
    return host


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_prediction_equals_prediction_on_the_normalised_slide(dev, slide600, dtype):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched, predict_random_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, FullImageRndSampler
    from deephisto_amd.stain import StainNormalizer
    from deephisto_amd.tissue import TissueFilter
    norm, model = StainNormalizer(), _model(dtype, dev)
    raw = torch.from_numpy(slide600).to(dev)
    normed = norm.normalize(raw)
    np.testing.assert_array_equal(normed.cpu().numpy(), R.normalize(slide600, norm)[0])
    assert not torch.equal(normed, raw)
    kw = dict(layer=1, patch_size=128, batch_size=8, stride=96, device=dev)
    a, b = FullImageDenseSampler(raw, **kw), FullImageDenseSampler(normed, **kw)
    for tissue in (None, TissueFilter("otsu")):
        ia, ib, sinfo = {}, {}, {}
        got = predict_full_patched(a, model, 5, return_logits=True, return_proba=True, tissue=tissue, tissue_info=ia,
                                   stain=norm, stain_info=sinfo)
        want = predict_full_patched(b, model, 5, return_logits=True, return_proba=True, tissue=tissue, tissue_info=ib)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        assert _same(got[2].proba, want[2].proba) and _same(got[2].count, want[2].count) and _same(got[2].class_map, want[2].class_map)
        assert sinfo["fit"].to_json() == R.fit(slide600, norm).to_json()
        if tissue is not None:
            assert ia["threshold"] == ib["threshold"] and np.array_equal(ia["kept"], ib["kept"])
            assert np.array_equal(ia["histogram"], ib["histogram"]) and 0 < ia["n_kept"] < ia["n_tiles"]
    assert torch.equal(a.data_device, raw) and torch.equal(raw.cpu(), torch.from_numpy(slide600))
    kw = dict(layer=1, patch_size=128, batch_size=8, device=dev, index_logic="device")
    np.random.seed(3)
    ra = FullImageRndSampler(raw, **kw)
    got = predict_random_patched(ra, model, 5, return_canvas=True, stain=norm)
    np.random.seed(3)
    want = predict_random_patched(FullImageRndSampler(normed, **kw), model, 5, return_canvas=True)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert torch.equal(ra.data_device, raw)


def test_streamed_sampler_is_refused(dev, slide600, tmp_path):
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, SamplerExecutionMode
    from deephisto_amd.stain import StainNormalizer
    np.save(tmp_path / "slide.npy", slide600)
    disk = FullImageDenseSampler(tmp_path / "slide.npy", layer=1, patch_size=128, batch_size=8, stride=128, device=dev,
                                 mode=SamplerExecutionMode.ONDISK_MULTIPROC)
    with pytest.raises(ValueError, match="stain normalisation needs an HBM-resident slide"):
        predict_full_patched(disk, _model("f32", dev), 5, stain=StainNormalizer())


def test_region_samplers_cut_from_the_normalised_slide(dev):
    """With `stain`, a device batch equals the batch cut by hand from the normalised slide at the same origins and flips, and
    host_patch shows the same pixels; the caller's arrays are left as they are."""
    from deephisto_amd.patch_samplers.region_samplers import (AnnoRegionDenseSampler, AnnoRegionRndSampler, RectRegion,
                                                              RectRegionRndSampler)
    from deephisto_amd.stain import StainNormalizer
    norm = StainNormalizer()
    img0, img1 = R.synth_he(500, 620, 1, 0.3), R.synth_he(420, 400, 2, 0.6)
    normed = [R.normalize(img0, norm)[0], R.normalize(img1, norm)[0]]
    a0 = [{"class": "TUM", "vertices": [[30, 40], [590, 30], [600, 470], [20, 480]]}]
    a1 = [{"class": "LP", "vertices": [[10, 10], [390, 20], [380, 400], [15, 390]]}]
    smp = AnnoRegionRndSampler([(img0, a0), (img1, a1)], layer=1, patch_size=96, patches_from_one_region=4, device=dev, stain=norm)
    np.random.seed(22); torch.manual_seed(5)
    recs = smp._records(8)
    np.random.seed(22); torch.manual_seed(5)
    fh = torch.rand(1).item() < 0.5
    fv = torch.rand(1).item() < 0.5
    torch.manual_seed(5)
    x, lab, c = next(smp.device_batches(8, 1))
    for i, (j, y, xx, cls) in enumerate(recs):
        want = torch.from_numpy(normed[j][y:y + 96, xx:xx + 96].astype(np.float32) / 255).permute(2, 0, 1)
        if fh: want = torch.flip(want, dims=[2])
        if fv: want = torch.flip(want, dims=[1])
        assert torch.equal(x[i].cpu(), want)
        np.testing.assert_array_equal(smp._bank.host_patch(j, y, xx, 96), normed[j][y:y + 96, xx:xx + 96])
    dense = AnnoRegionDenseSampler([(img1, a1)], layer=1, patch_size=128, stride=128, device=dev, stain=norm)
    patches = [p for p, _ in dense.structs_generator()]
    xs = torch.cat([b[0] for b in dense.device_batches(4, layout=0)])
    assert len(patches) == len(xs) > 0
    for p, t in zip(patches, xs):
        np.testing.assert_array_equal(p.data, normed[1][p.pos_y:p.pos_y + 128, p.pos_x:p.pos_x + 128])
        np.testing.assert_array_equal(t.cpu().numpy(), p.data.astype(np.float32) / 255)
    dev_img = torch.from_numpy(img0).to(dev)
    rect = RectRegionRndSampler(dev_img, [RectRegion("TUM", 0, 0, 500, 620)], layer=1, patch_size=64, seed=1, device=dev, stain=norm)
    np.testing.assert_array_equal(rect.slide.cpu().numpy(), normed[0])
    assert torch.equal(dev_img.cpu(), torch.from_numpy(img0))
    plain = RectRegionRndSampler(dev_img, [RectRegion("TUM", 0, 0, 500, 620)], layer=1, patch_size=64, seed=1, device=dev)
    assert torch.equal(plain.slide, dev_img)


def test_cli_saves_a_fit_and_takes_it_as_target(built_lib, tmp_path):
    """`--synthetic 600 600 --stain macenko --save_stain_fit`, then a second run with `--stain_target` of that file, each in a
    fresh child process: the saved fit reloads to equal numbers and the outputs exist."""
    from deephisto_amd.stain import StainFit
    env = dict(os.environ, PYTHONPATH=f"{REPO / 'compat'}:{REPO}")
    base = [sys.executable, "-m", "examples.predict_full_patched", "--synthetic", "600", "600", "--weights", "", "--patch_size", "128",
            "--stride", "128", "--batch_size", "8", "--stain", "macenko"]
    for k, extra in enumerate((["--save_stain_fit", str(tmp_path / "fit.json")],
                               ["--stain_target", str(tmp_path / "fit.json"), "--save_stain_fit", str(tmp_path / "fit2.json")])):
        r = subprocess.run(base + ["--out_dir", str(tmp_path / f"out{k}")] + extra, env=env, cwd=tmp_path, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "stain:" in r.stdout
        for f in ("synthetic_600x600_mask.jpg", "synthetic_600x600.jpg", "synthetic_600x600_overlay.jpg"):
            assert (tmp_path / f"out{k}" / f).stat().st_size > 0
    text = (tmp_path / "fit.json").read_text()
    fit = StainFit.from_json(text)
    assert fit.to_json() == text and fit.n_stained == fit.moments[0]
    assert StainFit.from_json((tmp_path / "fit2.json").read_text()) == fit        # the fit does not depend on the target
