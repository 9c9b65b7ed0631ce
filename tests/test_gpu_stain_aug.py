"""GPU: the stain-jitter gather (dh_tile_gather_stain_aug) against the NumPy restatement in
tests/helpers/stain_aug_ref.py, bit for bit; the region samplers' `stain_aug=`; `dataset.stain_augment` in the training loop."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import stain_aug_ref as A  # noqa: E402
import stain_ref as R  # noqa: E402

from deephisto_amd import stain as S  # noqa: E402
from deephisto_amd._lib import DH_LAYOUT_NCHW, DH_LAYOUT_NHWC  # noqa: E402

pytestmark = pytest.mark.gpu

HE = np.array(S.TARGET_HE, dtype=np.float64)
H, W = 40, 56
FLIPS = ((False, False), (True, False), (False, True), (True, True))


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def host_slide():
    img = R.synth_he(H, W, 4)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def rows():
    """Five different parameter rows; row 2 is the identity."""
    alpha = np.array([[1.3, 0.8], [0.5, 1.5], [1.0, 1.0], [0.82, 1.17], [1.45, 0.55]])
    beta = np.array([[0.05, -0.02], [-0.1, 0.1], [0.0, 0.0], [0.3, 0.0], [-0.04, -0.3]])
    p = S.jitter_params(HE, alpha, beta)
    p.setflags(write=False)
    return p


def origins(P, n):
    """(0, 0), the far corner, two that hang over the border, one inside; n = 1: one that hangs over the corner's side."""
    o = np.array([[0, 0], [H - P, W - P], [-3, 50], [36, -2], [11, 23]], np.int32)
    return o[3:4] if n == 1 else o


@functools.lru_cache(maxsize=None)
def reference(P, n, fh, fv, nchw):
    ref = A.gather(host_slide(), origins(P, n), P, rows()[3:4] if n == 1 else rows(), fh, fv, nchw)
    ref.setflags(write=False)
    return ref


def run(dev, img, o, P, layout, dtype, params, fh=False, fv=False, host_check=True):
    from deephisto_amd import tiles
    slide = torch.from_numpy(np.array(img)).to(dev)   # np.array: writable copies of the cached, read-only inputs
    return tiles.gather_tiles_stain_aug(slide, torch.from_numpy(np.array(o, dtype=np.int32)).to(dev), P, layout, dtype,
                                        torch.from_numpy(np.array(params, dtype=np.int32)).to(dev), fh, fv,
                                        params_host=params if host_check else None)


def same_bits(got, ref_f32):
    """f32: the float32 bits; bf16: the raw bits of torch's round-to-nearest-even conversion of the float32 reference."""
    if got.dtype == torch.float32:
        return np.array_equal(got.cpu().numpy().view(np.uint32), ref_f32.view(np.uint32))
    want = torch.from_numpy(np.array(ref_f32)).to(torch.bfloat16).view(torch.int16)
    return torch.equal(got.view(torch.int16).cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [DH_LAYOUT_NHWC, DH_LAYOUT_NCHW], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("P", [8, 7])
def test_gather_equals_the_restatement(dev, P, n, layout, dtype):
    nchw = layout == DH_LAYOUT_NCHW
    params = rows()[3:4] if n == 1 else rows()
    for fh, fv in FLIPS:
        got = run(dev, host_slide(), origins(P, n), P, layout, dtype, params, fh, fv)
        assert tuple(got.shape) == ((n, 3, P, P) if nchw else (n, P, P, 3)) and got.dtype == dtype
        ref = reference(P, n, fh, fv, nchw)
        assert same_bits(got, ref), (fh, fv)
        # pixels outside the slide are exactly 0 (the restatement has them at 0; here against the geometry itself)
        _, inside = A.source_pixels(host_slide(), origins(P, n), P, fh, fv)
        g = got.float().cpu().numpy()
        g = g.transpose(0, 2, 3, 1) if nchw else g
        assert not inside.all() and (g[~inside] == 0).all() and (np.signbit(g[~inside]) == 0).all()


def test_more_than_one_workgroup_per_tile_and_rows_that_straddle_them(dev):
    """P = 67: 4 489 pixels, two workgroups per tile, the second starting inside row 61."""
    img = R.synth_he(90, 100, 6)
    o = np.array([[0, 0], [23, 33], [-5, 60], [40, -9]], np.int32)
    params = rows()[[0, 1, 3, 4]]
    for layout, dtype, fh, fv in ((DH_LAYOUT_NCHW, torch.bfloat16, True, False), (DH_LAYOUT_NHWC, torch.float32, False, True),
                                  (DH_LAYOUT_NCHW, torch.float32, True, True)):
        got = run(dev, img, o, 67, layout, dtype, params, fh, fv)
        assert same_bits(got, A.gather(img, o, 67, params, fh, fv, layout == DH_LAYOUT_NCHW))


def test_identity_row_inside_a_jittered_batch_is_the_plain_gather(dev):
    from deephisto_amd import tiles
    slide = torch.from_numpy(np.array(host_slide())).to(dev)
    assert rows()[2].tolist() == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
    for P in (8, 7):
        o = torch.from_numpy(origins(P, 5).copy()).to(dev)
        for layout in (DH_LAYOUT_NHWC, DH_LAYOUT_NCHW):
            for dtype in (torch.float32, torch.bfloat16):
                got = run(dev, host_slide(), origins(P, 5), P, layout, dtype, rows(), True, False)
                plain = tiles.gather_tiles_aug(slide, o, P, layout, dtype, True, False)
                assert torch.equal(got[2], plain[2])
                assert not torch.equal(got[1], plain[1]) and not torch.equal(got[3], plain[3])   # its neighbours are jittered


def test_both_ends_of_the_output_table_clamp(dev):
    img = np.empty((H, W, 3), np.uint8)
    rng = np.random.default_rng(5)
    img[:, :W // 2] = rng.integers(0, 6, (H, W // 2, 3))          # dark half: optical density 3.75 .. 5.5 per channel
    img[:, W // 2:] = rng.integers(250, 256, (H, W - W // 2, 3))  # glass half
    alpha = np.array([[0.1, 0.1], [1.9, 1.9], [1.0, 1.0]])
    beta = np.array([[0.0, 0.0], [0.0, 0.0], [-3.0, -3.0]])       # a bias that drives every o_c negative on glass
    params = S.jitter_params(HE, alpha, beta)
    o = np.array([[0, 0], [10, 3], [20, 30]], np.int32)
    px, _ = A.source_pixels(img, o, 8)
    raw = A.raw_index(px, params)
    assert (raw[1] >= S.LUT_SIZE).any() and (raw[2] < 0).any()   # the restatement reaches both clamps
    for layout in (DH_LAYOUT_NHWC, DH_LAYOUT_NCHW):
        got = run(dev, img, o, 8, layout, torch.float32, params)
        assert same_bits(got, A.gather(img, o, 8, params, nchw=layout == DH_LAYOUT_NCHW))
        assert float(got[1].min()) == 0.0 and float(got[2].max()) == 1.0


def test_entry_refusals_launch_nothing(dev):
    from deephisto_amd._lib import lib
    from deephisto_amd.tiles import _stream
    slide = torch.from_numpy(np.array(host_slide())).to(dev)
    od_dev, _, lut, od = S._tables(dev)
    o = torch.from_numpy(origins(8, 5).copy()).to(dev)
    p_dev = torch.from_numpy(np.array(rows())).to(dev)
    out = torch.full((5, 3, 8, 8), -7.0, device=dev)

    def call(params_host=None, lut_n=S.LUT_SIZE, shift=S.APPLY_SHIFT, n=5, od_host=od, layout=DH_LAYOUT_NCHW):
        return lib().dh_tile_gather_stain_aug(slide.data_ptr(), H, W, o.data_ptr(), p_dev.data_ptr(),
                                              params_host.ctypes.data_as(C.c_void_p) if params_host is not None else None, n, 8,
                                              layout, 0, 0, 0, od_dev.data_ptr(), od_host.ctypes.data_as(C.c_void_p), shift,
                                              lut.data_ptr(), lut_n, out.data_ptr(), _stream(dev))

    bad_matrix, bad_bias, bad_od = np.array(rows()), np.array(rows()), od.copy()
    bad_matrix[3, 4] = S.COEF_MAX + 1
    bad_bias[4, 10] = -(2 ** 30) - 1
    bad_od[17] = S.OD_MAX + 1
    for kw, name in (({"lut_n": S.LUT_SIZE + 1}, b"lut_n"), ({"lut_n": 0}, b"lut_n"), ({"params_host": bad_matrix}, b"params row 3, matrix"),
                     ({"params_host": bad_bias}, b"params row 4, bias"), ({"shift": 40}, b"shift"), ({"n": 65536}, b"n=65536"),
                     ({"od_host": bad_od}, b"od table entry 17"), ({"layout": 2}, b"layout")):
        assert call(**kw) == -22, kw
        assert name in lib().dh_last_error(), (kw, lib().dh_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(n=0) == 0
    assert call(params_host=np.array(rows())) == 0
    torch.cuda.synchronize()
    assert same_bits(out, reference(8, 5, False, False, True))
    with pytest.raises(ValueError, match="params must be int32"):
        run(dev, host_slide(), origins(8, 5), 8, DH_LAYOUT_NCHW, torch.float32, rows()[:4], host_check=False)


# ---- the samplers -----------------------------------------------------------------------------------------------------------
def _bank():
    imgs = [R.synth_he(300, 340, 1, 0.3), R.synth_he(260, 280, 2, 0.5)]
    annos = [[{"class": "TUM", "vertices": [[20, 20], [320, 30], [300, 280], [30, 260]]},
              {"class": "AT", "vertices": [[5, 5], [160, 8], [150, 150], [8, 140]]}],
             [{"class": "BG", "vertices": [[10, 10], [270, 20], [260, 250], [15, 240]]}]]
    return imgs, annos


def test_rnd_sampler_jitters_pixels_only(dev):
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionRndSampler
    imgs, annos = _bank()
    P, B = 32, 4
    make = lambda aug: AnnoRegionRndSampler(list(zip(imgs, annos)), layer=1, patch_size=P, patches_from_one_region=1, device=dev,  # noqa: E731
                                            stain_aug=aug)
    runs = []
    for aug in (S.StainAugmenter(0.2, 0.05, seed=1), None):
        smp = make(aug)
        np.random.seed(21); torch.manual_seed(8)
        runs.append((smp, [(x.cpu().numpy(), lab.cpu().numpy(), c.cpu().numpy()) for x, lab, c in smp.device_batches(B, 2)]))
    (smp, jit), (_, plain) = runs
    # the same stream replayed on the host: one chunk of records, then two coins per batch; the augmenter's own stream apart
    np.random.seed(21); torch.manual_seed(8)
    recs = smp._records(2 * B)
    assert all(len({r[0] for r in recs[B * b:B * b + B]}) == 2 for b in range(2)), "both batches must mix the two slides"
    fits = [R.fit(img, S.StainNormalizer()) for img in imgs]
    replay = S.StainAugmenter(0.2, 0.05, seed=1)
    for b in range(2):
        fh, fv = torch.rand(1).item() < 0.5, torch.rand(1).item() < 0.5
        alpha, beta = replay.draw(B)
        assert np.array_equal(jit[b][1], plain[b][1]) and np.array_equal(jit[b][2], plain[b][2])
        assert jit[b][1].tolist() == [r[3] for r in recs[B * b:B * b + B]]
        assert not np.array_equal(jit[b][0], plain[b][0])
        for i, (j, y, x, _cls) in enumerate(recs[B * b:B * b + B]):
            assert not fits[j].identity and np.array_equal(smp._bank.basis(j), np.array(fits[j].HE))
            params = S.jitter_params(fits[j].HE, alpha[i:i + 1], beta[i:i + 1])
            want = A.gather(imgs[j], [[y, x]], P, params, fh, fv, nchw=True)[0]
            assert np.array_equal(jit[b][0][i].view(np.uint32), want.view(np.uint32)), (b, i)
            assert np.array_equal(plain[b][0][i].view(np.uint32), A.plain(imgs[j], [[y, x]], P, fh, fv, nchw=True)[0].view(np.uint32))
    # stain_aug=False leaves the augmenter out (and its stream where it is)
    np.random.seed(21); torch.manual_seed(8)
    off = [x.cpu().numpy() for x, _, _ in smp.device_batches(B, 2, stain_aug=False)]
    assert all(np.array_equal(a, p[0]) for a, p in zip(off, plain))


def test_normalised_bank_is_jittered_in_the_target_basis(dev):
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionRndSampler
    imgs, annos = _bank()
    norm = S.StainNormalizer()
    smp = AnnoRegionRndSampler([(imgs[0], annos[0])], layer=1, patch_size=32, device=dev, stain=norm,
                               stain_aug=S.StainAugmenter(0.3, 0.02, seed=2))
    np.random.seed(5); torch.manual_seed(1)
    x, _, c = next(smp.device_batches(4, 1, flips=False))
    assert np.array_equal(smp._bank.basis(0), HE)
    mapped, _ = R.normalize(imgs[0], norm)
    alpha, beta = S.StainAugmenter(0.3, 0.02, seed=2).draw(4)
    want = A.gather(mapped, c.cpu().numpy().astype(np.int64), 32, S.jitter_params(HE, alpha, beta), nchw=True)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_all_glass_slide_is_left_unjittered(dev):
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionDenseSampler, AnnoRegionRndSampler
    glass = np.random.default_rng(3).integers(236, 256, (200, 220, 3), dtype=np.uint8)
    anno = [{"class": "BG", "vertices": [[10, 10], [210, 12], [205, 190], [12, 185]]}]
    out = []
    for aug in (S.StainAugmenter(0.9, 0.5, seed=4), None):
        smp = AnnoRegionRndSampler([(glass, anno)], layer=1, patch_size=32, device=dev, stain_aug=aug)
        np.random.seed(2); torch.manual_seed(2)
        out.append(torch.cat([x for x, _, _ in smp.device_batches(4, 2)]))
        if aug is not None:
            assert smp._bank.basis(0) is None
    assert torch.equal(out[0], out[1])
    dense = [torch.cat([x for x, _, _ in AnnoRegionDenseSampler([(glass, anno)], layer=1, patch_size=32, stride=40, device=dev,
                                                                  stain_aug=aug).device_batches(8)])
             for aug in (S.StainAugmenter(0.9, 0.5, seed=4), None)]
    assert len(dense[0]) > 8 and torch.equal(dense[0], dense[1])


def test_dense_sampler_draws_one_row_per_patch(dev):
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionDenseSampler
    imgs, annos = _bank()
    smp = AnnoRegionDenseSampler([(imgs[1], annos[1])], layer=1, patch_size=32, stride=48, device=dev,
                                 stain_aug=S.StainAugmenter(0.2, 0.05, seed=6))
    fit = R.fit(imgs[1], S.StainNormalizer())
    replay = S.StainAugmenter(0.2, 0.05, seed=6)
    n = 0
    for x, _, c in smp.device_batches(8, DH_LAYOUT_NHWC, torch.bfloat16):
        alpha, beta = replay.draw(len(x))
        want = A.gather(imgs[1], c.cpu().numpy().astype(np.int64), 32, S.jitter_params(fit.HE, alpha, beta))
        assert same_bits(x, want)
        n += len(x)
    assert n > 8   # more than one batch, the last one ragged or not


# ---- training ---------------------------------------------------------------------------------------------------------------
class _Recorder:
    """A sampler that keeps a copy of every batch it hands out, call by call."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    @property
    def stain_aug(self):
        return self.inner.stain_aug

    @stain_aug.setter
    def stain_aug(self, aug):
        self.inner.stain_aug = aug

    def device_batches(self, *args, **kwargs):
        got = []
        self.calls.append((kwargs, got))
        for x, lab, c in self.inner.device_batches(*args, **kwargs):
            got.append(x.clone())
            yield x, lab, c


def test_training_with_the_config_option(dev, tmp_path):
    """Two training steps with `dataset.stain_augment`: finite loss, jittered training batches, validation batches bitwise those
    of a run without the option."""
    from deephisto_amd.models.patch_cls_simple.train import train
    from deephisto_amd.patch_samplers.region_samplers import RectRegion, RectRegionRndSampler
    side = 512
    host = R.synth_he(side, side, 7, glass=0.2)
    regions = [RectRegion(name, 100 * i, 0, 100 * i + 100, side) for i, name in enumerate(["AT", "BG", "LP", "MM", "TUM"])]
    calls = []
    for option in ({"stain_augment": {"sigma_alpha": 0.2, "sigma_beta": 0.05, "seed": 3}}, {}):
        smp = _Recorder(RectRegionRndSampler(host, regions, layer=1, patch_size=64, seed=0, device=dev))
        cfg = {"model": {"n_classes": 5},
               "training": {"batch_size": 16, "n_epochs": 1, "lr": 1e-3, "save_dir": str(tmp_path / "ck"),
                            "out_dir": str(tmp_path / "out"), "val_steps": 2},
               "dataset": {"folder": "/nonexistent", "layer": 1, "patch_size": 64, "patches_from_one_region": 4, **option}}
        torch.manual_seed(0)
        _, hist = train(cfg, sampler=smp, epochs=1, steps_per_epoch=2, log=lambda *a: None)
        assert np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["val_loss"][0])
        assert len(smp.calls) == 2 and [len(c[1]) for c in smp.calls] == [2, 2]
        calls.append(smp.calls)
    (train_on, val_on), (train_off, val_off) = calls
    assert val_on[0].get("stain_aug") is False and "stain_aug" not in train_on[0] and "stain_aug" not in val_off[0]
    assert all(torch.equal(a, b) for a, b in zip(val_on[1], val_off[1]))
    assert not any(torch.equal(a, b) for a, b in zip(train_on[1], train_off[1]))
