"""Host math of the rotation and scale augmentation: the fixed-point rows, the NumPy restatement against
plain float64 bilinear sampling under a derived bound, the augmenter's private stream, the refusals and the config entry.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import geom_aug_ref as G  # noqa: E402
import stain_aug_ref as A  # noqa: E402
import stain_ref as R  # noqa: E402

from deephisto_amd import geom_aug as GA  # noqa: E402
from deephisto_amd import stain as S  # noqa: E402

IDENTITY = [32768, 0, 0, 32768]
QUARTER = [0, -32768, 32768, 0]
FLIPS = ((False, False), (True, False), (False, True), (True, True))


def test_rows_are_the_stated_formula():
    assert GA.affine_params(0, 1).tolist() == [IDENTITY] and GA.affine_params(0, 1).dtype == np.int32
    assert GA.affine_params(0.0, 1.0).shape == (1, 4)
    assert GA.affine_params(90, 1).tolist() == [QUARTER]
    assert GA.affine_params(180, 1).tolist() == [[-32768, 0, 0, -32768]]
    assert GA.affine_params(-90, 2).tolist() == [[0, 65536, -65536, 0]]
    assert GA.affine_params(np.zeros(0), np.zeros(0)).shape == (0, 4)
    th, s = np.array([37.0, -143.5, 12.25]), np.array([0.5, 1.3, 2.0])
    m = GA.affine_params(th, s)
    c, sn = s * np.cos(np.deg2rad(th)), s * np.sin(np.deg2rad(th))
    assert np.abs(m - np.stack([c, -sn, sn, c], 1) * 32768).max() <= 0.5 + 1e-9
    assert np.abs(m).max() <= GA.COEF_MAX == 2 ** 16
    assert GA.affine_params(45.0, np.array([0.5, 2.0])).shape == (2, 4)   # a scalar broadcasts


def test_identity_and_quarter_turn_land_on_integer_pixels():
    """The two properties the device tests rest on, on the restatement: for every P, x0 and sx the identity row gives
    X = 65536 (x0 + sx), so v is the plain gather's byte; the quarter-turn row gives out[r][c] = patch[c][P - 1 - r]."""
    img = R.synth_he(40, 52, 5)
    o = np.array([[-3, 47], [36, -2], [11, 23], [0, 0], [33, 45]], np.int64)
    for P in (8, 7):
        for fh, fv in FLIPS:
            x, y = G.coordinates(o, P, [IDENTITY] * 5, fh, fv)
            assert not (x & 65535).any() and not (y & 65535).any()
            got = G.gather(img, o, P, [IDENTITY] * 5, fh, fv)
            assert np.array_equal(got.view(np.uint32), A.plain(img, o, P, fh, fv).view(np.uint32))
        x, y = G.coordinates(o, P, [QUARTER] * 5)
        assert not (x & 65535).any() and not (y & 65535).any()
        inner = np.array([[11, 23], [20, 30]], np.int64)
        turned = G.gather(img, inner, P, [QUARTER] * 2)
        assert np.array_equal(turned, np.rot90(A.plain(img, inner, P), 1, axes=(1, 2)))   # counter-clockwise as displayed
    # with stain rows: the identity affine row in front of the jitter chain is the jitter restatement itself
    params = S.jitter_params(np.array(S.TARGET_HE), np.array([[1.3, 0.8]] * 5), np.array([[0.05, -0.02]] * 5))
    for fh, fv in FLIPS:
        got = G.gather(img, o, 8, [IDENTITY] * 5, fh, fv, params=params)
        assert np.array_equal(got.view(np.uint32), A.gather(img, o, 8, params, fh, fv).view(np.uint32))


@pytest.mark.parametrize("P", [8, 33])
def test_restatement_against_float64_bilinear_sampling(P):
    """Bound, derived: the coordinate error per axis is at most delta = 2^-8 (the weights keep 8 fraction bits, truncated) +
    P 2^-16 (two Q15 coefficients, each off by at most half a unit, times |U2|, |V2| <= P, in Q16); bilinear interpolation
    moves by at most g per pixel per axis, g the largest absolute difference between adjacent pixels; the result is rounded
    once (0.5).  So |v - exact| <= 0.5 + 2 g delta (+ 1e-9 for float rounding), asserted on every pixel with g the test
    image's own largest adjacent difference; taps outside the image are zero on both sides.  The report splits the worst error
    into pixels whose taps all lie inside the image and the rest."""
    img = R.synth_he(96, 128, 3)
    h, w = img.shape[:2]
    f = img.astype(np.int64)
    g = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
    rng = np.random.default_rng(P)
    n = 200
    theta, s = rng.uniform(-180.0, 180.0, n), rng.uniform(0.5, 2.0, n)
    o = np.stack([rng.integers(-P // 2, h - P // 2, n), rng.integers(-P // 2, w - P // 2, n)], 1)
    rows = GA.affine_params(theta, s)
    v, live = G.blend(img, o, P, rows)
    exact, x, y = G.sample_float64(img, o, P, theta, s)
    xq, yq = G.coordinates(o, P, rows)
    delta = 2.0 ** -8 + P * 2.0 ** -16
    assert np.abs(xq / 65536.0 - x).max() <= P * 2.0 ** -16 + 1e-9 and np.abs(yq / 65536.0 - y).max() <= P * 2.0 ** -16 + 1e-9
    inner = ((np.minimum(np.floor(x), xq >> 16) >= 0) & (np.maximum(np.floor(x), xq >> 16) <= w - 2) &
             (np.minimum(np.floor(y), yq >> 16) >= 0) & (np.maximum(np.floor(y), yq >> 16) <= h - 2))
    assert inner.any() and not inner.all()            # both kinds of pixel are exercised
    assert not live.all() and (v[~live] == 0).all()   # some windows leave the image altogether
    err = np.abs(v.astype(np.float64) - exact).max(axis=-1)
    bound = 0.5 + 2.0 * g * delta + 1e-9
    print(f"P={P}: g={g}, delta={delta:.6f}, bound {bound:.4f}, worst |v - exact| inside {err[inner].max():.4f}, "
          f"at the border {err[~inner].max():.4f}")
    assert (err <= bound).all()


def test_refusals_name_the_argument():
    for kw, name in (({"rotate_deg": 180.5}, "rotate_deg"), ({"rotate_deg": -1.0}, "rotate_deg"), ({"rotate_deg": float("nan")}, "rotate_deg"),
                     ({"rotate_deg": "90"}, "rotate_deg"), ({"scale": (0.4, 1.0)}, r"scale\[0\]"), ({"scale": (1.0, 2.5)}, r"scale\[1\]"),
                     ({"scale": (1.2, 0.9)}, "scale"), ({"scale": 1.0}, "scale"), ({"scale": (1.0, float("nan"))}, r"scale\[1\]"),
                     ({"seed": -1}, "seed"), ({"seed": 1.5}, "seed"), ({"seed": True}, "seed")):
        with pytest.raises(ValueError, match=name):
            GA.GeometricAugmenter(**kw)
    GA.GeometricAugmenter(0.0, (0.5, 2.0))            # the ends of the ranges are accepted
    GA.GeometricAugmenter(180.0, (2.0, 2.0), seed=2 ** 40)
    with pytest.raises(ValueError, match="s must lie"):
        GA.affine_params(0.0, 2.01)
    with pytest.raises(ValueError, match="s must lie"):
        GA.affine_params(0.0, float("nan"))
    with pytest.raises(ValueError, match="theta_deg"):
        GA.affine_params(float("inf"), 1.0)


def test_draw_is_reproducible_and_private():
    np.random.seed(7)
    torch.manual_seed(7)
    np_state, torch_state = np.random.get_state(), torch.get_rng_state()
    a = GA.GeometricAugmenter(30.0, (0.8, 1.25), seed=3)
    theta, s = a.draw(64)
    assert theta.dtype == s.dtype == np.float64 and theta.shape == s.shape == (64,)
    # one uniform(size=(n, 2)) call of PCG64(seed), columns (theta, s)
    u = np.random.Generator(np.random.PCG64(3)).uniform(size=(64, 2))
    assert np.array_equal(theta, 30.0 * (2.0 * u[:, 0] - 1.0)) and np.array_equal(s, 0.8 + (1.25 - 0.8) * u[:, 1])
    assert np.abs(theta).max() <= 30.0 and np.abs(theta).max() > 25.0 and s.min() >= 0.8 and s.max() <= 1.25 and s.max() - s.min() > 0.3
    assert not np.array_equal(theta, a.draw(64)[0])                      # the stream moves on
    assert not np.array_equal(theta, GA.GeometricAugmenter(30.0, (0.8, 1.25), seed=4).draw(64)[0])
    zero = GA.GeometricAugmenter(0.0, (1.0, 1.0))
    assert zero.rows(5).tolist() == [IDENTITY] * 5
    # the same rows whether or not a StainAugmenter (same seed) drew in between
    b, c, st = GA.GeometricAugmenter(30.0, (0.8, 1.25), seed=3), GA.GeometricAugmenter(30.0, (0.8, 1.25), seed=3), S.StainAugmenter(0.2, 0.05, seed=3)
    first = b.rows(16)
    st.draw(16)
    second = b.rows(16)
    assert np.array_equal(np.concatenate([first, second]), c.rows(32)) and first.dtype == np.int32
    alone = S.StainAugmenter(0.2, 0.05, seed=3)   # and the stain stream is where it is without the geometric draws
    alone.draw(16)
    assert np.array_equal(st.draw(8)[0], alone.draw(8)[0])
    state = np.random.get_state()
    assert state[0] == np_state[0] and np.array_equal(state[1], np_state[1]) and state[2:] == np_state[2:]
    assert torch.equal(torch.get_rng_state(), torch_state)


def test_record_stream_does_not_depend_on_the_augmenter():
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionDenseSampler, AnnoRegionRndSampler
    imgs = [R.synth_he(300, 340, 1), R.synth_he(260, 280, 2)]
    annos = [[{"class": "TUM", "vertices": [[20, 20], [320, 30], [300, 280], [30, 260]]}],
             [{"class": "BG", "vertices": [[10, 10], [270, 20], [260, 250], [15, 240]]}]]
    streams = []
    for aug in (None, GA.GeometricAugmenter(0.0), GA.GeometricAugmenter(180.0, (0.5, 2.0), seed=1)):
        smp = AnnoRegionRndSampler(list(zip(imgs, annos)), layer=1, patch_size=32, device="cpu", geom_aug=aug)
        assert smp.geom_aug is aug and smp.stain_aug is None
        np.random.seed(11)
        streams.append(smp._records(24))
    assert streams[0] == streams[1] == streams[2] and len(streams[0]) == 24
    aug = GA.GeometricAugmenter(10.0)
    dense = AnnoRegionDenseSampler(list(zip(imgs, annos)), layer=1, patch_size=32, stride=48, device="cpu", geom_aug=aug)
    assert dense.geom_aug is aug
    dense.geom_aug = None
    assert dense.geom_aug is None


def test_config_entry():
    from deephisto_amd.models.patch_cls_simple.train import _geom_aug_from_cfg
    assert _geom_aug_from_cfg({"dataset": {}}) is None and _geom_aug_from_cfg({}) is None
    aug = _geom_aug_from_cfg({"dataset": {"geom_augment": {"rotate_deg": 45, "scale_min": 0.8, "scale_max": 1.25, "seed": 5}}}, rank=2)
    assert (aug.rotate_deg, aug.scale, aug.seed) == (45.0, (0.8, 1.25), 7)   # data parallel: seed + rank
    dflt = _geom_aug_from_cfg({"dataset": {"geom_augment": {}}})
    assert (dflt.rotate_deg, dflt.scale, dflt.seed) == (180.0, (1.0, 1.0), 0)
    for entry, name in (({"rotate": 10}, "rotate"), ({"rotate_deg": 200}, "rotate_deg"), ({"scale_min": 0.3}, "scale_min"),
                        ({"scale_max": "big"}, "scale_max"), ({"scale_min": 1.5, "scale_max": 1.2}, "scale_min"),
                        ({"seed": 1.5}, "seed"), ({"seed": -2}, "seed"), ("on", "must be a mapping"), ([10, 1.0], "must be a mapping")):
        with pytest.raises(ValueError, match=rf"dataset\.geom_augment.*{name}"):
            _geom_aug_from_cfg({"dataset": {"geom_augment": entry}})


def test_bounds_stay_below_their_limits():
    b = GA.overflow_bounds()
    assert b["coef_product"] == (2 ** 16 * 4095, 2 ** 31) and b["pixel_blend"] == (255 * 65536 + 32768, 2 ** 32)
    assert all(worst < limit for worst, limit in b.values())
    both = S.overflow_bounds()
    assert {f"affine_{k}" for k in b} <= set(both) and all(worst < limit for worst, limit in both.values())
    # the restatement's own worst case: every coefficient at its cap, the largest patch, an origin at the int32 limit
    x, y = G.coordinates([[2 ** 31 - 1, 2 ** 31 - 1]], 4096, [[2 ** 16] * 4])
    assert int(np.abs(x).max()) <= b["source_coordinate"][0] and int(np.abs(y).max()) <= b["source_coordinate"][0]
