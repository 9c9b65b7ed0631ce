"""Host math of the stain jitter: the augmenter's private stream, the fixed-point parameter rows, the
overflow bound, the NumPy restatement against plain float64, and the refusals.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import stain_aug_ref as A  # noqa: E402
import stain_ref as R  # noqa: E402

from deephisto_amd import stain as S  # noqa: E402

HE = np.array(S.TARGET_HE, dtype=np.float64)
IDENTITY_ROW = [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]


def test_identity_parameters_are_exact_and_keep_every_byte():
    p = S.jitter_params(HE, np.ones((3, 2)), np.zeros((3, 2)))
    assert p.dtype == np.int32 and p.tolist() == [IDENTITY_ROW] * 3
    assert S.jitter_params(R.HE_TRUE, np.ones((1, 2)), np.zeros((1, 2))).tolist() == [IDENTITY_ROW]
    assert S.jitter_params(HE, np.ones((0, 2)), np.zeros((0, 2))).shape == (0, 12)
    # lut[T[v]] == v for every byte, so identity parameters give the plain gather's bits
    ramp = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)[:, :, ::-1].copy()
    ramp[..., 1] = np.arange(256, dtype=np.uint8).reshape(16, 16).T
    for fh, fv in ((False, False), (True, False), (False, True), (True, True)):
        got = A.gather(ramp, [[0, 0], [-3, 9]], 16, p[:2], fh, fv)
        assert np.array_equal(got.view(np.uint32), A.plain(ramp, [[0, 0], [-3, 9]], 16, fh, fv).view(np.uint32))
    assert np.array_equal(np.rint(A.gather(ramp, [[0, 0]], 16, p[:1])[0] * 255).astype(np.uint8), ramp)


def test_parameter_rows_are_the_stated_formulas():
    alpha, beta = np.array([[1.3, 0.8], [0.5, 1.5]]), np.array([[0.05, -0.02], [-0.1, 0.1]])
    p = S.jitter_params(HE, alpha, beta)
    for k in range(2):
        a = np.eye(3) + HE @ np.diag(alpha[k] - 1.0) @ S.pinv32(HE)
        assert np.abs(p[k, :9].reshape(3, 3) - a * 4096).max() <= 0.5 + 1e-9
        assert np.abs(p[k, 9:] - (HE @ beta[k]) * 2.0 ** 24).max() <= 0.5 + 1e-6
    # OD' = OD + HE ((alpha - 1) * c + beta): a pixel of pure haematoxylin, concentration 1, moves along HE[:, 0] only
    od = HE[:, 0]
    a0, b0 = p[0, :9].reshape(3, 3) / 4096.0, p[0, 9:] / 2.0 ** 24
    assert np.allclose(a0 @ od + b0, od + HE @ ((alpha[0] - 1.0) * np.array([1.0, 0.0]) + beta[0]), atol=2e-3)


def test_draw_is_reproducible_and_private():
    np.random.seed(7)
    torch.manual_seed(7)
    np_state, torch_state = np.random.get_state(), torch.get_rng_state()
    a, b = S.StainAugmenter(0.2, 0.05, seed=3), S.StainAugmenter(0.2, 0.05, seed=3)
    al, be = a.draw(64)
    assert al.dtype == be.dtype == np.float64 and al.shape == be.shape == (64, 2)
    al2, be2 = b.draw(64)
    assert np.array_equal(al, al2) and np.array_equal(be, be2)
    assert not np.array_equal(al, a.draw(64)[0])                      # the stream moves on
    assert not np.array_equal(al, S.StainAugmenter(0.2, 0.05, seed=4).draw(64)[0])
    assert (np.abs(al - 1.0) <= 0.2).all() and np.abs(al - 1.0).max() > 0.15 and (np.abs(be) <= 0.05).all() and np.abs(be).max() > 0.03
    # one uniform(size=(n, 4)) call of PCG64(seed), columns (alpha H, alpha E, beta H, beta E)
    u = 2.0 * np.random.Generator(np.random.PCG64(3)).uniform(size=(64, 4)) - 1.0
    assert np.array_equal(al, 1.0 + 0.2 * u[:, :2]) and np.array_equal(be, 0.05 * u[:, 2:])
    zero = S.StainAugmenter(0.0, 0.0).draw(5)
    assert np.array_equal(zero[0], np.ones((5, 2))) and np.array_equal(zero[1], np.zeros((5, 2)))
    s = np.random.get_state()
    assert s[0] == np_state[0] and np.array_equal(s[1], np_state[1]) and s[2:] == np_state[2:]
    assert torch.equal(torch.get_rng_state(), torch_state)


def test_record_stream_does_not_depend_on_the_augmenter():
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionRndSampler
    imgs = [R.synth_he(300, 340, 1), R.synth_he(260, 280, 2)]
    annos = [[{"class": "TUM", "vertices": [[20, 20], [320, 30], [300, 280], [30, 260]]}],
             [{"class": "BG", "vertices": [[10, 10], [270, 20], [260, 250], [15, 240]]}]]
    streams = []
    for aug in (None, S.StainAugmenter(0.0, 0.0), S.StainAugmenter(0.2, 0.05, seed=1)):
        smp = AnnoRegionRndSampler(list(zip(imgs, annos)), layer=1, patch_size=32, device="cpu", stain_aug=aug)
        assert smp.stain_aug is aug
        np.random.seed(11)
        streams.append(smp._records(24))
    assert streams[0] == streams[1] == streams[2] and len(streams[0]) == 24


def test_fixed_point_is_within_one_grey_level_of_float64():
    """The restatement against 256 exp(-(A OD + b)) - 1 in float64, rounded and clamped: at most 1 grey level, the bound the
    normaliser documents (the same tables are the error sources).  Measured: worst difference 1."""
    img = R.synth_he(96, 128, 3)
    rng = np.random.default_rng(0)
    alpha, beta = rng.uniform(0.5, 1.5, (200, 2)), rng.uniform(-0.1, 0.1, (200, 2))
    params = S.jitter_params(HE, alpha, beta)
    px = np.broadcast_to(img, (1,) + img.shape)
    worst = 0
    for k in range(200):
        fixed = S.output_lut()[np.clip(A.raw_index(px, params[k:k + 1]), 0, S.LUT_SIZE - 1)][0]
        want = A.jitter_float64(img, HE, alpha[k], beta[k])
        worst = max(worst, int(np.abs(fixed.astype(np.int64) - want.astype(np.int64)).max()))
    print("worst difference, grey levels:", worst)
    assert worst <= 1


def test_refusals_name_the_argument():
    with pytest.raises(ValueError, match="sigma_alpha"):
        S.StainAugmenter(sigma_alpha=0.95)
    with pytest.raises(ValueError, match="sigma_alpha"):
        S.StainAugmenter(sigma_alpha=-0.1)
    with pytest.raises(ValueError, match="sigma_beta"):
        S.StainAugmenter(sigma_beta=0.6)
    with pytest.raises(ValueError, match="sigma_beta"):
        S.StainAugmenter(sigma_beta=float("nan"))
    with pytest.raises(ValueError, match="seed"):
        S.StainAugmenter(seed=-1)
    S.StainAugmenter(0.9, 0.5)                                           # the ends of both ranges are accepted
    with pytest.raises(ValueError, match="bias"):                        # |HE beta| 2^24 beyond 2^30
        S.jitter_params(HE, np.ones((1, 2)), np.array([[100.0, 0.0]]))
    near = np.array([[0.6, 0.6 + 1e-4], [0.7, 0.7], [0.38, 0.38]])        # near-parallel basis: the pseudo-inverse explodes
    with pytest.raises(ValueError, match="jitter matrix"):
        S.jitter_params(near, np.array([[1.5, 1.0]]), np.zeros((1, 2)))
    with pytest.raises(ValueError, match="alpha and beta"):
        S.jitter_params(HE, np.ones((2, 2)), np.zeros((3, 2)))


def test_malformed_config_entry_is_refused_by_key():
    from deephisto_amd.models.patch_cls_simple.train import _stain_aug_from_cfg
    assert _stain_aug_from_cfg({"dataset": {}}) is None and _stain_aug_from_cfg({}) is None
    aug = _stain_aug_from_cfg({"dataset": {"stain_augment": {"sigma_alpha": 0.3, "sigma_beta": 0.01, "seed": 5}}}, rank=2)
    assert (aug.sigma_alpha, aug.sigma_beta, aug.seed) == (0.3, 0.01, 7)   # data parallel: seed + rank
    dflt = _stain_aug_from_cfg({"dataset": {"stain_augment": {}}})
    assert (dflt.sigma_alpha, dflt.sigma_beta, dflt.seed) == (0.2, 0.0, 0)
    for entry, name in (({"sigma": 0.2}, "sigma"), ({"sigma_alpha": 0.95}, "sigma_alpha"), ({"sigma_beta": "big"}, "sigma_beta"),
                        ({"seed": 1.5}, "seed"), ("on", "must be a mapping"), ([0.2, 0.0], "must be a mapping")):
        with pytest.raises(ValueError, match=rf"dataset\.stain_augment.*{name}"):
            _stain_aug_from_cfg({"dataset": {"stain_augment": entry}})


def test_jittered_accumulator_stays_below_its_limit():
    worst, limit = S.overflow_bounds()["jittered_od"]
    assert worst == 3 * S.COEF_MAX * S.OD_MAX + 2 ** 30 and limit == 2 ** 63 and worst < limit
    # the restatement's own worst case: every matrix entry and the bias at their caps, all-black pixels
    row = np.array([[S.COEF_MAX] * 9 + [S.BIAS_MAX] * 3], np.int64)
    assert int(A.raw_index(np.zeros((1, 1, 1, 3), np.uint8), row).max()) << S.APPLY_SHIFT <= worst
