"""Host: the area resampling of DESIGN.md section 4.14 without a GPU -- the NumPy restatement (tests/helpers/resample_ref.py)
against exact rational arithmetic, the sizes, the refusals, the overflow bounds and the kernel's division rule."""
import random
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import resample_ref as R  # noqa: E402

from deephisto_amd import resample as RS  # noqa: E402

FACTORS = [Fraction(1), Fraction(2), Fraction(3), Fraction(7), Fraction(64), Fraction(3, 2), Fraction(4, 3), Fraction(7, 3),
           Fraction(255, 128), Fraction(625, 607), Fraction(2048, 2047)]


def image_for(f, seed=0):
    """A random image of sizes that are multiples of nothing, with at least one footprint (here two) in each axis."""
    h, w = max(37, int(2 * f) + 3), max(53, int(2 * f) + 5)
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def exact(a, f):
    """Round half up of the true mean over each output pixel's footprint, in Fractions: the overlap of [j, j+1) with
    [y f, (y+1) f) as a length, no common denominator."""
    f = Fraction(f)
    h, w = a.shape[:2]
    oh, ow = int(h / f), int(w / f)

    def overlaps(n_out, n_src):
        rows = []
        for y in range(n_out):
            lo, hi = y * f, (y + 1) * f
            rows.append([(j, min(Fraction(j + 1), hi) - max(Fraction(j), lo)) for j in range(int(lo), min(n_src, int(hi) + 1))
                         if min(Fraction(j + 1), hi) > max(Fraction(j), lo)])
        return rows

    oy, ox = overlaps(oh, h), overlaps(ow, w)
    out = np.empty((oh, ow, 3), np.uint8)
    mean = np.empty((oh, ow, 3), np.float64)
    for y in range(oh):
        for x in range(ow):
            for c in range(3):
                m = sum(ly * lx * int(a[j, i, c]) for j, ly in oy[y] for i, lx in ox[x]) / (f * f)
                out[y, x, c] = int(m + Fraction(1, 2))      # floor(m + 1/2): half up
                mean[y, x, c] = float(m)
    return out, mean


@pytest.mark.parametrize("f", FACTORS, ids=str)
def test_restatement_is_the_exact_mean_rounded_half_up(f):
    a = image_for(f)
    if f >= 7:   # keep the Fraction loops short: a few footprints are enough
        a = a[:int(2 * f) + 3, :int(2 * f) + 5]
    want, mean = exact(a, f)
    got = R.resample(a, f)
    assert got.shape == want.shape and got.shape[0] >= 1 and got.shape[1] >= 1
    np.testing.assert_array_equal(got, want)
    assert np.abs(got.astype(np.float64) - mean).max() <= 0.5 + 1e-9


@pytest.mark.parametrize("L", [1, 2, 3, 7, 64])
def test_integer_factor_is_the_block_sum(L):
    a = image_for(Fraction(L), seed=L)
    oh, ow = a.shape[0] // L, a.shape[1] // L
    s = a[:oh * L, :ow * L].astype(np.int64).reshape(oh, L, ow, L, 3).sum((1, 3))
    np.testing.assert_array_equal(R.resample(a, L), (2 * s + L * L) // (2 * L * L))


@pytest.mark.parametrize("f", FACTORS, ids=str)
def test_weights_sum_to_num_and_constants_stay(f):
    num, den = f.numerator, f.denominator
    n_src = 3 * num + 5
    wts = R.weights(n_src, (n_src * den) // num, num, den)
    assert wts.shape[0] >= 1 and (wts.sum(1) == num).all() and wts.min() >= 0
    for v in (0, 1, 127, 255):
        a = np.full((int(2 * f) + 3, int(2 * f) + 4, 3), v, np.uint8)
        assert (R.resample(a, f) == v).all()


def test_resampled_size_and_factor_forms():
    assert RS.resampled_size(37, 53, 2) == (18, 26)
    assert RS.resampled_size(37, 53, Fraction(3, 2)) == (24, 35)
    assert RS.resampled_size(37, 53, "3/2") == (24, 35) == RS.resampled_size(37, 53, "6/4")
    assert RS.resampled_size(37, 53, "7") == (5, 7)
    assert RS.resampled_size(1, 1, 2) == (0, 0)
    assert RS.resampled_size(50000, 50000, 64) == (781, 781)
    assert RS.parse_factor(Fraction(4096, 4094)) == (2048, 2047)
    assert RS.parse_factor(np.int64(4)) == (4, 1)
    for f in FACTORS:
        assert RS.resampled_size(37, 53, f) == R.size(37, 53, f)
        assert RS.strip_width(f.numerator, f.denominator) >= 21


@pytest.mark.parametrize("bad, exc, word", [
    (2.0, TypeError, "float"), (np.float32(2), TypeError, "float"), (True, TypeError, "bool"), (None, TypeError, "NoneType"),
    (Fraction(1, 2), ValueError, "below 1"), ("1/2", ValueError, "below 1"), (0, ValueError, "below 1"),
    ("2/0", ValueError, "zero denominator"), ("two", ValueError, "NUM/DEN"), ("3/2/1", ValueError, "NUM/DEN"), ("-2", ValueError, "NUM/DEN"),
    (65, ValueError, "at most 64"), (Fraction(2049, 2048), ValueError, "2048"), ("4099/4097", ValueError, "2048"),
])
def test_factor_refusals_by_name(bad, exc, word):
    with pytest.raises(exc, match=word):
        RS.parse_factor(bad)


def test_area_resample_refuses_host_tensors_by_name():
    import torch
    with pytest.raises(ValueError, match="GPU memory"):
        RS.area_resample(torch.zeros((8, 8, 3), dtype=torch.uint8), 2)
    with pytest.raises(TypeError, match="torch tensor"):
        RS.area_resample(np.zeros((8, 8, 3), np.uint8), 2)
    with pytest.raises(TypeError, match="float"):
        RS.area_resample(torch.zeros((8, 8, 3), dtype=torch.uint8), 2.0)


def test_pyramid_slide_host_protocol(tmp_path):
    """What needs no GPU: sizes, layer checks, layer-1 reads of a host base, the .npy route, the band heights."""
    a = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    np.save(tmp_path / "s.npy", a)
    from deephisto_amd.psimage_compat import ArraySlide, open_slide
    for base in (a, tmp_path / "s.npy", str(tmp_path / "s.npy")):
        with RS.PyramidSlide(base, device="cpu") as p:
            assert open_slide(p) is p
            assert (p.height, p.width) == (37, 53)
            assert p.layer_size(1) == (37, 53) and p.layer_size(2) == (18, 26) and p.layer_size(4) == (9, 13)
            np.testing.assert_array_equal(p.get_region_from_layer(1, (3, 5), (20, 41)), a[3:20, 5:41])
            np.testing.assert_array_equal(p.get_region((3, 5), (20, 41), (7, 9)), ArraySlide(a).get_region((3, 5), (20, 41), (7, 9)))
            for bad in (0, -1, 65, 2.0, True):
                with pytest.raises(ValueError, match="invalid layer"):
                    p.layer_size(bad)
    with pytest.raises(ValueError, match="layers of its own"):
        RS.PyramidSlide("slide.psi")
    with pytest.raises(ValueError, match=r"uint8\[h, w, 3\]"):
        RS.PyramidSlide(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="band_bytes"):
        RS.PyramidSlide(a, band_bytes=0)
    # bands: whole multiples of the layer, in groups of 16 layer rows when that many fit, never above band_bytes unless one
    # layer row's sources alone exceed it
    row = 3 * 53
    assert RS.PyramidSlide(a, device="cpu", band_bytes=row * 7).band_rows(2) == 6
    assert RS.PyramidSlide(a, device="cpu", band_bytes=row * 70).band_rows(2) == 64
    assert RS.PyramidSlide(a, device="cpu", band_bytes=1).band_rows(4) == 4


def test_overflow_bounds_with_python_ints():
    b = RS.overflow_bounds()
    assert b["rounded_numerator"][0] == 511 * 2048 ** 2
    d = RS.MAX_NUM ** 2
    assert b["weighted_sum"][0] == 255 * d and b["vertical_sum"][0] == 255 * RS.MAX_NUM
    for name, (worst, limit) in b.items():
        assert isinstance(worst, int) and isinstance(limit, int) and 0 < worst < limit, name
    # the largest reachable numerator really is reached by an all-white footprint at the largest factor
    assert 2 * (255 * d) + d == b["rounded_numerator"][0]
    assert (RS.MAX_SIDE * (RS.MAX_NUM - 1) + RS.MAX_NUM) == b["coordinate"][0]


def test_division_rule_every_num():
    """The kernel's multiply-high by (2^64 - 1) // (2 D) + 1, with its widths, equals Python's // at the edges of every num."""
    for num in range(1, RS.MAX_NUM + 1):
        D = num * num
        m = RS.div_magic(2 * D)
        assert 0 < m < 1 << 64
        for S in (0, 1, D - 1, D, 255 * D):
            n = 2 * S + D
            assert RS.div_by_magic(n, m) == n // (2 * D), (num, S)


def test_division_rule_random_sums():
    rng = random.Random(7)
    for num in (1, 2, 3, 7, 64, 255, 607, 625, 1023, 1024, 2047, 2048):
        D = num * num
        m = RS.div_magic(2 * D)
        for _ in range(10000):
            S = rng.randint(0, 255 * D)
            n = 2 * S + D
            assert RS.div_by_magic(n, m) == n // (2 * D), (num, S)


def test_division_by_den_rule():
    """The same multiply-high serves floor(n / den) for the footprint bounds: every reduced den >= 2, the largest coordinates."""
    top = RS.overflow_bounds()["coordinate"][0]
    rng = random.Random(11)
    for den in range(2, RS.MAX_NUM):
        m = RS.div_magic(den)
        for n in (0, 1, den - 1, den, den + 1, top - 1, top, rng.randint(0, top)):
            assert RS.div_by_magic(n, m) == n // den, (den, n)


def test_dataset_pyramid_is_refused_by_name_unless_bool():
    from deephisto_amd.models.patch_cls_simple import train
    assert train._pyramid_from_cfg({"dataset": {}}) is False and train._pyramid_from_cfg({}) is False
    assert train._pyramid_from_cfg({"dataset": {"pyramid": True}}) is True
    for bad in (1, 0, "true", "yes", None, 2.0):
        with pytest.raises(ValueError, match="dataset.pyramid must be true or false"):
            train._pyramid_from_cfg({"dataset": {"pyramid": bad}})


def test_cli_refuses_pyramid_with_ondisk_and_psimage_paths(capsys):
    from deephisto_amd.examples import predict_full_patched as P
    ap = P._build_parser()
    for argv, word in ((["--synthetic", "512", "512", "--pyramid", "--ondisk"], "--ondisk"),
                       (["--image", "slide.psi", "--pyramid"], "layers of its own")):
        with pytest.raises(SystemExit):
            P._check_args(ap, ap.parse_args(argv))
        assert word in capsys.readouterr().err
    args = ap.parse_args(["--synthetic", "512", "512", "--pyramid"])
    P._check_args(ap, args)
    assert args.pyramid
