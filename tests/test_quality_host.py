"""Tile quality filter, host side: the NumPy restatement against an independent float64 formulation,
csrc/quality_rule.h in a stand-alone program under AddressSanitizer + UBSan against the restatement, QualityFilter
validation, max_ink_pixels, the fill-class conflict, the CLI's refusals and the C entry points' argument checks.  CPU only."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import quality_ref as Q  # noqa: E402

REPO = Path(__file__).resolve().parents[1]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_float64_variance(seed):
    """np.var of the masked Laplacian (float64, an independent formulation with explicit neighbour loops) times n_t^2 equals
    n_t*S2 - S1^2 in Python ints."""
    rng = np.random.default_rng(seed)
    h, w, P = int(rng.integers(9, 30)), int(rng.integers(9, 30)), int(rng.integers(3, 9))
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    t = int(rng.integers(-1, 200))
    origins = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0), (int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1)))]
    stats = Q.tile_stats(img, origins, P, t)
    yl = (77 * img[..., 0].astype(float) + 150 * img[..., 1].astype(float) + 29 * img[..., 2].astype(float) + 128) // 256
    for (y0, x0), (n_t, s1, s2, n_ink) in zip(origins, stats.tolist()):
        vals, ink = [], 0
        for y in range(y0, y0 + P):
            for x in range(x0, x0 + P):
                r, g, b = (int(v) for v in img[y, x])
                ink += (max(r, g, b) - min(r, g, b) > 40 and g - min(r, b) >= 16) or max(r, g, b) <= 40
                if max(r, g, b) - min(r, g, b) > t:
                    nb = [yl[max(y - 1, 0), x], yl[min(y + 1, h - 1), x], yl[y, max(x - 1, 0)], yl[y, min(x + 1, w - 1)]]
                    vals.append(4 * yl[y, x] - sum(nb))
        assert n_t == len(vals) and n_ink == ink
        if n_t:
            assert s1 == int(sum(vals))
            # var * n^2 is an integer below 2^53 here (n <= 64, |L| <= 1020), so float64 holds it to a relative 1e-12
            assert n_t * s2 - s1 * s1 == pytest.approx(float(np.var(np.array(vals))) * n_t * n_t, rel=1e-9, abs=1e-6)


def test_painted_slide_separates():
    """What the GPU tests rely on: sharp tiles far above, blurred tiles far below min_sharpness = 200; flat tiles have
    sharpness 0 and are all ink; pink noise has no ink pixel."""
    img, areas = Q.painted(300, 300, 0)
    P = 64
    o = np.array([[8, 8], [8, 200], [200, 8], [200, 200]], np.int32)
    for k, name in enumerate(("sharp", "blur", "blue", "black")):
        assert Q.inside(o[k:k + 1], P, areas[name], 300, 300)[0]
    s = Q.tile_stats(img, o, P, -1)
    sharp = [(n * s2 - s1 * s1) / (n * n) for n, s1, s2, _ in s.tolist()]
    assert sharp[0] > 1000 and sharp[1] < 50 and sharp[2] == 0 and sharp[3] == 0
    assert s[:, 3].tolist() == [0, 0, P * P, P * P]
    r, keep = Q.flags(s, 200, Q.max_ink_pixels(0.1, P))
    assert r.tolist() == [0, Q.BLUR, Q.BLUR | Q.INK, Q.BLUR | Q.INK] and keep.tolist() == [1, 0, 0, 0]
    r, _ = Q.flags(s, 0, Q.max_ink_pixels(0.1, P))
    assert r.tolist() == [0, 0, Q.INK, Q.INK]


# ---- quality_rule.h under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("quality") / "quality_rule_check"
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(REPO / "tests" / "helpers" / "quality_rule_check.cc"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def _run_check(exe, step, t, ink_chroma, ink_margin, dark_max, cases=()):
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    r = subprocess.run([str(exe), str(step), str(t), str(ink_chroma), str(ink_margin), str(dark_max)], input=text,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    px = np.array([ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("P ")], np.int64)
    tiles = [[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("T ")]
    return px, tiles


@pytest.mark.parametrize("t,ink_chroma,ink_margin,dark_max", [(37, 40, 16, 40), (-1, 0, 0, -1), (255, 255, 255, 255), (0, 100, 1, 0)])
def test_pixel_rule_of_the_header_equals_restatement(rule_check, t, ink_chroma, ink_margin, dark_max):
    px, _ = _run_check(rule_check, 5, t, ink_chroma, ink_margin, dark_max)
    assert len(px) == 52 ** 3            # 0, 5, ..., 250 and 255 on each axis
    rgb = px[:, :3].astype(np.uint8)
    for corner in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255)):
        assert (rgb == corner).all(axis=1).any()
    np.testing.assert_array_equal(px[:, 3], Q.luma(rgb))
    assert px[:, 3].min() == 0 and px[:, 3].max() == 255
    np.testing.assert_array_equal(px[:, 4], Q.chroma(rgb))
    np.testing.assert_array_equal(px[:, 5], Q.tissue_mask(rgb, t))
    np.testing.assert_array_equal(px[:, 6], Q.ink_mask(rgb, ink_chroma, ink_margin, dark_max))


def test_tile_decision_of_the_header_at_the_bounds(rule_check):
    cases = Q.boundary_cases()
    _, tiles = _run_check(rule_check, 255, 0, 40, 16, 40, cases)
    assert len(tiles) == len(cases)
    seen = set()
    for c, got in zip(cases, tiles):
        assert tuple(got[:6]) == c
        assert got[6] == Q.reason(*c), c
        seen.add(got[6])
    assert seen == {0, Q.BLUR, Q.INK, Q.BLUR | Q.INK}
    n, m = 2 ** 20, 1020 * 1020
    assert Q.reason(n, 0, n * m, 0, m, 0) == 0 and Q.reason(n, 0, n * m - 1, 0, m, 0) == Q.BLUR     # equality keeps the tile
    assert Q.reason(n, 1020 * n, n * m, 0, 1, 0) == Q.BLUR and Q.reason(n, 1020 * n, n * m, 0, 0, 0) == 0
    assert Q.reason(0, 0, 0, 0, 0, 0) == 0 and Q.reason(0, 0, 0, 0, 1, 0) == Q.BLUR
    assert n * n * m < 2 ** 63           # the bound the header's comment states


# ---- QualityFilter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(min_sharpness=-1), dict(min_sharpness=1040401), dict(min_sharpness=1.5), dict(min_sharpness=True),
                                dict(min_sharpness="200"), dict(min_sharpness=None), dict(min_sharpness=float("nan")),
                                dict(max_ink_fraction=-0.1), dict(max_ink_fraction=1.01), dict(max_ink_fraction=float("nan")),
                                dict(max_ink_fraction="0.3"), dict(max_ink_fraction=True),
                                dict(ink_chroma=-1), dict(ink_chroma=256), dict(ink_chroma=True), dict(ink_chroma=4.0),
                                dict(ink_margin=-1), dict(ink_margin=256), dict(ink_margin=False),
                                dict(dark_max=-2), dict(dark_max=256), dict(dark_max=True), dict(dark_max=float("nan")),
                                dict(fill_class=-2), dict(fill_class=1.0), dict(fill_class="BG"), dict(fill_class=True)])
def test_quality_filter_refuses_bad_fields(kw):
    from deephisto_amd.quality import QualityFilter
    with pytest.raises(ValueError, match=next(iter(kw))):
        QualityFilter(**kw)


def test_quality_filter_defaults_fields_and_repr():
    from deephisto_amd.quality import QualityFilter
    f = QualityFilter()
    assert (f.min_sharpness, f.max_ink_fraction, f.ink_chroma, f.ink_margin, f.dark_max, f.fill_class) == (0, 1.0, 40, 16, 40, -1)
    assert f.max_ink_pixels(224) == 224 * 224            # the defaults keep every tile: no tile has more ink pixels than pixels
    f = QualityFilter(np.int64(200), 0, np.int32(10), 3, -1, 4)
    assert (f.min_sharpness, f.max_ink_fraction, f.ink_chroma, f.ink_margin, f.dark_max, f.fill_class) == (200, 0.0, 10, 3, -1, 4)
    assert type(f.min_sharpness) is int and type(f.max_ink_fraction) is float
    assert repr(f) == ("QualityFilter(min_sharpness=200, max_ink_fraction=0.0, ink_chroma=10, ink_margin=3, dark_max=-1, "
                       "fill_class=4)")
    assert QualityFilter(1040400).min_sharpness == 1040400


def test_max_ink_pixels_rounding():
    from deephisto_amd.quality import QualityFilter, max_ink_pixels
    assert max_ink_pixels(0.1, 224) == 5017              # 5017.6 rounds down
    assert max_ink_pixels(0.0, 224) == 0 and max_ink_pixels(1.0, 1024) == 2 ** 20
    assert max_ink_pixels(0.5, 3) == 4                   # 4.5 rounds down
    assert max_ink_pixels(0.07, 100) == 700              # 700.0000000000001 in float64: the rule is the float product, floored
    assert QualityFilter(max_ink_fraction=0.25).max_ink_pixels(256) == 16384
    for f, P in ((0.1, 64), (0.33, 31), (1.0, 17)):
        assert max_ink_pixels(f, P) == Q.max_ink_pixels(f, P)


def test_sharpness_is_nan_without_tissue():
    from deephisto_amd.quality import sharpness, sharpness_summary
    stats = np.array([[4, 2, 21, 0], [0, 0, 0, 7], [2 ** 20, 0, 2 ** 20 * 1020 * 1020, 0]], np.int64)
    s = sharpness(stats)
    assert s.dtype == np.float64 and s[0] == 5.0 and np.isnan(s[1]) and s[2] == 1040400.0
    q = sharpness_summary(stats)
    assert (q["n"], q["min"], q["max"]) == (2, 5.0, 1040400.0)
    assert sharpness_summary(stats[1:2])["n"] == 0


def test_fill_class_conflict():
    from deephisto_amd.quality import QualityFilter, check_fill_classes
    from deephisto_amd.tissue import TissueFilter
    check_fill_classes(None, QualityFilter(fill_class=3))
    check_fill_classes(TissueFilter(fill_class=3), None)
    check_fill_classes(TissueFilter(fill_class=3), QualityFilter(fill_class=3))
    with pytest.raises(ValueError, match="fill_class"):
        check_fill_classes(TissueFilter(fill_class=3), QualityFilter())


# ---- CLI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [(["--min_sharpness", "200", "--random_sampler"], "--random_sampler"),
                                       (["--max_ink", "0.1", "--ondisk"], "--ondisk"),
                                       (["--quality_fill", "BG", "--random_sampler"], "--random_sampler"),
                                       (["--min_sharpness", "-3"], "min_sharpness"),
                                       (["--min_sharpness", "2000000"], "min_sharpness"),
                                       (["--max_ink", "1.5"], "max_ink_fraction"),
                                       (["--max_ink", "0.1", "--quality_fill", "XX"], "--quality_fill"),
                                       (["--quality_json", "q.json"], "--quality_json needs"),
                                       (["--min_sharpness", "200", "--patch_size", "2048"], "--patch_size"),
                                       (["--tissue", "otsu", "--tissue_fill", "BG", "--min_sharpness", "200"], "same class")])
def test_cli_refuses_bad_quality_flags(extra, msg, capsys):
    """Refused by argparse before the process group or any GPU is touched."""
    from deephisto_amd.examples.predict_full_patched import main
    with pytest.raises(SystemExit) as e:
        main(["--synthetic", "512", "512", "--weights", "", *extra])
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_cli_quality_flags_parse():
    from deephisto_amd.examples import predict_full_patched as P
    ap = P._build_parser()
    base = ["--synthetic", "512", "512", "--weights", ""]

    def filt(*extra):
        args = ap.parse_args(base + list(extra))
        P._check_args(ap, args)
        return args.quality_filter

    assert filt() is None
    f = filt("--min_sharpness", "200")
    assert (f.min_sharpness, f.max_ink_fraction, f.fill_class) == (200, 1.0, -1)
    f = filt("--max_ink", "0.1", "--quality_fill", "BG")
    assert (f.min_sharpness, f.max_ink_fraction, f.fill_class) == (0, 0.1, 1)
    f = filt("--quality_fill", "-1")
    assert (f.min_sharpness, f.max_ink_fraction, f.fill_class) == (0, 1.0, -1)
    f = filt("--tissue", "otsu", "--tissue_fill", "BG", "--quality_fill", "BG", "--min_sharpness", "7")
    assert f.fill_class == 1 and f.min_sharpness == 7


# ---- C entry points -------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments(built_lib):
    """Argument checks of the C ABI; every case fails before a device call, so fake addresses are safe here."""
    lib = built_lib
    fake = C.c_void_p(1 << 20)
    yx = np.array([[0, 0], [10, 580]], np.int32)

    def stats(h=100, w=100, P=32, t=20, ic=40, im=16, dm=40, host=None, slide=fake, out=fake):
        return lib.dh_quality_tile_stats(slide, h, w, fake, host, 2, P, t, ic, im, dm, out, None)

    assert stats(slide=None) == -22 and b"null" in lib.dh_last_error()
    assert stats(out=None) == -22 and b"null" in lib.dh_last_error()
    assert stats(h=0) == -22 and b"bad sizes" in lib.dh_last_error()
    assert stats(t=256) == -22 and b"threshold 256" in lib.dh_last_error()
    assert stats(t=-2) == -22 and b"threshold -2" in lib.dh_last_error()
    assert stats(P=101) == -22 and b"patch 101 larger than the 100 x 100 slide" in lib.dh_last_error()
    assert stats(h=50, w=200, P=60) == -22 and b"larger than" in lib.dh_last_error()
    assert stats(h=2000, w=2000, P=1025) == -22 and b"patch 1025 above 1024" in lib.dh_last_error()
    assert stats(ic=256) == -22 and b"ink_chroma 256" in lib.dh_last_error()
    assert stats(im=-1) == -22 and b"ink_margin -1" in lib.dh_last_error()
    assert stats(dm=-2) == -22 and b"dark_max -2" in lib.dh_last_error()
    assert stats(h=600, w=600, host=yx.ctypes.data_as(C.c_void_p)) == -22
    assert b"origin 1 (10, 580) outside the 600 x 600 slide at patch 32" in lib.dh_last_error()
    assert lib.dh_quality_flags(None, 3, 0, 0, fake, fake, None) == -22 and b"null" in lib.dh_last_error()
    assert lib.dh_quality_flags(fake, 3, 0, 0, fake, None, None) == -22 and b"null" in lib.dh_last_error()
    assert lib.dh_quality_flags(fake, -1, 0, 0, fake, fake, None) == -22 and b"tile count" in lib.dh_last_error()
    assert lib.dh_quality_flags(fake, 3, -1, 0, fake, fake, None) == -22 and b"min_sharpness -1" in lib.dh_last_error()
    assert lib.dh_quality_flags(fake, 3, 1040401, 0, fake, fake, None) == -22 and b"min_sharpness 1040401" in lib.dh_last_error()
    assert lib.dh_quality_flags(fake, 3, 0, -1, fake, fake, None) == -22 and b"max_ink_pixels -1" in lib.dh_last_error()
    assert lib.dh_quality_flags(None, 0, 0, 0, None, None, None) == 0
