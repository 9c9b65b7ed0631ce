"""Tissue filter, host side: the exact Otsu rule, min_pixels, TissueFilter validation, the CLI's
refusals and the C entry points' argument checks (which return before any device call).  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest


def _otsu_float64(hist):
    """Brute-force restatement: between-class variance w0*w1*(mu0-mu1)^2 in float64 for every t with both classes non-empty."""
    h = np.asarray(hist, dtype=np.float64)
    c = np.arange(256, dtype=np.float64)
    N = h.sum()
    best, best_t = -1.0, 0
    for t in range(255):
        n0 = h[:t + 1].sum()
        n1 = N - n0
        if n0 == 0 or n1 == 0:
            continue
        mu0 = (h[:t + 1] * c[:t + 1]).sum() / n0
        mu1 = (h[t + 1:] * c[t + 1:]).sum() / n1
        v = (n0 / N) * (n1 / N) * (mu0 - mu1) ** 2
        if v > best:
            best, best_t = v, t
    return best_t


@pytest.mark.parametrize("seed", range(8))
def test_otsu_matches_float64_restatement(seed):
    from deephisto_amd.tissue import otsu_threshold
    rng = np.random.default_rng(seed)
    # glass near chroma 0..10, stain well above: two separated modes of seeded sizes and widths
    lo_c, hi_c = rng.integers(2, 12), rng.integers(60, 200)
    x = np.concatenate([rng.normal(lo_c, rng.uniform(1, 4), rng.integers(10_000, 1_000_000)),
                        rng.normal(hi_c, rng.uniform(5, 30), rng.integers(10_000, 1_000_000))])
    hist = np.bincount(np.clip(np.rint(x), 0, 255).astype(np.int64), minlength=256).astype(np.uint64)
    t = otsu_threshold(hist)
    assert t == _otsu_float64(hist)
    assert lo_c < t < hi_c


def test_otsu_exact_on_huge_counts():
    """Counts of a 50 000^2 slide: the integer rule does not overflow or round (Python ints)."""
    from deephisto_amd.tissue import otsu_threshold
    hist = np.zeros(256, np.uint64)
    hist[0], hist[1], hist[120], hist[130] = 1_250_000_000, 3, 600_000_000, 650_000_000
    assert otsu_threshold(hist) == _otsu_float64(hist) == 1


def test_otsu_tie_rule_and_degenerate_histograms():
    from deephisto_amd.tissue import otsu_threshold
    h = np.zeros(256, np.uint64)
    h[0] = h[2] = h[4] = 1           # t = 0 and t = 2 (and 1, 3) give the same value: the smallest wins
    assert otsu_threshold(h) == 0
    h = np.zeros(256, np.uint64)
    h[10] = h[20] = 5                # every t in 10..19 splits the same way
    assert otsu_threshold(h) == 10
    assert otsu_threshold(np.zeros(256, np.uint64)) == 0
    for b in (0, 7, 255):            # a single non-empty bin
        h = np.zeros(256, np.uint64)
        h[b] = 123
        assert otsu_threshold(h) == 0
    h = np.zeros(256, np.uint64)
    h[254], h[255] = 1, 1            # the last possible split
    assert otsu_threshold(h) == 254
    with pytest.raises(ValueError):
        otsu_threshold(np.zeros(255, np.uint64))


def test_min_pixels_rounding():
    from deephisto_amd.tissue import TissueFilter, min_pixels
    assert min_pixels(0.25, 224) == 12544
    assert min_pixels(0.0, 224) == 0 and min_pixels(1.0, 224) == 224 * 224
    assert min_pixels(0.5, 3) == 5                 # 4.5 rounds up
    assert min_pixels(0.1, 3) == math.ceil(0.1 * 9) == 1
    assert min_pixels(0.07, 100) == 701        # 0.07 * 100 * 100 = 700.0000000000001 in float64: the rule is the float product
    assert min_pixels(1e-9, 256) == 1              # any positive fraction needs at least one pixel
    assert TissueFilter(min_fraction=0.25).min_pixels(256) == 16384


@pytest.mark.parametrize("kw", [dict(threshold="OTSU"), dict(threshold="50"), dict(threshold=256), dict(threshold=-1),
                                dict(threshold=1.5), dict(threshold=True), dict(threshold=None),
                                dict(min_fraction=-0.1), dict(min_fraction=1.01), dict(min_fraction=float("nan")),
                                dict(min_fraction="0.3"), dict(min_fraction=True),
                                dict(fill_class=-2), dict(fill_class=1.0), dict(fill_class="BG")])
def test_tissue_filter_refuses_bad_fields(kw):
    from deephisto_amd.tissue import TissueFilter
    with pytest.raises(ValueError):
        TissueFilter(**kw)


def test_tissue_filter_defaults_and_fields():
    from deephisto_amd.tissue import TissueFilter
    f = TissueFilter()
    assert (f.threshold, f.min_fraction, f.fill_class) == ("otsu", 0.25, -1)
    f = TissueFilter(np.int64(0), 1, 4)
    assert (f.threshold, f.min_fraction, f.fill_class) == (0, 1.0, 4) and type(f.threshold) is int


@pytest.mark.parametrize("extra,msg", [(["--tissue", "otsu", "--random_sampler"], "--random_sampler"),
                                       (["--tissue", "40", "--ondisk"], "--ondisk"),
                                       (["--tissue", "300"], "threshold"),
                                       (["--tissue", "glass"], "threshold"),
                                       (["--tissue", "otsu", "--tissue_min_fraction", "1.5"], "min_fraction"),
                                       (["--tissue", "otsu", "--tissue_fill", "XX"], "--tissue_fill")])
def test_cli_refuses_bad_tissue_flags(extra, msg, capsys):
    """Refused by argparse before the process group or any GPU is touched."""
    from deephisto_amd.examples.predict_full_patched import main
    with pytest.raises(SystemExit) as e:
        main(["--synthetic", "512", "512", "--weights", "", *extra])
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_cli_tissue_flags_parse():
    import argparse

    from deephisto_amd.examples.predict_full_patched import _tissue_from_args
    ap = argparse.ArgumentParser()

    def ns(**kw):
        base = dict(tissue="off", random_sampler=False, ondisk=False, tissue_min_fraction=0.25, tissue_fill="-1")
        return argparse.Namespace(**{**base, **kw})

    assert _tissue_from_args(ap, ns()) is None
    f = _tissue_from_args(ap, ns(tissue="otsu", tissue_fill="BG", tissue_min_fraction=0.5))
    assert (f.threshold, f.min_fraction, f.fill_class) == ("otsu", 0.5, 1)
    f = _tissue_from_args(ap, ns(tissue="12"))
    assert (f.threshold, f.fill_class) == (12, -1)


def test_c_entries_refuse_bad_arguments(built_lib):
    """Argument checks of the C ABI; every case fails before a device call, so fake (aligned) addresses are safe here."""
    lib = built_lib
    fake = C.c_void_p(1 << 20)
    yx = np.array([[0, 0], [10, 580]], np.int32)
    k = C.c_int64()

    def counts(h=100, w=100, P=32, t=20, host=None, words=10_000, slide=fake):
        return lib.dh_tissue_tile_counts(slide, h, w, fake, host, 2 if host is not None else 0, P, t, fake, words, fake, None)

    assert lib.dh_tissue_histogram(None, 10, 10, fake, None) == -22 and b"null" in lib.dh_last_error()
    assert lib.dh_tissue_histogram(C.c_void_p((1 << 20) + 3), 10, 10, fake, None) == -22 and b"aligned" in lib.dh_last_error()
    assert lib.dh_tissue_histogram(fake, 0, 10, fake, None) == -22
    assert counts(slide=None) == -22 and b"null" in lib.dh_last_error()
    assert counts(t=256) == -22 and b"threshold 256" in lib.dh_last_error()
    assert counts(t=-1) == -22 and b"threshold" in lib.dh_last_error()
    assert counts(P=101) == -22 and b"larger than" in lib.dh_last_error()
    assert counts(h=50, w=200, P=60) == -22 and b"larger than" in lib.dh_last_error()
    assert counts(words=156) == -22 and b"157 needed" in lib.dh_last_error()
    assert counts(h=600, w=600, host=yx.ctypes.data_as(C.c_void_p)) == -22
    assert b"origin 1 (10, 580) outside" in lib.dh_last_error()
    assert lib.dh_tissue_select(fake, fake, 4, -1, fake, fake, fake, C.byref(k), None) == -22
    assert b"min_pixels" in lib.dh_last_error()
    assert lib.dh_tissue_select(fake, fake, 4, 5, None, fake, fake, C.byref(k), None) == -22 and b"null" in lib.dh_last_error()
    assert lib.dh_fill_uncovered(fake, 3, 0, 16, 100, 100, -1, fake, fake, None) == -22
    assert lib.dh_fill_uncovered(fake, 3, 32, 16, 100, 100, -1, None, fake, None) == -22 and b"null" in lib.dh_last_error()
