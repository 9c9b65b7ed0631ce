"""GPU: pyramid layers by exact area resampling against the NumPy restatement in
tests/helpers/resample_ref.py.  Every output byte is an integer function of the source bytes and is compared bit for bit; through
`PyramidSlide` the samplers, the prediction and the CLI give exactly what they give over the resampled slide."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FACTORS = [Fraction(1), Fraction(2), Fraction(3), Fraction(7), Fraction(64), Fraction(3, 2), Fraction(4, 3), Fraction(7, 3),
           Fraction(255, 128), Fraction(625, 607), Fraction(2048, 2047)]
SHAPES = [(37, 53), (64, 64), (130, 4099), (515, 1030)]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rand(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def check(host, f, dev):
    from deephisto_amd.resample import area_resample, resampled_size
    src = torch.from_numpy(host).to(dev)
    got = area_resample(src, f)
    want = R.resample(host, f)
    assert tuple(got.shape) == want.shape == (*resampled_size(*host.shape[:2], f), 3) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want)), f"{host.shape[:2]} at {f}"
    assert torch.equal(src.cpu(), torch.from_numpy(host))


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_factor_equals_the_restatement(dev, h, w):
    from deephisto_amd.resample import area_resample
    host = rand(h, w, h)
    for f in FACTORS:
        if h < f or w < f:
            with pytest.raises(ValueError, match="smaller than the factor"):
                area_resample(torch.from_numpy(host).to(dev), f)
        else:
            check(host, f, dev)


def test_row_pitches_take_several_phases():
    """3 w mod 16 over the shapes: source rows start at several byte phases, not only at 16-byte multiples."""
    assert len({3 * w % 16 for _, w in SHAPES}) >= 4 and any(w % 2 for _, w in SHAPES)


@pytest.mark.parametrize("f", [Fraction(2), Fraction(3, 2), Fraction(64), Fraction(2048, 2047)], ids=str)
def test_widths_around_the_tiling_constants(dev, f):
    """Output widths one below, at and one above the strip width (resample.strip_width: the columns of one workgroup), twice the
    strip, and around the 16-byte store group (3 ow = 15, 18, 45, 48, 51 bytes); source widths with and without a ragged
    remainder."""
    from deephisto_amd.resample import STORE_GROUP, strip_width
    strip = strip_width(f.numerator, f.denominator)
    assert STORE_GROUP == 16
    for ow in (5, 6, 15, 16, 17, strip - 1, strip, strip + 1, 2 * strip, 2 * strip + 1):
        w = -((-ow * f.numerator) // f.denominator)        # the narrowest source with ow whole output pixels
        h = int(2 * f) + 1
        check(rand(h, w, ow), f, dev)
        if R.size(h, w + 1, f)[1] == ow:
            check(rand(h, w + 1, ow + 1), f, dev)           # one more source column, dropped


@pytest.mark.parametrize("f", [Fraction(2), Fraction(3, 2), Fraction(7, 3)], ids=str)
def test_heights_around_the_band(dev, f):
    """Output heights one below, at and one above BAND_H (the output rows of one workgroup), and two bands and a row."""
    from deephisto_amd.resample import BAND_H
    assert BAND_H == 16
    for oh in (1, BAND_H - 1, BAND_H, BAND_H + 1, 2 * BAND_H + 1):
        h = -((-oh * f.numerator) // f.denominator)
        check(rand(h, 61, oh), f, dev)
        if R.size(h + 1, 61, f)[0] == oh:
            check(rand(h + 1, 61, oh + 1), f, dev)


def test_smallest_slides_and_refusals(dev):
    from deephisto_amd.resample import area_resample
    check(rand(64, 64, 1), 64, dev)          # one output pixel
    check(rand(2, 2, 2), 2, dev)
    check(rand(1, 1, 3), 1, dev)
    t = torch.from_numpy(rand(40, 50, 4)).to(dev)
    for shape, f in (((1, 50), 2), ((40, 1), 2), ((63, 64), 64), ((64, 63), 64), ((2, 2), Fraction(7, 3))):
        with pytest.raises(ValueError, match="smaller than the factor"):
            area_resample(t[:shape[0], :shape[1]].contiguous(), f)
    with pytest.raises(ValueError, match="GPU memory"):
        area_resample(t.cpu(), 2)
    with pytest.raises(ValueError, match="contiguous"):
        area_resample(t[:, ::2], 2)
    with pytest.raises(ValueError, match="contiguous"):
        area_resample(t.permute(1, 0, 2), 2)
    with pytest.raises(ValueError, match="must be uint8"):
        area_resample(t.to(torch.int16), 2)
    with pytest.raises(ValueError, match=r"uint8\[h, w, 3\]"):
        area_resample(t[:, :, :2].contiguous(), 2)
    with pytest.raises(ValueError, match=r"uint8\[h, w, 3\]"):
        area_resample(t[0], 2)
    with pytest.raises(TypeError, match="float"):
        area_resample(t, 2.0)
    with pytest.raises(ValueError, match="below 1"):
        area_resample(t, Fraction(1, 2))
    with pytest.raises(ValueError, match="at most 64"):
        area_resample(t, 65)
    with pytest.raises(ValueError, match="2048"):
        area_resample(t, Fraction(2049, 2048))
    for bad in (torch.empty((20, 24, 3), dtype=torch.uint8, device=dev), torch.empty((20, 25, 3), dtype=torch.int8, device=dev),
                torch.empty((20, 25, 3), dtype=torch.uint8), torch.empty((20, 50, 3), dtype=torch.uint8, device=dev)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a contiguous uint8"):
            area_resample(t, 2, out=bad)
    inside = t.view(-1)[48:48 + 20 * 25 * 3].view(20, 25, 3)
    with pytest.raises(ValueError, match="overlap"):
        area_resample(t, 2, out=inside)
    with pytest.raises(ValueError, match="overlap"):
        area_resample(t, 1, out=t)


def test_the_library_refuses_what_python_lets_through(dev, built_lib):
    """The C entry checks for itself: sizes that do not follow from the factor, an overlap, an unaligned pointer."""
    t = torch.from_numpy(rand(40, 50, 4)).to(dev)
    o = torch.empty((20, 25, 3), dtype=torch.uint8, device=dev)
    call = built_lib.dh_resample_area
    assert call(t.data_ptr(), 40, 50, 2, 1, o.data_ptr(), 20, 25, None) == 0
    torch.cuda.synchronize()
    for args, word in (((t.data_ptr(), 40, 50, 2, 1, o.data_ptr(), 20, 24, None), b"expected"),
                       ((t.data_ptr(), 40, 50, 1, 2, o.data_ptr(), 20, 25, None), b"outside"),
                       ((t.data_ptr(), 40, 50, 130, 2, o.data_ptr(), 0, 0, None), b"above 64"),
                       ((t.data_ptr(), 1, 50, 2, 1, o.data_ptr(), 0, 25, None), b"no whole output pixel"),
                       ((t.data_ptr(), 40, 50, 2, 1, t.data_ptr() + 48, 20, 25, None), b"overlap"),
                       ((t.data_ptr(), 40, 50, 2, 1, o.data_ptr() + 4, 20, 25, None), b"aligned")):
        assert call(*args) == -22 and word in built_lib.dh_last_error(), word


def test_out_is_honoured_and_the_source_is_left_alone(dev):
    from deephisto_amd.resample import area_resample
    host = rand(131, 257, 9)
    src = torch.from_numpy(host).to(dev)
    for f in (2, Fraction(3, 2), 1):
        want = torch.from_numpy(R.resample(host, f))
        out = torch.full(want.shape, 7, dtype=torch.uint8, device=dev)
        got = area_resample(src, f, out=out)
        assert got is out and torch.equal(out.cpu(), want) and torch.equal(src.cpu(), torch.from_numpy(host))
    # an `out` that does not start at a 16-byte multiple (rows of another tensor) is still honoured
    flat = torch.zeros(8 + 65 * 128 * 3, dtype=torch.uint8, device=dev)
    odd = flat[8:].view(65, 128, 3)
    want = torch.from_numpy(R.resample(host, 2))
    assert area_resample(src, 2, out=odd).data_ptr() == odd.data_ptr() and odd.data_ptr() % 16 == 8
    assert torch.equal(odd.cpu(), want) and not flat[:8].any()
    copy = area_resample(src, 1)
    assert copy.data_ptr() != src.data_ptr() and torch.equal(copy, src)


def test_byte_offsets_past_two_to_the_32(dev):
    """A source of 4.3e9 bytes, built from a 1021 x 1031 block (prime sides: an offset that wrapped by 2^31 or 2^32 bytes lands on
    other pixels).  The output rows whose source rows hold byte offsets 2^31 and 2^32, and the last rows, equal the restatement
    of just those source rows copied back."""
    from deephisto_amd.resample import area_resample, resampled_size
    h, w = 40000, 36000
    block = torch.from_numpy(rand(1021, 1031, 5)).to(dev)
    src = block.repeat(40, 35, 1)[:h, :w].contiguous()
    del block
    assert src.numel() > 2 ** 32
    pitch = 3 * w
    for f in (Fraction(16), Fraction(3, 2)):
        oh, ow = resampled_size(h, w, f)
        got = area_resample(src, f)
        assert tuple(got.shape) == (oh, ow, 3)
        for edge in (2 ** 31, 2 ** 32):
            y = int((edge // pitch) / f)                     # an output row under the source row that holds the offset
            j0, j1 = R.source_rows(f, y - 2, y + 3)
            assert j0 * pitch < edge < j1 * pitch
            want = R.resample_rows(src[j0:j1].cpu().numpy(), j0, f, y - 2, y + 3)
            assert torch.equal(got[y - 2:y + 3].cpu(), torch.from_numpy(want)), (f, edge)
        j0, j1 = R.source_rows(f, oh - 3, oh)
        want = R.resample_rows(src[j0:j1].cpu().numpy(), j0, f, oh - 3, oh)
        assert torch.equal(got[oh - 3:].cpu(), torch.from_numpy(want)), (f, "last rows")
        del got


# ---- PyramidSlide -------------------------------------------------------------------------------------------------------------
def test_pyramid_layers_from_a_device_and_a_host_base(dev, tmp_path):
    from deephisto_amd.resample import PyramidSlide, area_resample
    host = rand(203, 301, 21)                 # 203 is no multiple of 2, 3 or 4
    t = torch.from_numpy(host).to(dev)
    np.save(tmp_path / "s.npy", host)
    p = PyramidSlide(t)
    assert p.layer_device(1) is p.layer_device(1) and p.layer_device(1).data_ptr() == t.data_ptr()
    for L in (2, 3, 4):
        want = area_resample(t, L)
        assert torch.equal(want.cpu(), torch.from_numpy(R.resample(host, L)))
        assert torch.equal(p.layer_device(L), want) and p.layer_device(L) is p.layer_device(L)
        assert p.layer_size(L) == tuple(want.shape[:2])
        np.testing.assert_array_equal(p.get_region_from_layer(L, (3, 5), (40, 61)), want[3:40, 5:61].cpu().numpy())
        # a host base in bands: 13 source rows' worth of bytes give bands of 12 rows at L = 2, 3, 4 (their rows of the layer
        # start at any byte); 50 rows' worth and more give bands in groups of 16 L rows (aligned) where they fit; the last band
        # is shorter
        for base, band_bytes in ((host, 3 * 301 * 13), (host, 3 * 301 * 70), (tmp_path / "s.npy", 3 * 301 * 50), (host, 1 << 30)):
            q = PyramidSlide(base, device=dev, band_bytes=band_bytes)
            rows = q.band_rows(L)
            assert rows % L == 0 and (rows <= band_bytes // (3 * 301) or rows == L)
            if band_bytes < 1 << 30:
                assert (203 // L * L) % rows and 203 // L * L > 2 * rows          # several bands, a shorter last one
            assert torch.equal(q.layer_device(L), want), (L, band_bytes)
            np.testing.assert_array_equal(q.get_region_from_layer(L, (3, 5), (40, 61)), want[3:40, 5:61].cpu().numpy())
            assert torch.equal(q.layer_device(1).cpu(), torch.from_numpy(host))
    p.close()
    assert torch.equal(p.layer_device(2).cpu(), torch.from_numpy(R.resample(host, 2)))


def _model(dtype, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    torch.manual_seed(0)
    return get_model(5, dtype, arch="resnet18").to(dev).eval()


def test_samplers_and_prediction_read_the_layer(dev):
    """`layer=2` over a PyramidSlide is the half-resolution slide: the dense sampler's batches and origins and the predicted class
    map equal those over area_resample(t, 2)."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    from deephisto_amd.resample import PyramidSlide, area_resample
    t = tiles.synth_slide(1111, 1300, 0, dev)
    half = area_resample(t, 2)
    kw = dict(patch_size=128, batch_size=8, stride=96, device=dev)
    a = FullImageDenseSampler(PyramidSlide(t), layer=2, **kw)
    b = FullImageDenseSampler(half, layer=2, **kw)
    assert (a.h, a.w) == (555, 650) == (b.h, b.w) and np.array_equal(a.origins, b.origins) and len(a) == len(b) > 1
    assert torch.equal(a.data_device, half)
    for (xa, oa, _), (xb, ob, _) in zip(a.generator_device(), b.generator_device()):
        assert torch.equal(xa, xb) and np.array_equal(oa, ob)
    host = FullImageDenseSampler(PyramidSlide(t.cpu().numpy(), device=dev, band_bytes=3 * 1300 * 100), layer=2, **kw)
    assert torch.equal(host.data_device, half)
    model = _model("bf16", dev)
    got, want = predict_full_patched(a, model, 5), predict_full_patched(b, model, 5)
    assert got.shape == want.shape == (555 // 16, 650 // 16) and torch.equal(got, want)


def test_annotation_sampler_reads_the_layer(dev):
    """At layer=2 the annotation is halved; over a PyramidSlide the pixels are too.  The records and patches equal those over
    ArraySlide(restatement(a, 2)), where layer=2 only scales the annotation: until now the only truthful way to get them."""
    from deephisto_amd.patch_samplers.region_samplers import AnnoRegionRndSampler
    from deephisto_amd.psimage_compat import ArraySlide
    from deephisto_amd.resample import PyramidSlide
    a = rand(701, 900, 31)
    anno = [{"class": "TUM", "vertices": [[60, 80], [850, 60], [860, 640], [40, 660]]},
            {"class": "LP", "vertices": [[100, 100], [500, 120], [480, 500], [120, 480]]}]
    half = R.resample(a, 2)
    kw = dict(layer=2, patch_size=96, patches_from_one_region=4, device=dev)
    out = []
    for source in (PyramidSlide(a, device=dev, band_bytes=3 * 900 * 64), ArraySlide(half)):
        smp = AnnoRegionRndSampler([(source, anno)], **kw)
        np.random.seed(17); torch.manual_seed(3)
        recs = smp._records(8)
        np.random.seed(17); torch.manual_seed(3)
        x, lab, c = next(smp.device_batches(8, 1))
        np.random.seed(17)
        structs = next(smp.structs_generator(8, 1))
        out.append((recs, x, lab, c, [p.data.copy() for p, _ in structs], smp._bank.size(0)))
    (r0, x0, l0, c0, s0, z0), (r1, x1, l1, c1, s1, z1) = out
    assert r0 == r1 and z0 == z1 == (350, 450)
    assert torch.equal(x0, x1) and torch.equal(l0, l1) and torch.equal(c0, c1)
    for p, q, (_, y, x, _) in zip(s0, s1, r0):
        np.testing.assert_array_equal(p, q)
        np.testing.assert_array_equal(p, half[y:y + 96, x:x + 96])


def test_cli_pyramid(dev, tmp_path, capsys):
    """`--synthetic 2048 3072 --layer 2 --pyramid`: the map of the half-size slide, equal to the in-process call."""
    from deephisto_amd import tiles
    from deephisto_amd.examples.predict_full_patched import main, predict_full_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
    from deephisto_amd.resample import PyramidSlide
    model = _model("bf16", dev)
    argv = ["--synthetic", "2048", "3072", "--layer", "2", "--weights", "", "--batch_size", "16", "--no_visualizations",
            "--out_dir", str(tmp_path / "out")]
    pred = main(argv + ["--pyramid"], model=model)
    assert tuple(pred.shape) == (1024 // 16, 1536 // 16)
    smp = FullImageDenseSampler(PyramidSlide(tiles.synth_slide(2048, 3072, 0, dev)), layer=2, patch_size=224, batch_size=16, stride=112,
                                device=dev)
    assert torch.equal(pred, predict_full_patched(smp, model, 5))
    plain = main(argv, model=model)           # without the flag: one layer, whatever --layer says
    assert tuple(plain.shape) == (2048 // 16, 3072 // 16)
    with pytest.raises(SystemExit):
        main(argv + ["--pyramid", "--ondisk"], model=model)
    assert "--ondisk" in capsys.readouterr().err
