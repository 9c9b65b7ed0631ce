"""GPU: every kernel that reads the resident slide, past byte 2^31 and byte 2^32 of one allocation, against an independent reference.

The slide is 30 301 x 47 791 (tests/helpers/slide_scale.py: 2^32 + 49 377 977 bytes, rows of 143 373 bytes, H * W % 16 == 3), either the
closed-form synthetic slide, whose reference is computed from coordinates, or a 1021 x 1031 H&E block repeated, whose whole-slide
statistics are integer combinations of the block's.  tests/test_slide_scale_host.py shows on the CPU that an address wrapped by 2^31
or 2^32 bytes reads other bytes at every origin used here and that each such error fails the comparisons made here.  Every case
asserts of its own origins that a tile lies on each side of both edges, one holds each edge and one holds the allocation's last byte.

  (a) the seven gather kernels at those origins, bit for bit against oracle/synth.py, stain_aug_ref.py and geom_aug_ref.py;
  (b) gather OUTPUTS past 2^32 bytes and 2^31 elements (and n = 65 535 tiles) from a NaN prefill;
  (c) the stems (ResNet-18 bf16 and f32, ResNet-50 bf16) through the forward taps against oracle/layer_ref.py under the gates of
      tests/test_gpu_layer_parity.py; dh_debug_stem_pool_bf16 against the tap (ResNet-18: the entry takes no ResNet-50 handle);
      forward_tiles / features_tiles / cam_tiles against a small slide of the same windows;
  (d) the four stain passes over the periodic slide, fixed and fitted operands, the fit, out-of-place and in-place apply, and an
      all-black slide (every count of the histograms in one bin, the largest product sums).

RECORDS (one MI355X).  All 36 cases ran on the GPU and passed on their first complete run; no kernel or launcher was changed.  Identical
fraction of the stem against the float64 reference: 1.0000 (ResNet-18 bf16), 1.0000 (ResNet-50 bf16), 0.5941 (ResNet-18 float32; floor
0.12).  Wall time of the file: 5.8 s of a 6.6 s run that also held the two existing large-offset tests; its slowest test
(test_gather_output_past_two_to_the_32_bytes[gather-nchw-f32]) took 0.28 s, `test_byte_offsets_past_two_to_the_32` of
tests/test_gpu_resample.py 0.74 s and of tests/test_gpu_dihedral.py 0.02 s in the same run.  These are records, not thresholds.
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import geom_aug_ref as G  # noqa: E402
import slide_scale as SS  # noqa: E402
import stain_aug_ref as A  # noqa: E402
import stain_ref as R  # noqa: E402

import layer_parity as LP  # noqa: E402
from deephisto_amd import geom_aug as GA  # noqa: E402
from deephisto_amd import stain as S  # noqa: E402
from deephisto_amd._lib import DH_DTYPE_BF16, DH_DTYPE_F32, DH_LAYOUT_NCHW, DH_LAYOUT_NHWC  # noqa: E402
from oracle import layer_ref as lr  # noqa: E402
from oracle import synth  # noqa: E402
from test_gpu_geom_aug import ANGLES, SCALES  # noqa: E402
from test_gpu_stain import E_FIX, M_FIX, P_FIX  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = SS.H, SS.W
SEED = 6
HE = np.array(S.TARGET_HE, dtype=np.float64)
FLIPS = ((False, False), (True, False), (False, True), (True, True))
LAYOUTS = ((DH_LAYOUT_NHWC, "nhwc"), (DH_LAYOUT_NCHW, "nchw"))
DTYPES = (torch.float32, torch.bfloat16)
N_LAUNCH = 65535          # the most tiles dh_tile_gather and its kin take in one launch
PREFILL = 0x7FC0          # a bf16 NaN no gather writes; two of them are a float32 NaN


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _Resident:
    """The one slide-sized tensor of the module: the next one is built after the last one is freed."""

    def __init__(self):
        self.kind, self.slide = None, None

    def get(self, kind, build):
        if self.kind != kind:
            self.drop()
            self.slide, self.kind = build(), kind
        return self.slide

    def drop(self):
        self.kind, self.slide = None, None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def resident(dev):
    r = _Resident()
    yield r
    r.drop()


CLOSED = SS.ClosedForm(H, W, SEED)


@pytest.fixture
def closed(resident, dev):
    return resident.get("closed", lambda: CLOSED.device(dev))


@functools.lru_cache(maxsize=None)
def periodic_host():
    return SS.Periodic(SS.he_block(), H, W)


@pytest.fixture
def periodic(resident, dev):
    return resident.get("periodic", lambda: periodic_host().device(dev))


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


# ---- (a) the gathers, reading past the edges -------------------------------------------------------------------------------------
def test_the_resident_slide_is_the_closed_form(closed):
    assert tuple(closed.shape) == (H, W, 3) and closed.numel() > 2 ** 32
    for y, x in SS.spots(H, W, 64):
        np.testing.assert_array_equal(closed[y:y + 64, x:x + 64].cpu().numpy(), synth.synth_region(int(y), int(x), 64, 64, SEED))


@pytest.mark.parametrize("P", [64, 37, 330, 332])
def test_gather_tiles_past_the_edges(closed, dev, P):
    """P = 64: the fast NCHW and NHWC kernels; 37: the generic kernel; 330 (no multiple of 4, so the generic kernel too): 326 700
    elements a tile, a second trip round its grid-stride loop of 1 024 x 256 threads; 332: the fast kernels' second trip round their
    `pj` / `bj` loops (332 > 256 pixels, 996 > 256 bytes a row)."""
    from deephisto_amd import tiles
    o = SS.spots(H, W, P)
    SS.assert_reaches_both_edges(o, H, W, P)
    u8 = np.stack([CLOSED.window(y, x, P, P) for y, x in o])
    nhwc = u8.astype(np.float32) / np.float32(255)
    ref = {DH_LAYOUT_NHWC: nhwc, DH_LAYOUT_NCHW: np.ascontiguousarray(nhwc.transpose(0, 3, 1, 2))}
    for layout, name in LAYOUTS:
        for dtype in DTYPES:
            got = tiles.gather_tiles(closed, o, P, layout, dtype)
            assert SS.same_bits(got, ref[layout]), (name, dtype)


@pytest.mark.parametrize("P", [8, 7])
def test_gather_aug_and_raw_past_the_edges(closed, dev, P):
    from deephisto_amd import tiles
    o = SS.spots(H, W, P, over=True)
    SS.assert_reaches_both_edges(o, H, W, P)
    o_dev = up(o, dev)
    for layout, name in LAYOUTS:
        for fh, fv in FLIPS:
            ref = A.plain(CLOSED, o, P, fh, fv, nchw=layout == DH_LAYOUT_NCHW)
            for dtype in DTYPES:
                assert SS.same_bits(tiles.gather_tiles_aug(closed, o_dev, P, layout, dtype, fh, fv), ref), (name, fh, fv, dtype)
    px, inside = A.source_pixels(CLOSED, o, P)
    assert not inside.all()
    assert SS.same_bits(tiles.gather_tiles_raw(closed, o_dev, P), px.astype(np.float32))


def stain_rows(n):
    """n parameter rows drawn as tests/test_gpu_stain_aug.py draws its five (row 2 is the identity), repeated."""
    alpha = np.array([[1.3, 0.8], [0.5, 1.5], [1.0, 1.0], [0.82, 1.17], [1.45, 0.55]])
    beta = np.array([[0.05, -0.02], [-0.1, 0.1], [0.0, 0.0], [0.3, 0.0], [-0.04, -0.3]])
    return np.ascontiguousarray(np.resize(S.jitter_params(HE, alpha, beta), (n, 12)))


@pytest.mark.parametrize("P", [64, 37])
def test_gather_stain_aug_past_the_edges(closed, dev, P):
    from deephisto_amd import tiles
    o = SS.spots(H, W, P, over=True)
    SS.assert_reaches_both_edges(o, H, W, P)
    params = stain_rows(len(o))
    o_dev, p_dev = up(o, dev), up(params, dev)
    k = 0
    for layout, name in LAYOUTS:
        for dtype in DTYPES:
            fh, fv = FLIPS[k % 4]
            k += 1
            got = tiles.gather_tiles_stain_aug(closed, o_dev, P, layout, dtype, p_dev, fh, fv, params_host=params)
            assert SS.same_bits(got, A.gather(CLOSED, o, P, params, fh, fv, layout == DH_LAYOUT_NCHW)), (name, dtype, fh, fv)


@functools.lru_cache(maxsize=None)
def affine_case(P):
    """80 tiles: every origin of spots(over=True) under five of the 20 (angle, scale) pairs of tests/test_gpu_geom_aug.py, every pair
    at four origins."""
    o = SS.spots(H, W, P, over=True)
    th, s = np.meshgrid(np.array(ANGLES), np.array(SCALES), indexing="ij")
    rows = GA.affine_params(th.ravel(), s.ravel())
    assert len(o) == 16 and len(rows) == 20
    i = np.arange(80)
    return o[i % 16], np.ascontiguousarray(rows[i % 20]), stain_rows(80)


@pytest.mark.parametrize("stain", [False, True], ids=["plain", "stain"])
@pytest.mark.parametrize("P", [64, 37])
def test_gather_affine_aug_past_the_edges(closed, dev, P, stain):
    from deephisto_amd import tiles
    o, rows, params = affine_case(P)
    SS.assert_reaches_both_edges(o, H, W, P)
    params = params if stain else None
    o_dev, a_dev, p_dev = up(o, dev), up(rows, dev), (up(params, dev) if stain else None)
    k = int(stain)
    for layout, name in LAYOUTS:
        for dtype in DTYPES:
            fh, fv = FLIPS[k % 4]
            k += 1
            got = tiles.gather_tiles_affine_aug(closed, o_dev, P, layout, dtype, a_dev, fh, fv, affine_host=rows, params_dev=p_dev,
                                                params_host=params)
            ref = G.gather(CLOSED, o, P, rows, fh, fv, layout == DH_LAYOUT_NCHW, params=params)
            assert SS.same_bits(got, ref), (name, dtype, fh, fv)
            assert len(np.unique(ref)) > 200 and (ref == 0).any()


# ---- (c) the stems and what reads them -------------------------------------------------------------------------------------------
ENGINES = [("r18", "bf16"), ("r18", "f32"), ("r50", "bf16")]
STEM_P = 96               # 24 pooled columns: two strips of the fused stem and one seam


@pytest.fixture(scope="module", params=ENGINES, ids=["-".join(e) for e in ENGINES])
def engine(request, dev):
    arch, dtype = request.param
    ref = LP._oracle(arch)
    return arch, dtype, ref, LP._model(ref, arch, dtype, dev)


def test_stem_past_the_edges(closed, dev, engine):
    arch, dtype, ref, m = engine
    P = STEM_P
    o = SS.spots(H, W, P)
    SS.assert_reaches_both_edges(o, H, W, P)
    o_dev = up(o, dev)
    sel = np.arange(len(o), dtype=np.int32)
    taps = LP._Taps(m, arch, closed, o_dev, P, sel)
    layers, shapes = LP._shapes(ref, P)
    L = layers[0]
    assert L["name"] == "conv1" and shapes["maxpool"] == (64, 24, 24)
    u8 = np.stack([CLOSED.window(y, x, P, P) for y, x in o])
    x = np.ascontiguousarray((u8 / 255).astype(np.float32).transpose(0, 3, 1, 2)).astype(np.float64)
    if dtype == "bf16":
        x = torch.from_numpy(x).bfloat16().double().numpy()
    fused = dtype == "bf16"
    w_, sc, sh = LP._operands(m, arch, L)
    K = lr.rounding_count(3, 7, dtype, False)
    want, A_ = lr.conv_epilogue(x, w_, sc, sh, 2, None, True, pool=fused, fmt=dtype)
    got = taps.get("conv1", shapes["maxpool"] if fused else shapes["conv1"])
    assert got.shape == want.shape
    ok = lr.gate_mask(got, want, A_, K, dtype)
    assert ok.all(), LP._fail_report(f"{arch} {dtype} conv1", got, want, A_, ok, sel)
    frac = float((got == want).mean())
    print(f"\n{arch} {dtype} stem at slide scale: identical fraction {frac:.4f}")
    assert frac >= LP.IDENTICAL[dtype]
    pooled = taps.get("maxpool", shapes["maxpool"])
    if fused:
        assert np.array_equal(pooled, got)
    else:
        assert np.array_equal(pooled, F.max_pool2d(torch.from_numpy(got), 3, 2, 1).numpy())
        want_p, A_p = lr.conv_epilogue(x, w_, sc, sh, 2, None, True, pool=True, fmt=dtype)
        ok = lr.gate_mask(pooled, want_p, A_p, K, dtype)
        assert ok.all(), LP._fail_report(f"{arch} {dtype} maxpool", pooled, want_p, A_p, ok, sel)
        assert float((pooled == want_p).mean()) >= LP.IDENTICAL[dtype]
    if (arch, dtype) == ("r18", "bf16"):
        from deephisto_amd._lib import check, lib
        direct = torch.empty((len(o), 24, 24, 64), dtype=torch.float32, device=dev)
        check(lib().dh_debug_stem_pool_bf16(m._handle, closed.data_ptr(), H, W, o_dev.data_ptr(), len(o), P, direct.data_ptr(), None),
              "dh_debug_stem_pool_bf16")
        assert np.array_equal(direct.permute(0, 3, 1, 2).cpu().numpy().astype(np.float64), got)


def test_tile_consumers_equal_a_small_slide_of_the_same_windows(closed, dev, engine):
    arch, dtype, _, m = engine
    P = STEM_P
    o = SS.spots(H, W, P)
    SS.assert_reaches_both_edges(o, H, W, P)
    o_dev = up(o, dev)
    small = torch.cat([closed[y:y + P, x:x + P] for y, x in o.tolist()], dim=1).contiguous()
    s_dev = up([[0, k * P] for k in range(len(o))], dev)
    assert tuple(small.shape) == (P, len(o) * P, 3)
    for call in (lambda s, t: m.forward_tiles(s, t, P), lambda s, t: m.features_tiles(s, t, P, return_logits=True),
                 lambda s, t: m.cam_tiles(s, t, P, return_logits=True)):
        big, ref = call(closed, o_dev), call(small, s_dev)
        big, ref = (big, ref) if isinstance(big, tuple) else ((big,), (ref,))
        for a, b in zip(big, ref):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ---- (b) gather outputs past 2^32 bytes and 2^31 elements ------------------------------------------------------------------------
SMALL = 1024


@pytest.fixture
def small_slide(resident, dev):
    from deephisto_amd import tiles
    return resident.get("small", lambda: tiles.synth_slide(SMALL, SMALL, SEED, dev))


@functools.lru_cache(maxsize=None)
def small_host():
    img = synth.synth_slide(SMALL, SMALL, SEED)
    img.setflags(write=False)
    return img


def _prefilled(n_elems, dtype, dev):
    if dtype == torch.bfloat16:
        return torch.full((n_elems,), PREFILL, dtype=torch.int16, device=dev), PREFILL
    word = PREFILL << 16 | PREFILL
    return torch.full((n_elems,), word, dtype=torch.int32, device=dev), word


def _launch(kind, slide, o_dev, n, P, layout, dtype, out):
    from deephisto_amd._lib import check, lib
    from deephisto_amd.tiles import _stream
    code = DH_DTYPE_BF16 if dtype == torch.bfloat16 else DH_DTYPE_F32
    if kind == "gather":
        check(lib().dh_tile_gather(slide.data_ptr(), SMALL, SMALL, o_dev.data_ptr(), None, n, P, layout, code, out.data_ptr(),
                                   _stream(slide.device)), "dh_tile_gather")
    else:
        check(lib().dh_tile_gather_aug(slide.data_ptr(), SMALL, SMALL, o_dev.data_ptr(), n, P, layout, code, 1, 0, out.data_ptr(),
                                       _stream(slide.device)), "dh_tile_gather_aug")


def _check_output(kind, slide, dev, n, P, layout, dtype, picks):
    rng = np.random.default_rng(n + P)
    o = np.stack([rng.integers(0, SMALL - P + 1, n), rng.integers(0, SMALL - P + 1, n)], 1).astype(np.int32)
    per_tile = 3 * P * P
    out, word = _prefilled(n * per_tile, dtype, dev)
    _launch(kind, slide, up(o, dev), n, P, layout, dtype, out)
    assert not bool((out == word).any()), "prefill left in the output"
    nchw = layout == DH_LAYOUT_NCHW
    for k in picks:
        got = out[k * per_tile:(k + 1) * per_tile].view(dtype).view((1, 3, P, P) if nchw else (1, P, P, 3))
        ref = A.plain(small_host(), o[k:k + 1], P, kind == "aug", False, nchw=nchw)
        assert SS.same_bits(got, ref), (kind, layout, dtype, k)
    del out


OUTPUT_CASES = [("gather", DH_LAYOUT_NCHW, torch.float32, 5462), ("gather", DH_LAYOUT_NHWC, torch.float32, 5462),
                ("gather", DH_LAYOUT_NCHW, torch.bfloat16, 10924), ("gather", DH_LAYOUT_NHWC, torch.bfloat16, 10924),
                ("aug", DH_LAYOUT_NHWC, torch.bfloat16, 10924)]


@pytest.mark.parametrize("kind,layout,dtype,n", OUTPUT_CASES,
                         ids=[f"{k}-{'nchw' if lay == DH_LAYOUT_NCHW else 'nhwc'}-{'f32' if d == torch.float32 else 'bf16'}"
                              for k, lay, d, _ in OUTPUT_CASES])
def test_gather_output_past_two_to_the_32_bytes(small_slide, dev, kind, layout, dtype, n):
    """P = 256: a tile is 196 608 elements.  5 462 float32 tiles end 524 288 bytes past byte 2^32; 10 924 bf16 tiles end 262 144
    elements past element 2^31, which is byte 2^32.  Checked: tile 0, the tile before the one that holds the boundary, that tile,
    the one after it where there is one, the last tile -- and no element left as it was."""
    P = 256
    esz = 4 if dtype == torch.float32 else 2
    per_tile = 3 * P * P
    b = 2 ** 32 // (per_tile * esz)            # the tile that holds the boundary: 5 461 (the last one) or 10 922 (the last but one)
    assert 0 < b < n and b * per_tile * esz < 2 ** 32 < n * per_tile * esz
    if dtype == torch.bfloat16:
        assert b * per_tile < 2 ** 31 < n * per_tile
    _check_output(kind, small_slide, dev, n, P, layout, dtype, sorted({0, b - 1, b, min(b + 1, n - 1), n - 1}))


@pytest.mark.parametrize("kind", ["gather", "aug"])
def test_the_most_tiles_of_one_launch(small_slide, dev, kind):
    _check_output(kind, small_slide, dev, N_LAUNCH, 4, DH_LAYOUT_NCHW, torch.float32, [0, N_LAUNCH - 1])


# ---- (d) the stain passes --------------------------------------------------------------------------------------------------------
def _stat(name, vmax, operand=None):
    """(device pass, restatement on an image) of one statistic."""
    if name == "moments":
        return (lambda s: S.stain_moments(s, vmax)), (lambda im: R.moments(im, vmax))
    if name == "angle":
        return (lambda s: S.angle_histogram(s, vmax, operand)), (lambda im: R.angle_hist(im, vmax, operand))
    return (lambda s: S.conc_histogram(s, vmax, operand)), (lambda im: R.conc_hist(im, vmax, operand))


@pytest.fixture(scope="module")
def ref_fit():
    """The fit over the three multiplicity sums of the restatement (host only), and the operands it passed to them."""
    norm, per, seen = S.StainNormalizer(), periodic_host(), {}

    def angle(e):
        seen["angle"] = np.array(e)
        return per.additive(_stat("angle", norm.vmax, e)[1])

    def conc(p):
        seen["conc"] = np.array(p)
        return per.additive(_stat("conc", norm.vmax, p)[1])

    fit = S.fit_with(lambda: per.additive(_stat("moments", norm.vmax)[1]), angle, conc, norm.beta, norm.alpha)
    assert not fit.identity and set(seen) == {"angle", "conc"}
    return fit, seen


def test_the_resident_slide_is_the_periodic_one(periodic):
    per = periodic_host()
    assert tuple(periodic.shape) == (H, W, 3) and (H * W) % 16 == 3
    for y, x in SS.spots(H, W, 64):
        np.testing.assert_array_equal(periodic[y:y + 64, x:x + 64].cpu().numpy(), per.window(int(y), int(x), 64, 64))


@pytest.mark.parametrize("name,operands", [("moments", "none"), ("angle", "fixed"), ("angle", "fitted"), ("conc", "fixed"), ("conc", "fitted")])
def test_stain_statistics_of_the_whole_slide(periodic, ref_fit, name, operands):
    vmax = S.StainNormalizer().vmax
    operand = {"none": None, "fixed": {"angle": E_FIX, "conc": P_FIX}.get(name), "fitted": ref_fit[1].get(name)}[operands]
    device, restated = _stat(name, vmax, operand)
    want = periodic_host().additive(restated)
    assert int(want.sum()) > 2 ** 28           # some hundred million stained pixels
    np.testing.assert_array_equal(device(periodic), want)


def test_stain_fit_of_the_whole_slide(periodic, ref_fit):
    got = S.StainNormalizer().fit(periodic)
    assert got.to_json() == ref_fit[0].to_json()
    assert got.n_stained > 2 ** 28 and not got.identity


def _equals_the_repeated_block(out, block_ref_dev):
    """out[y, x] == block_ref[y % bh, x % bw] over the whole slide, a block row of the slide at a time."""
    bh = block_ref_dev.shape[0]
    band = SS.repeat_on_device(block_ref_dev, bh, W)
    return all(torch.equal(out[y:y + bh], band[:min(bh, H - y)]) for y in range(0, H, bh))


@pytest.mark.parametrize("operands", ["fixed", "fitted"])
def test_stain_apply_over_the_whole_slide(periodic, ref_fit, dev, operands):
    """Out of place and in place (on a clone), both against apply(block) repeated on the device and, at the spots, against the
    restatement of the window."""
    per, norm = periodic_host(), S.StainNormalizer()
    matrix = M_FIX if operands == "fixed" else norm.matrix_q(ref_fit[0])
    run = (lambda s, out: S.apply_fixed(s, M_FIX, out=out)) if operands == "fixed" else (lambda s, out: norm.apply(s, ref_fit[0], out=out))
    block_ref = torch.from_numpy(R.apply_fixed(per.block, matrix)).to(dev)
    assert not torch.equal(block_ref.cpu(), torch.from_numpy(per.block))
    o = SS.spots(H, W, 64)
    SS.assert_reaches_both_edges(o, H, W, 64)
    for in_place in (True, False):
        if in_place:
            out = periodic.clone()
            assert run(out, out) is out
        else:
            out = run(periodic, None)
            assert out.data_ptr() != periodic.data_ptr()
        assert _equals_the_repeated_block(out, block_ref), ("in place" if in_place else "out of place")
        for y, x in o.tolist():
            np.testing.assert_array_equal(out[y:y + 64, x:x + 64].cpu().numpy(), R.apply_fixed(per.window(y, x, 64, 64), matrix))
        np.testing.assert_array_equal(out[H - 1, W - 3:].cpu().numpy(), R.apply_fixed(per.window(H - 1, W - 3, 1, 3), matrix)[0])
        del out
    assert _equals_the_repeated_block(periodic, torch.from_numpy(per.block).to(dev))   # the slide itself is untouched


def test_all_black_slide_fills_one_bin_and_the_largest_sums(resident, dev):
    """1.4e9 black pixels: the accumulator bound of test_passes_equal_the_restatement[black] (tests/test_gpu_stain.py) at slide scale,
    and every count of both histograms in one bin -- the case behind the kernels' "counts stay below 2^32" comments."""
    black = resident.get("black", lambda: torch.zeros((H, W, 3), dtype=torch.uint8, device=dev))
    norm = S.StainNormalizer()
    fit = norm.fit(black)
    assert fit.identity and fit.n_stained == H * W and fit.moments[4] == H * W * 22713 ** 2
    one = np.zeros((1, 1, 3), np.uint8)
    np.testing.assert_array_equal(S.stain_moments(black, norm.vmax), np.uint64(H * W) * R.moments(one, norm.vmax))
    np.testing.assert_array_equal(S.angle_histogram(black, norm.vmax, E_FIX), np.uint64(H * W) * R.angle_hist(one, norm.vmax, E_FIX))
    np.testing.assert_array_equal(S.conc_histogram(black, norm.vmax, P_FIX), np.uint64(H * W) * R.conc_hist(one, norm.vmax, P_FIX))
