"""Host: the slide-scale GPU tests (tests/test_gpu_slide_scale.py) can fail.

Their two slides (tests/helpers/slide_scale.py) are never held on the host, and their references are computed from coordinates or from
a block's multiplicities.  Here, without a GPU: the virtual images equal the real ones on windows and small slides; at every origin the
tests use, what an address wrapped by 2^31 or 2^32 bytes would read differs from the true bytes almost everywhere; and each error such
a wrap (or a lost tail) would cause, planted in a NumPy restatement, is rejected by the comparison the GPU test makes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import geom_aug_ref as G  # noqa: E402
import slide_scale as SS  # noqa: E402
import stain_aug_ref as A  # noqa: E402
import stain_ref as R  # noqa: E402

from oracle import synth  # noqa: E402
from test_gpu_stain import E_FIX, P_FIX  # noqa: E402

H, W = SS.H, SS.W
SEED = 6


@pytest.fixture(scope="module")
def closed():
    return SS.ClosedForm(H, W, SEED)


@pytest.fixture(scope="module")
def periodic():
    return SS.Periodic(SS.he_block(), H, W)


def test_geometry_and_spots():
    for P in (4, 7, 8, 37, 64, 96, 330, 332):
        for over in (False, True):
            o = SS.spots(H, W, P, over)
            assert o.dtype == np.int32 and len(o) == 14 + 2 * over
            SS.assert_reaches_both_edges(o, H, W, P)
            inside = o[:14]
            assert (inside >= 0).all() and (inside[:, 0] + P <= H).all() and (inside[:, 1] + P <= W).all()
    # a slide below 2^31 bytes has no edge spots, and the check says so
    small = SS.spots(1024, 1024, 256)
    assert len(small) == 8
    with pytest.raises(AssertionError):
        SS.assert_reaches_both_edges(small, 1024, 1024, 256)


def test_closed_form_equals_synth_region(closed):
    for y0, x0, hh, ww in ((0, 0, 5, 9), (H - 40, W - 33, 40, 33), (2 ** 32 // SS.ROW_BYTES - 3, 17, 9, 70), (14978, W - 12, 3, 12)):
        want = synth.synth_region(y0, x0, hh, ww, SEED)
        yy, xx = np.arange(y0, y0 + hh)[:, None], np.arange(x0, x0 + ww)[None, :]
        np.testing.assert_array_equal(closed[yy, xx], want)
        np.testing.assert_array_equal(closed.window(y0, x0, hh, ww), want)
        a = SS.tile_addresses((y0, x0), 3, W)
        np.testing.assert_array_equal(closed.flat(a), want[:3, :3].reshape(3, 9))
    # the two references take it as an image
    small = SS.ClosedForm(40, 52, 3)
    real = synth.synth_slide(40, 52, 3)
    o = np.array([[-3, 5], [4, -2], [30, 47], [11, 23]], np.int32)
    rows = np.array([[32768, 0, 0, 32768], [20000, -9000, 9000, 20000], [0, -32768, 32768, 0], [40000, 30000, -30000, 40000]])
    np.testing.assert_array_equal(A.plain(small, o, 7, True, False), A.plain(real, o, 7, True, False))
    np.testing.assert_array_equal(G.gather(small, o, 7, rows, False, True), G.gather(real, o, 7, rows, False, True))


def test_periodic_views_and_multiplicities():
    """5 x 7 repeats of a 13 x 17 block with ragged ends: every view equals the materialised slide, and the multiplicity sums equal the
    brute-force statistics."""
    block = R.synth_he(13, 17, 3, glass=0.3)
    h, w = 5 * 13 + 6, 7 * 17 + 9
    per = SS.Periodic(block, h, w)
    real = np.tile(block, (6, 8, 1))[:h, :w]
    np.testing.assert_array_equal(per.window(9, 30, 40, 90), real[9:49, 30:120])
    yy, xx = np.arange(60, 71)[:, None], np.arange(100, 128)[None, :]
    np.testing.assert_array_equal(per[yy, xx], real[60:71, 100:128])
    a = SS.tile_addresses((50, 99), 21, w)
    np.testing.assert_array_equal(per.flat(a), real[50:71, 99:120].reshape(21, 63))
    assert sum(m * s.shape[0] * s.shape[1] for m, s in per.parts()) == h * w
    for f in (lambda im: R.moments(im, 219), lambda im: R.angle_hist(im, 219, E_FIX), lambda im: R.conc_hist(im, 219, P_FIX)):
        np.testing.assert_array_equal(per.additive(f), f(real))
        np.testing.assert_array_equal(per.additive_rows(f, 58, 71), f(real[58:71]))
    assert per.additive(lambda im: R.moments(im, 219))[0] > 0
    # no ragged ends: the empty sub-blocks are left out
    assert len(SS.Periodic(block, 26, 34).parts()) == 1


@pytest.mark.parametrize("kind", ["closed", "periodic"])
def test_a_wrapped_address_reads_other_bytes(kind, closed, periodic):
    """For every origin and patch size of the GPU tests: the bytes at the tile's addresses truncated to 32 or 31 bits, whole or in the
    row product only, equal the true bytes in fewer than 2 % of the tile's positions (wherever the truncation moves the address)."""
    img = closed if kind == "closed" else periodic
    worst, moved = 0.0, 0
    for P in (64, 37, 96):
        for y0, x0 in SS.spots(H, W, P):
            a = SS.tile_addresses((y0, x0), P, W)
            true = img.flat(a)
            for modulus in SS.EDGES:
                for rows_only in (False, True):
                    b = SS.wrapped(a, W, modulus, rows_only)
                    m = b != a
                    if not m.any():
                        continue
                    same = float((img.flat(b[m]) == true[m]).mean())
                    worst, moved = max(worst, same), moved + 1
                    assert same < 0.02, (kind, P, y0, x0, modulus, rows_only, same)
    print(f"\n{kind}: {moved} wrapped tiles, at most {worst:.4f} of a tile's bytes unchanged")
    # per P and kind of truncation at least: 31 bits -- two tiles at 2^31, three at 2^32, the two bottom corners; 32 bits -- four of them
    assert moved >= 3 * 2 * (7 + 4)


def test_planted_stain_errors_change_every_statistic(periodic):
    """The whole-slide moments, angle histogram and concentration histogram of the periodic slide (the multiplicity sums the GPU test
    compares with), against the same three with (a) the pixels past byte 2^32 dropped, (b) those pixels read from the head of the slide
    (their addresses less 2^32), (c) the last H * W % 16 = 3 pixels dropped."""
    from deephisto_amd.stain import StainNormalizer
    vmax = StainNormalizer().vmax
    fs = {"moments": lambda im: R.moments(im, vmax), "angle": lambda im: R.angle_hist(im, vmax, E_FIX),
          "conc": lambda im: R.conc_hist(im, vmax, P_FIX)}
    npix = H * W
    p0 = 2 ** 32 // 3 + 1                     # the first pixel wholly past byte 2^32
    ye, xe = divmod(p0, W)
    n_tail = npix - p0
    head_rows = periodic.window(0, 0, -(-(3 * n_tail + 2) // SS.ROW_BYTES), W).reshape(-1)
    head = head_rows[3 * p0 - 2 ** 32:3 * p0 - 2 ** 32 + 3 * n_tail].reshape(1, -1, 3)   # bytes 3 p - 2^32 .. of every tail pixel p
    assert head.shape[1] == n_tail and 3 * p0 - 2 ** 32 == 2
    for name, f in fs.items():
        total = periodic.additive(f)
        tail = f(periodic.window(ye, xe, 1, W - xe)) + periodic.additive_rows(f, ye + 1, H)
        last = f(periodic.window(H - 1, W - 3, 1, 3))
        assert total.sum() > 0 and (tail <= total).all() and (last <= total).all()
        if name != "moments":
            assert int(total.sum()) // (2 if name == "conc" else 1) == int(periodic.additive(fs["moments"])[0])
        dropped = total - tail
        replaced = dropped + f(head)
        short = total - last
        for what, planted in (("dropped", dropped), ("replaced", replaced), ("short", short)):
            assert not np.array_equal(planted, total), (name, what)
        assert int(last.sum()) >= 3            # all three tail pixels are stained


def test_planted_gather_wrap_fails_the_comparison(closed):
    """A gather whose source offset is formed in 32 bits, restated in NumPy, against the reference of the GPU test, through the test's
    own comparison."""
    import torch
    for P in (64, 37):
        o = SS.spots(H, W, P)
        ref = A.plain(closed, o, P)
        true = np.stack([closed.flat(SS.tile_addresses(t, P, W)).reshape(P, P, 3) for t in o]).astype(np.float32) / np.float32(255)
        assert SS.same_bits(torch.from_numpy(true), ref) and SS.same_bits(torch.from_numpy(true).bfloat16(), ref)
        lo, _ = SS.byte_span(o, H, W, P)
        for rows_only in (False, True):
            bad = np.stack([closed.flat(SS.wrapped(SS.tile_addresses(t, P, W), W, 2 ** 32, rows_only)).reshape(P, P, 3) for t in o])
            bad = bad.astype(np.float32) / np.float32(255)
            assert not SS.same_bits(torch.from_numpy(bad), ref) and not SS.same_bits(torch.from_numpy(bad).bfloat16(), ref)
            for k in np.flatnonzero(lo > 2 ** 32):     # each tile past the edge on its own
                assert not SS.same_bits(torch.from_numpy(bad[k]), ref[k])
            for k in np.flatnonzero(lo + P * SS.ROW_BYTES < 2 ** 32):
                assert SS.same_bits(torch.from_numpy(bad[k]), ref[k])


def test_stem_reference_rejects_a_wrapped_tile(closed):
    """The float64 stem reference (conv1 + BN + ReLU + maxpool, the bf16 engine's operands) of a tile past byte 2^32 against the same
    reference fed the bytes at the addresses less 2^32: the project's gate (oracle/layer_ref.py) fails on more than half of the pooled
    elements, so a stem that wrapped could not pass tests/test_gpu_slide_scale.py."""
    import torch
    from oracle import layer_ref as lr
    from layer_parity import _oracle
    ref = _oracle("r18")
    P = 96
    o = SS.spots(H, W, P)
    lo, _ = SS.byte_span(o, H, W, P)
    o = o[lo > 2 ** 32]
    assert len(o) >= 2
    w = ref.conv1.weight.detach().bfloat16().double().numpy()
    sd = {k: v.double().numpy() for k, v in ref.state_dict().items()}
    sc, sh = lr.bn_scale_shift(sd["bn1.weight"], sd["bn1.bias"], sd["bn1.running_mean"], sd["bn1.running_var"])
    sc, sh = sc.astype(np.float32), sh.astype(np.float32)

    def x_of(tiles_u8):
        x = (np.stack(tiles_u8) / 255).astype(np.float32).transpose(0, 3, 1, 2)
        return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().double().numpy()

    a = [SS.tile_addresses(t, P, W) for t in o]
    want, A_ = lr.conv_epilogue(x_of([closed.flat(t).reshape(P, P, 3) for t in a]), w, sc, sh, 2, pool=True, fmt="bf16")
    got, _ = lr.conv_epilogue(x_of([closed.flat(t - 2 ** 32).reshape(P, P, 3) for t in a]), w, sc, sh, 2, pool=True, fmt="bf16")
    K = lr.rounding_count(3, 7, "bf16", False)
    assert lr.gate_mask(want, want, A_, K, "bf16").all()
    ok = lr.gate_mask(got, want, A_, K, "bf16")
    print(f"\nwrapped stem tiles: {1 - ok.mean():.4f} of the pooled elements outside the gate")
    for k in range(len(o)):
        assert (~ok[k]).mean() > 0.5, (k, float((~ok[k]).mean()))
