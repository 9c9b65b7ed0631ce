"""Whole-slide probability maps, host side: the NumPy restatement `proba_np` that the GPU tests compare
against is pinned to the pinned oracle (identity instead of softmax, no division: oracle.tiling.accumulate_logits bit for bit;
counts: a brute-force per-cell count), the CLI's refusals, and the C entry points' argument checks.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from oracle import tiling


def softmax_np(v, dtype=np.float32):
    """One row: m = max, e_c = exp(x_c - m), s = e_0 + e_1 + ... in class order, p_c = e_c / s, all in `dtype`."""
    v = np.asarray(v, dtype=dtype)
    e = np.exp(v - v.max())
    s = dtype(0)
    for c in range(len(e)):
        s = s + e[c]
    return e / s


def proba_np(h, w, n_cls, d, runs, dtype=np.float32, fill=-1, softmax=True, divide=True):
    """The reference's accumulation loop with its `count` array and `prediction /= count` enabled and a softmax on each patch's
    prediction.  `runs`: [(patch, origins int[n, 2], rows [n, n_cls])], applied in order; rows are logits (`softmax`) or values
    taken as they are.  Returns dict(sum, count, proba, class_map, confidence); cells nothing covers: proba 0, class `fill`."""
    prediction = np.zeros([h // d, w // d, n_cls], dtype=dtype)
    count = np.zeros([h // d, w // d], dtype=np.int32)
    for patch, origins, rows in runs:
        for (y, x), v in zip(np.asarray(origins).tolist(), rows):
            p = softmax_np(v, dtype) if softmax else np.asarray(v, dtype=dtype)
            prediction[y // d:(y + patch) // d, x // d:(x + patch) // d, :] += p
            count[y // d:(y + patch) // d, x // d:(x + patch) // d] += 1
    out = dict(sum=prediction.copy(), count=count)
    if not divide:
        return out
    covered = count > 0
    proba = np.zeros_like(prediction)
    proba[covered] = prediction[covered] / count[covered][:, None].astype(dtype)
    class_map = np.argmax(proba, axis=2).astype(np.int64)
    confidence = np.take_along_axis(proba, class_map[..., None], axis=2)[..., 0]
    class_map[~covered] = fill
    out.update(proba=proba, class_map=class_map, confidence=confidence)
    return out


def brute_count(h, w, d, patch, origins):
    """count[cy, cx] = number of tiles with y//d <= cy < (y+P)//d and x//d <= cx < (x+P)//d: no slicing, one comparison per
    (tile, row) and (tile, column)."""
    o = np.asarray(origins, dtype=np.int64)
    cy, cx = np.arange(h // d)[None, :], np.arange(w // d)[None, :]
    rows = ((o[:, :1] // d <= cy) & (cy < (o[:, :1] + patch) // d)).astype(np.int64)
    cols = ((o[:, 1:] // d <= cx) & (cx < (o[:, 1:] + patch) // d)).astype(np.int64)
    return (rows.T @ cols).astype(np.int32)


def test_restatement_is_pinned_to_the_oracle(golden_meta):
    grids = {k: g for k, g in golden_meta["grids"].items() if g["h"] < 50000}
    assert {"g4096_224_112_16", "g1000x1300_256_256_16", "g256x600_256_256_4"} <= set(grids)
    for k, (name, g) in enumerate(sorted(grids.items())):
        h, w, P = g["h"], g["w"], g["patch"]
        o = tiling.batched_origins(h, w, P, g["stride"], g["batch"]).reshape(-1, 2)
        assert len(o) == g["n_padded"]
        for d in (16, 7):
            logits = (np.random.default_rng(100 * k + d).standard_normal((len(o), 5)) * 3).astype(np.float32)
            got = proba_np(h, w, 5, d, [(P, o, logits)], softmax=False, divide=False)
            want = tiling.accumulate_logits(h, w, 5, d, P, o, logits)
            assert got["sum"].dtype == np.float32 and got["sum"].tobytes() == want.tobytes(), (name, d)
            np.testing.assert_array_equal(got["count"], brute_count(h, w, d, P, o), err_msg=f"{name} d={d}")


def test_restatement_finish_rules():
    """Division, first maximum, confidence and the fill on a hand-made case; counts above 255 do not wrap."""
    o = np.array([[0, 0]] * 300 + [[0, 16]], np.int32)
    rows = np.tile(np.array([[0.25, 0.5, 0.25]], np.float32), (301, 1))
    rows[300] = [0.5, 0.5, 0.0]
    r = proba_np(32, 64, 3, 16, [(16, o, rows)], softmax=False, fill=-1)
    np.testing.assert_array_equal(r["count"], [[300, 1, 0, 0], [0, 0, 0, 0]])
    np.testing.assert_array_equal(r["class_map"], [[1, 0, -1, -1], [-1, -1, -1, -1]])
    np.testing.assert_array_equal(r["confidence"], np.array([[0.5, 0.5, 0, 0], [0, 0, 0, 0]], np.float32))
    assert r["proba"][0, 0].tolist() == [0.25, 0.5, 0.25] and not r["proba"][1].any()
    p = softmax_np(np.array([80.0, -80.0, 0.0], np.float32))
    assert p[0] == 1.0 and p.sum() == 1.0 and np.isfinite(p).all()
    assert np.array_equal(softmax_np(np.full(4, 7.5, np.float32)), np.full(4, 0.25, np.float32))


@pytest.mark.parametrize("extra,msg", [(["--proba", "--heat", "NOPE"], "--heat"),
                                       (["--heat", "TUM"], "--heat needs --proba"),
                                       (["--save_proba", "p.npy"], "--save_proba needs --proba")])
def test_cli_refuses_bad_proba_flags(extra, msg, capsys, monkeypatch):
    """Refused by argparse before the process group or any GPU is touched."""
    from deephisto_amd import distributed
    from deephisto_amd.examples.predict_full_patched import main
    monkeypatch.setattr(distributed, "init_from_env", lambda *a, **k: pytest.fail("init_from_env was reached"))
    with pytest.raises(SystemExit) as e:
        main(["--synthetic", "512", "512", "--weights", "", *extra])
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_c_entries_refuse_bad_arguments(built_lib):
    """Argument checks of the four C entries; every case fails before a device call, so fake addresses are safe here."""
    lib = built_lib
    fake = C.c_void_p(1 << 20)
    yx = np.zeros((2, 2), np.int32).ctypes.data_as(C.c_void_p)
    col = (C.c_uint8 * 3)(255, 0, 0)

    def err():
        return lib.dh_last_error()

    assert lib.dh_softmax_rows(fake, 4, 65, fake, None) == -22 and b"n_cls=65" in err()
    assert lib.dh_softmax_rows(fake, 4, 0, fake, None) == -22 and b"n_cls=0" in err()
    assert lib.dh_softmax_rows(fake, -1, 5, fake, None) == -22 and b"n=-1" in err()
    assert lib.dh_softmax_rows(None, 4, 5, fake, None) == -22 and b"logits" in err()
    assert lib.dh_softmax_rows(None, 0, 5, None, None) == 0

    def acc(n=2, P=32, d=16, n_cls=5, h=100, w=100, s=fake, c=fake, m=fake, cf=fake, probs=fake):
        return lib.dh_accumulate_mean(probs, yx, n, P, d, n_cls, h, w, s, c, m, cf, -1, None)

    assert acc(n_cls=65) == -22 and b"n_cls=65" in err()
    assert acc(n=-1) == -22 and b"n=-1" in err()
    assert acc(P=0) == -22 and b"patch=0" in err()
    assert acc(d=0) == -22 and b"downscale=0" in err()
    assert acc(h=0) == -22 and b"h=0" in err()
    assert acc(s=None) == -22 and b"sum" in err()
    assert acc(c=None) == -22 and b"count" in err()
    assert acc(cf=None) == -22 and b"confidence" in err()
    assert acc(probs=None) == -22 and b"probs" in err()
    assert acc(h=10, w=10) == 0   # an empty canvas: nothing to do
    assert lib.dh_finish_mean(fake, fake, 10, 65, -1, fake, fake, fake, None) == -22 and b"n_cls=65" in err()
    assert lib.dh_finish_mean(fake, None, 10, 5, -1, fake, fake, fake, None) == -22 and b"count" in err()
    assert lib.dh_finish_mean(fake, fake, -3, 5, -1, fake, fake, fake, None) == -22 and b"n_cells=-3" in err()
    assert lib.dh_heatmap_blend(fake, fake, 1, 10, col, 1.5, fake, None) == -22 and b"alpha=1.5" in err()
    assert lib.dh_heatmap_blend(fake, fake, 0, 10, col, 0.5, fake, None) == -22 and b"field_stride=0" in err()
    assert lib.dh_heatmap_blend(fake, fake, 1, 10, None, 0.5, fake, None) == -22 and b"color" in err()
    assert lib.dh_heatmap_blend(None, fake, 1, 10, col, 0.5, fake, None) == -22 and b"img" in err()


def test_wrappers_refuse_host_tensors():
    """The Python wrappers check their arguments before any library call."""
    import torch

    from deephisto_amd import tiles
    with pytest.raises(ValueError, match="logits must live in GPU memory"):
        tiles.softmax_rows(torch.zeros(3, 5))
    with pytest.raises(ValueError, match="logits must live in GPU memory"):
        tiles.accumulate_probabilities(torch.zeros(3, 5), np.zeros((3, 2), np.int32), 32, 16, 64, 64)
    with pytest.raises(ValueError, match="img must live in GPU memory"):
        tiles.heatmap_blend(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4), (255, 0, 0))
