"""Host: the definitions behind the fine maps of DESIGN.md section 4.20 without a GPU -- the expanded list, the one-position-per-cell
rule the accumulation kernels apply, and the refusals that fire before any GPU call."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import cam_ref  # noqa: E402


def _origins(rng, n, h, w, P):
    o = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P), (3, 5), (3, 5)]
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(n)]
    return np.asarray(o, np.int32)


@pytest.mark.parametrize("P", [32, 64, 224, 256])
def test_expand_positions_is_the_brute_force_list(P):
    from deephisto_amd import tiles
    o = _origins(np.random.default_rng(P), 9, 700, 900, P)
    got = tiles.expand_positions(o, P)
    want = cam_ref.expand_positions(o, P)
    assert got.dtype == np.int32 and got.flags.c_contiguous and got.shape == (len(o) * (P // 32) ** 2, 2)
    assert np.array_equal(got, want)
    assert tiles.expand_positions(np.zeros((0, 2), np.int32), P).shape == (0, 2)
    # position p = i * S + j: i along y, j along x
    S = P // 32
    assert np.array_equal(got[:S * S].reshape(S, S, 2)[:, 0, 0], o[0, 0] + 32 * np.arange(S))
    assert np.array_equal(got[:S * S].reshape(S, S, 2)[0, :, 1], o[0, 1] + 32 * np.arange(S))


def test_expand_positions_refuses_other_patch_sizes():
    from deephisto_amd import tiles
    for P in (0, 48, 100, -32):
        with pytest.raises(ValueError, match="multiple of 32"):
            tiles.expand_positions(np.zeros((1, 2), np.int32), P)


@pytest.mark.parametrize("d", [1, 7, 16, 32, 48, 100])
@pytest.mark.parametrize("P", [32, 64, 224])
def test_one_position_owns_each_covered_cell(P, d):
    """Along one axis: the sub-tiles' cell ranges partition the tile's, and the formula names the owner.  Both axes are independent,
    so this is the whole rule."""
    S = P // 32
    rng = np.random.default_rng(1000 * P + d)
    for y in [0, 1, d - 1, d, 31, 32, 33, *rng.integers(0, 5000, 60).tolist()]:
        cells = range(y // d, (y + P) // d)
        owners = {c: [i for i in range(S) if (y + 32 * i) // d <= c < (y + 32 * i + 32) // d] for c in cells}
        assert all(len(v) == 1 for v in owners.values()), (P, d, y)
        assert all(cam_ref.owner(c, d, y, P) == v[0] for c, v in owners.items()), (P, d, y)
        # no sub-tile reaches a cell outside the tile's range
        for i in range(S):
            lo, hi = (y + 32 * i) // d, (y + 32 * i + 32) // d
            assert hi <= lo or (lo >= y // d and hi <= (y + P) // d)


def test_reference_loop_over_the_expanded_list_adds_one_row_per_tile_and_cell():
    """cam_ref.accumulate with identical rows at every position is the tile-level loop: counts agree with the tiles' footprints."""
    from oracle import tiling
    rng = np.random.default_rng(5)
    h, w, P, d = 300, 420, 64, 7
    o = _origins(rng, 12, h, w, P)
    v = rng.integers(-8, 8, (len(o), 1, 3)).astype(np.float32)   # small integers: every order of additions is exact
    cam = np.broadcast_to(v, (len(o), (P // 32) ** 2, 3))
    assert np.array_equal(cam_ref.accumulate(h, w, d, P, o, cam), tiling.accumulate_logits(h, w, 3, d, P, o, v[:, 0]))


def test_predict_fine_patched_refuses_before_any_gpu_call(built_lib):
    from deephisto_amd.cam import predict_fine_patched
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, FullImageRndSampler
    from oracle import synth

    class Streamed(FullImageDenseSampler):
        resident = property(lambda self: False)

    host = synth.synth_slide(200, 260, 1)
    model = object()
    with pytest.raises(ValueError, match="multiple of 32"):
        predict_fine_patched(FullImageDenseSampler(host, layer=1, patch_size=48, batch_size=4, stride=48, device="cpu"), model, 5)
    dense = FullImageDenseSampler(host, layer=1, patch_size=64, batch_size=4, stride=64, device="cpu")
    with pytest.raises(ValueError, match="64 classes"):
        predict_fine_patched(dense, model, 65)
    with pytest.raises(ValueError, match="dense sampler"):
        predict_fine_patched(object.__new__(FullImageRndSampler), model, 5)
    with pytest.raises(ValueError, match="resident"):
        predict_fine_patched(Streamed(host, layer=1, patch_size=64, batch_size=4, stride=64, device="cpu"), model, 5)
    with pytest.raises(TypeError):
        predict_fine_patched(dense, model, 5, tta="d4")


def test_entries_refuse_bad_arguments_on_the_host(built_lib):
    """P = 48 and a null handle are refused by the cam_tiles entries, bad patch sizes by the accumulations: no GPU call is reached."""
    import ctypes as C
    one = (C.c_float * 8)()
    err = lambda: built_lib.dh_last_error().decode()   # noqa: E731
    for entry in (built_lib.dh_resnet18_cam_tiles, built_lib.dh_resnet50_cam_tiles):
        assert entry(None, one, 300, 300, one, 4, 96, one, None, None) == -22 and "null handle" in err()
    h18 = C.c_void_p()
    assert built_lib.dh_resnet18_create(C.byref(h18), 5, 1) == 0
    assert built_lib.dh_resnet18_cam_tiles(h18, one, 300, 300, one, 4, 48, one, None, None) == -22 and "multiple of 32" in err()
    assert built_lib.dh_resnet18_cam_tiles(h18, one, 300, 300, one, 4, 96, one, None, None) == -22 and "finalize" in err()
    built_lib.dh_resnet18_destroy(h18)
    h65 = C.c_void_p()
    assert built_lib.dh_resnet50_create(C.byref(h65), 65) == 0
    assert built_lib.dh_resnet50_cam_tiles(h65, one, 300, 300, one, 4, 64, one, None, None) == -22 and "65 classes" in err()
    built_lib.dh_resnet50_destroy(h65)
    yx = (C.c_int32 * 2)()
    assert built_lib.dh_accumulate_cam(one, yx, 1, 48, 16, 5, 300, 300, one, None, None) == -22 and "multiple of 32" in err()
    assert built_lib.dh_accumulate_cam_mean(one, yx, 1, 48, 16, 5, 300, 300, one, one, None, None, -1, None) == -22
    assert "multiple of 32" in err()
    assert built_lib.dh_accumulate_cam_mean(one, yx, 1, 64, 16, 65, 300, 300, one, one, None, None, -1, None) == -22 and "n_cls" in err()


@pytest.mark.parametrize("other", [["--random_sampler"], ["--ondisk"], ["--tta", "flips"], ["--tta", "d4"], ["--clusters", "4"],
                                   ["--pca", "3"], ["--patch_size", "48"]])
def test_cli_refuses_fine_off_its_route(built_lib, capsys, other):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(["--synthetic", "300", "300", "--weights", "", "--fine", *other])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert "--fine" in capsys.readouterr().err


def test_cli_refuses_fine_with_stored_embeddings(built_lib, tmp_path, capsys):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(["--synthetic", "300", "300", "--weights", "", "--fine", "--save_embeddings", str(tmp_path / "e.npz")])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert "--fine" in capsys.readouterr().err


def test_cli_takes_fine_with_the_flags_it_composes_with(built_lib):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(["--synthetic", "300", "300", "--weights", "", "--fine", "--proba", "--heat", "TUM", "--tissue", "otsu",
                          "--stain", "macenko", "--patch_size", "64", "--stride", "32"])
    _check_args(ap, args)
    assert args.fine and not ap.parse_args(["--synthetic", "300", "300"]).fine
