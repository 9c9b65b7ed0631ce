"""Host-side planning of predict_full_patched (deephisto_amd.predict): the ordered accumulation list and the launch size, and
the names examples/predict_full_patched.py keeps importable.  NumPy only: no GPU, no library load."""
import itertools

import numpy as np
import pytest


def _origins(n_unique, pad):
    """A padded origin list whose every entry is distinct, so that an origin taken from the wrong place shows."""
    o = np.stack([np.arange(n_unique + pad) * 112, 7 + np.arange(n_unique + pad) * 3], axis=1).astype(np.int32)
    return o


def _unfiltered_tail(origins, n_unique, dedupe_padding):
    """The inline tail of predict_full_patched before there was one list: the logits are `cat([unique, corner row x pad])`."""
    pad = len(origins) - n_unique
    rows = np.concatenate([np.arange(n_unique), np.full(pad, n_unique - 1)]) if pad else np.arange(n_unique)
    return (rows[:n_unique], origins[:n_unique]) if dedupe_padding else (rows, origins)


def _masked_tail(origins, n_unique, kept, dedupe_padding):
    """The tissue-filtered tail (_finish_masked) before there was one list: one logits row per kept tile."""
    pad = len(origins) - n_unique
    k = len(kept)
    rows, yx = np.arange(0), origins[:0]
    if k:
        rows, yx = np.arange(k), origins[:n_unique][kept]
        if pad and not dedupe_padding and kept[-1] == n_unique - 1:
            rows = np.concatenate([rows, np.full(pad, k - 1)])
            yx = np.concatenate([yx, origins[n_unique:]])
    return rows, yx


N_UNIQUE = 12
KEPT = {"all": np.arange(N_UNIQUE), "with_corner": np.array([0, 3, 4, 9, 11]), "without_corner": np.array([1, 2, 10]),
        "corner_only": np.array([11]), "empty": np.zeros(0, np.int64)}


@pytest.mark.parametrize("pad,dedupe,kept", list(itertools.product((0, 4), (False, True), (None, *KEPT))))
def test_accumulation_list_equals_the_two_tails(pad, dedupe, kept):
    from deephisto_amd.predict import accumulation_list
    origins = _origins(N_UNIQUE, pad)
    if kept is None:
        want_rows, want_yx = _unfiltered_tail(origins, N_UNIQUE, dedupe)
        rows, yx = accumulation_list(origins, N_UNIQUE, dedupe_padding=dedupe)
        n = N_UNIQUE if dedupe else N_UNIQUE + pad
        np.testing.assert_array_equal(rows, np.minimum(np.arange(n), N_UNIQUE - 1))
        np.testing.assert_array_equal(yx, origins[:n])
    else:
        want_rows, want_yx = _masked_tail(origins, N_UNIQUE, KEPT[kept], dedupe)
        rows, yx = accumulation_list(origins, N_UNIQUE, KEPT[kept], dedupe)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(yx, want_yx)
    assert yx.dtype == np.int32 and yx.shape == (len(rows), 2) and rows.dtype.kind == "i"
    if kept == "all":   # every tile kept is the unfiltered run
        for a, b in zip((rows, yx), accumulation_list(origins, N_UNIQUE, None, dedupe)):
            np.testing.assert_array_equal(a, b)
    if kept == "empty":
        assert len(rows) == 0 and len(yx) == 0


def test_launch_size(monkeypatch):
    from deephisto_amd.predict import launch_size
    monkeypatch.delenv("DH_MB_ALIGN", raising=False)
    assert launch_size(38416, 4096) == 3968
    starts = range(0, 38416, 3968)   # 9 x 3 968 + 2 704
    assert len(starts) == 10 and 38416 - starts[-1] == 2704
    for n in (0, 1, 1000, 4096):
        assert launch_size(n, 4096) == 4096   # one launch: the cap, unchanged
    assert launch_size(1025, 1024) == 640 and launch_size(8192, 4096) == 4096 and launch_size(4097, 4096) == 2176
    assert launch_size(1000, 100) == 100 and launch_size(1001, 100) == 91   # below 128: the plain near-equal size
    for n, mb in itertools.product((129, 4097, 38416, 198916, 10 ** 6 + 1), (64, 128, 1000, 1024, 4096)):
        size = launch_size(n, mb)
        assert 1 <= size <= mb, (n, mb, size)
        assert -(-n // size) == -(-n // mb), "no more launches than full ones would take"
        assert mb < 128 or size % 128 == 0 or size == mb, (n, mb, size)
    monkeypatch.setenv("DH_MB_ALIGN", "0")
    assert launch_size(38416, 4096) == 3842
    assert launch_size(1000, 4096) == 4096


@pytest.mark.parametrize("world,n_unique,micro_batch", list(itertools.product((1, 2, 3), (0, 1, 11, 12, 13), (4, 4096))))
def test_plan_shards_tile_the_work_in_order(world, n_unique, micro_batch):
    """plan_shard with explicit world and rank, no filter, on the CPU: the ranks' [lo, hi) tile [0, n_work) in order, every rank
    sizes the same block for the exchange, and the launch size is launch_size of the rank's own share."""
    from deephisto_amd.plan import TileGrid, plan_shard
    from deephisto_amd.predict import launch_size
    origins = _origins(n_unique, 3 if n_unique else 0)
    grid = TileGrid(origins, n_unique, 112, 2000, 2000)
    end = 0
    for rank in range(world):
        p = plan_shard(grid, world, rank, micro_batch, "cpu")
        assert (p.world, p.rank, p.n_work, p.kept, p.kept_yx_dev, p.fill_class) == (world, rank, n_unique, None, None, None)
        assert p.lo == end and p.lo <= p.hi
        end = p.hi
        assert p.per_rank == -(-n_unique // world) and p.hi - p.lo <= p.per_rank
        assert p.mb == launch_size(p.hi - p.lo, micro_batch)
        assert p.o_dev.dtype.is_floating_point is False and p.o_dev.device.type == "cpu"
        np.testing.assert_array_equal(p.o_dev.numpy(), origins[p.lo:p.hi])
    assert end == n_unique


# every project name importable from deephisto_amd.examples.predict_full_patched before the engine and the visualiser moved out
# (taken by hand from that file; `_finish_masked`, which `_finish` replaced, and the stdlib modules it imported are left out)
SURFACE = (
    "ImagePredictorPatched", "batch_predictor", "load_model", "detect_arch", "resolve_arch", "ARCHS", "main", "_n_classes",
    "shard_range", "exchange_logits", "predict_full_patched", "predict_random_patched", "_forward_streamed", "_side_stream",
    "_SIDE_STREAMS", "perform_and_save_visualizations", "KNOWN_COLORS", "ERROR_COLORS", "save_proba",
    "_anno_from_args", "_tissue_from_args", "_proba_from_args", "_regions_from_args",
    "SlideRegions", "clean_map", "export_annotation", "extract_regions", "label_components", "region_table", "save_regions",
    "trace_polygons", "SlideScore", "confusion", "rasterize_annotation", "save_score", "score_prediction",
    "TissueFilter", "fill_uncovered", "score_tiles", "tiles", "DH_LAYOUT_NCHW", "check", "ResNetHIP", "ResNet18HIP", "get_model",
    "DevicePatch", "FullImageDenseSampler", "Patch", "open_slide",
)


def test_examples_module_keeps_its_import_surface():
    import inspect

    from deephisto_amd import predict, visualize
    from deephisto_amd.examples import predict_full_patched as pfp
    for name in SURFACE:
        assert hasattr(pfp, name), name
    assert pfp.main.__globals__ is vars(pfp)   # tests replace predict_full_patched / predict_random_patched there
    for name in ("shard_range", "exchange_logits", "predict_full_patched", "predict_random_patched"):
        assert getattr(pfp, name) is getattr(predict, name), name
    for name in ("perform_and_save_visualizations", "KNOWN_COLORS", "ERROR_COLORS", "save_proba"):
        assert getattr(pfp, name) is getattr(visualize, name), name
    assert pfp._run.__globals__ is vars(pfp) and {"predict_full_patched", "predict_random_patched"} <= set(pfp._run.__code__.co_names)
    assert list(inspect.signature(pfp.predict_full_patched).parameters) == [
        "sampler", "model", "n_classes", "downscale", "micro_batch", "group", "return_logits", "streams", "dedupe_padding",
        "timing", "tissue", "tissue_info", "return_proba"]
    assert list(inspect.signature(pfp.predict_random_patched).parameters) == [
        "sampler", "model", "n_classes", "downscale", "micro_batch", "return_canvas", "timing", "return_proba"]
