"""Host side of test-time augmentation: origin mapping, group tables, named view sets, refusals and the
CLI flag, all against the NumPy definition  view = k + 4 f:  np.rot90(np.fliplr(s) if f else s, k).  No GPU."""
import numpy as np
import pytest


def view_np(a, v):
    return np.rot90(np.fliplr(a) if v >> 2 else a, v & 3)


def test_names_ids_and_shapes():
    from deephisto_amd import tta
    assert tta.VIEWS == ("r0", "r90", "r180", "r270", "r0f", "r90f", "r180f", "r270f")
    a = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    for v, name in enumerate(tta.VIEWS):
        assert tta.view_id(name) == tta.view_id(v) == v
        assert tta.view_shape(2, 3, name) == view_np(a, v).shape[:2] == tta.view_shape(2, 3, v)
    for bad in ("r45", 8, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="unknown view"):
            tta.view_id(bad)


def test_map_origins_equals_numpy_for_every_view():
    """The mapped tile of the view is the view of the tile: ragged h != w, several patch sizes, the four corners and random
    origins."""
    from deephisto_amd import tta
    rng = np.random.default_rng(5)
    for h, w, P in ((37, 53, 8), (53, 37, 7), (64, 65, 64), (20, 31, 1), (19, 19, 19), (90, 41, 16)):
        slide = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        corners = [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
        inner = np.stack([rng.integers(0, h - P + 1, 12), rng.integers(0, w - P + 1, 12)], axis=1)
        origins = np.concatenate([np.array(corners), inner]).astype(np.int32)
        for v in range(8):
            img = view_np(slide, v)
            assert img.shape[:2] == tta.view_shape(h, w, v)
            mapped = tta.map_origins(origins, h, w, P, v)
            assert mapped.dtype == np.int32 and mapped.shape == origins.shape
            assert np.array_equal(mapped, tta.map_origins(origins.tolist(), h, w, P, tta.VIEWS[v]))
            for (y, x), (my, mx) in zip(origins, mapped):
                assert 0 <= my <= img.shape[0] - P and 0 <= mx <= img.shape[1] - P
                assert np.array_equal(img[my:my + P, mx:mx + P], view_np(slide[y:y + P, x:x + P], v)), (h, w, P, v, y, x)
    assert np.array_equal(tta.map_origins([(2, 3)], 10, 20, 4, "r90"), [[20 - 4 - 3, 2]])      # (y, x) -> (W - P - x, y)
    assert np.array_equal(tta.map_origins([(2, 3)], 10, 20, 4, "r0f"), [[2, 20 - 4 - 3]])      # (y, x) -> (y, W - P - x)
    assert tta.map_origins(np.zeros((0, 2), np.int32), 10, 20, 4, 3).shape == (0, 2)
    with pytest.raises(ValueError, match="integer array"):
        tta.map_origins(np.zeros((3, 2), np.float32), 10, 20, 4, 1)
    with pytest.raises(ValueError, match="integer array"):
        tta.map_origins(np.zeros((3, 3), np.int32), 10, 20, 4, 1)


def test_device_twin_of_map_origins_on_cpu_tensors():
    """The torch twin is integer arithmetic on int32 tensors; on CPU tensors it gives the host table's numbers."""
    import torch
    from deephisto_amd import tta
    rng = np.random.default_rng(6)
    o = np.stack([rng.integers(0, 600 - 256, 40), rng.integers(0, 700 - 256, 40)], axis=1).astype(np.int32)
    for v in range(8):
        got = tta.map_origins_device(torch.from_numpy(o), 600, 700, 256, v)
        assert got.dtype == torch.int32 and got.is_contiguous()
        assert np.array_equal(got.numpy(), tta.map_origins(o, 600, 700, 256, v))


def test_group_tables_agree_with_numpy():
    from deephisto_amd import tta
    a = np.arange(2 * 3).reshape(2, 3)          # no symmetry: the eight views differ
    views = [view_np(a, v) for v in range(8)]
    assert all(not (x.shape == y.shape and np.array_equal(x, y)) for i, x in enumerate(views) for y in views[:i])
    for p in range(8):
        for q in range(8):
            c = tta.compose(p, q)               # p first, then q
            assert c == tta.COMPOSE[p][q] == tta.compose(tta.VIEWS[p], tta.VIEWS[q])
            assert np.array_equal(view_np(view_np(a, p), q), views[c]), (p, q, c)
        i = tta.inverse(p)
        assert i == tta.INVERSE[p] and tta.compose(p, i) == 0 == tta.compose(i, p)
        assert np.array_equal(view_np(views[p], i), a)


def test_named_sets():
    from deephisto_amd import tta
    a = np.arange(2 * 3).reshape(2, 3)
    assert tta.TestTimeAugmenter().views == tta.TestTimeAugmenter("d4").views == tta.VIEWS
    assert tta.TestTimeAugmenter("rot").views == ("r0", "r90", "r180", "r270")
    flips = tta.TestTimeAugmenter("flips")
    assert flips.views == ("r0", "r0f", "r180f", "r180") and len(flips) == 4
    want = [a, np.fliplr(a), np.flipud(a), np.rot90(a, 2)]
    for v, w in zip(flips.ids, want):
        assert np.array_equal(view_np(a, v), w)
    custom = tta.TestTimeAugmenter(["r270f", "r0"])
    assert custom.views == ("r270f", "r0") and custom.ids == (7, 0)
    assert tta.as_augmenter(None) is None and tta.as_augmenter(custom) is custom and tta.as_augmenter("rot").views == tta.NAMED_SETS["rot"]


def test_refusals_name_the_offender():
    from deephisto_amd import tta
    with pytest.raises(ValueError, match="empty"):
        tta.TestTimeAugmenter([])
    with pytest.raises(ValueError, match="unknown view 'r45'"):
        tta.TestTimeAugmenter(["r0", "r45"])
    with pytest.raises(ValueError, match="unknown view 3"):
        tta.TestTimeAugmenter(["r0", 3])
    with pytest.raises(ValueError, match="duplicate view 'r90'"):
        tta.TestTimeAugmenter(["r90", "r0", "r90"])
    with pytest.raises(ValueError, match="unknown view set 'all'"):
        tta.TestTimeAugmenter("all")


def test_combination_is_the_stated_float32_fold():
    """acc = L[0]; acc += L[k]; acc *= float32(1 / V), in that order, on CPU tensors against NumPy float32."""
    import torch
    from deephisto_amd import tta
    rng = np.random.default_rng(7)
    for views in ("d4", "flips", ["r0", "r90", "r180f"], ["r90"]):
        aug = tta.TestTimeAugmenter(views)
        L = [(rng.standard_normal((9, 5)) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in aug.views]
        keep = [x.copy() for x in L]
        acc = L[0].copy()
        for x in L[1:]:
            acc += x
        acc *= np.float32(1 / len(L))
        got = aug.combine([torch.from_numpy(x) for x in L])
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), acc)
        assert all(np.array_equal(x, k) for x, k in zip(L, keep))           # the inputs are left alone
    with pytest.raises(ValueError, match="3 logits tensors for 4 views"):
        tta.TestTimeAugmenter("rot").combine([torch.zeros(1, 5)] * 3)


def test_kernel_constants():
    from deephisto_amd import resample, tta
    assert tta.TILE == 64 and tta.THREADS == 256 and tta.STORE_GROUP == 16 == resample.STORE_GROUP
    assert tta.LDS_PITCH == 196 and tta.LDS_PITCH % 4 == 0 and (tta.LDS_PITCH // 4) % 2 == 1 and tta.LDS_PITCH >= 3 * tta.TILE


def test_cli_flag(capsys):
    from deephisto_amd.examples import predict_full_patched as P
    ap = P._build_parser()
    base = ["--synthetic", "512", "512", "--weights", ""]
    args = ap.parse_args(base)
    P._check_args(ap, args)
    assert args.tta == "off" and args.tta_aug is None
    for name, n in (("flips", 4), ("d4", 8)):
        args = ap.parse_args(base + ["--tta", name])
        P._check_args(ap, args)
        assert args.tta_aug.views == P.TestTimeAugmenter(name).views and len(args.tta_aug) == n
    args = ap.parse_args(base + ["--tta", "d4", "--random_sampler"])
    P._check_args(ap, args)                     # the fused random route takes it
    assert len(args.tta_aug) == 8
    with pytest.raises(SystemExit):
        P._check_args(ap, ap.parse_args(base + ["--tta", "d4", "--ondisk"]))
    assert "--tta" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--tta", "rot"])
    capsys.readouterr()


def test_cli_refuses_the_callback_route_before_any_gpu(capsys, monkeypatch):
    """`--tta d4 --ondisk`, and a foreign model under --random_sampler, end in ap.error before the process group is touched."""
    import torch
    from deephisto_amd import distributed
    from deephisto_amd.examples import predict_full_patched as P

    def never(*a, **k):
        raise AssertionError("the process group was touched")
    monkeypatch.setattr(distributed, "init_from_env", never)
    base = ["--synthetic", "512", "512", "--weights", "", "--no_visualizations"]
    with pytest.raises(SystemExit):
        P.main(base + ["--tta", "d4", "--ondisk"])
    assert "--ondisk" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        P.main(base + ["--tta", "flips", "--random_sampler"], model=torch.nn.Linear(3, 5))
    assert "callback" in capsys.readouterr().err


def test_signatures_keep_their_positional_parameters():
    """`tta=` / `tta_info=` are keyword-only beside `stain=`: the positional parameters are the reference's, as before."""
    import inspect
    from deephisto_amd import predict
    for fn in (predict.predict_full_patched, predict.predict_random_patched):
        assert all(p.kind is p.POSITIONAL_OR_KEYWORD for p in inspect.signature(fn).parameters.values())
        assert "tta" in fn.__doc__ and "tta" not in inspect.signature(fn).parameters
        with pytest.raises(TypeError):
            fn(*([None] * (len(inspect.signature(fn).parameters) + 1)))
