"""Tile embeddings, host side (CPU only: no kernel runs): the NumPy restatement of the embed kernels against itself, tile labels, the
.npz round trips, every refused combination, the argument checks of the new entry points (before any GPU call, as in test_abi.py)
and the exchange of 512-wide rows over two gloo ranks."""
import ctypes as C
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import embed_ref as er  # noqa: E402


def _emb(origins, h, w, P, S, D=64, logits=False, **kw):
    from deephisto_amd.embeddings import SlideEmbeddings
    rng = np.random.default_rng(len(origins))
    n = len(origins)
    return SlideEmbeddings(torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)), origins, np.arange(n),
                           torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)) if logits else None,
                           patch_size=P, stride=S, h=h, w=w, **kw)


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_class_sums_ref_is_the_contract_order():
    """Two chunks and a ragged third: the restatement equals the order written out by hand, differs from a plain float32 running sum
    somewhere (so the order is observable), counts exactly and ignores labels outside [0, K)."""
    rng = np.random.default_rng(3)
    n, D, K = 2 * er.CHUNK_ROWS + 77, 8, 3
    f = (rng.standard_normal((n, D)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)
    lab = rng.integers(-1, K + 1, n).astype(np.int32)          # -1 and K among them
    sums, counts = er.class_sums_ref(f, lab, K)
    assert sums.dtype == np.float32 and counts.dtype == np.int64
    assert counts.tolist() == [int((lab == k).sum()) for k in range(K)]
    by_hand = np.zeros((K, D), np.float32)
    for c0 in (0, er.CHUNK_ROWS, 2 * er.CHUNK_ROWS):
        part = np.zeros((K, D), np.float32)
        for r in range(c0, min(c0 + er.CHUNK_ROWS, n)):
            if 0 <= lab[r] < K:
                part[lab[r]] = part[lab[r]] + f[r]
        by_hand = by_hand + part
    assert np.array_equal(sums, by_hand)
    running = np.zeros((K, D), np.float32)
    for r in range(n):
        if 0 <= lab[r] < K:
            running[lab[r]] = running[lab[r]] + f[r]
    assert not np.array_equal(sums, running)
    exact = np.stack([f[lab == k].astype(np.float64).sum(0) for k in range(K)])
    mag = np.stack([np.abs(f[lab == k]).astype(np.float64).sum(0) for k in range(K)])
    assert np.all(np.abs(sums - exact) <= (er.CHUNK_ROWS + 3) * er.U * mag)
    # an empty class, and everything in one class
    s1, c1 = er.class_sums_ref(f, np.where(lab == 1, -1, lab), K)
    assert c1[1] == 0 and not s1[1].any() and np.array_equal(s1[0], sums[0])
    s2, c2 = er.class_sums_ref(f, np.zeros(n, np.int32), 1)
    assert c2.tolist() == [n]


def test_normalize_and_scores_ref():
    rng = np.random.default_rng(5)
    f = rng.standard_normal((9, 64)).astype(np.float32)
    f[3] = 0
    f[4] = 0
    f[4, 17] = -2.5
    x = er.normalize_ref(f)
    assert not x[3].any() and x[4, 17] == -1.0 and np.count_nonzero(x[4]) == 1
    assert np.allclose((x * x).sum(1)[[0, 1, 2, 4, 5]], 1.0, rtol=0, atol=1e-15)
    p = rng.standard_normal((5, 64)).astype(np.float32)
    sc, bound = er.scores_ref(f, p, -2.0)
    assert sc.shape == bound.shape == (9, 5) and not sc[3].any() and not bound[3].any()
    got = (-2.0 * (f @ p.T)).astype(np.float64)      # a float32 product is inside its own bound
    assert np.all(np.abs(got - sc) <= bound)


ANNO_SEED = 36   # synthetic_annotation(700, 900, 2, 24, ...): four tile centres in a region of class 2 (LP), four in one of class 1 (BG);
                 # one region lies on the glass band of columns 380 .. 559, the other on tissue


def test_prototype_reference_alone_keeps_near_ties_rare():
    """The cap of tests/test_gpu_embeddings.py on undecided cells (at most 1 % of the cells), on the CPU: the float64 pipeline over
    seeded stand-in features on that test's grid (700 x 900, P = 96, stride 64, downscale 16, glass over columns 380 .. 559) with that
    test's labels (the two-region synthetic annotation of ANNO_SEED).  A stand-in row mixes a tissue and a glass direction by the
    tile's share of glass columns.  Measured: 0 undecided cells of 2 408 at D = 512, 0 at D = 2048 (the cap is 24)."""
    from deephisto_amd.anno.utils import AnnoDescription
    from deephisto_amd.scoring import annotation_rings, synthetic_annotation
    from deephisto_amd.visualize import KNOWN_COLORS
    from oracle import tiling
    h, w, P, S, d, K = 700, 900, 96, 64, 16, 5
    o = tiling.tile_origins(h, w, P, S)
    dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
    xy, start, cls, _ = annotation_rings(synthetic_annotation(h, w, 2, 24, list(KNOWN_COLORS), seed=ANNO_SEED), dsc, 1, h, w)
    lab = er.tile_labels_ref(xy, start, cls, o, P, d, h, w)
    assert np.bincount(lab[lab >= 0], minlength=K).tolist() == [0, 4, 4, 0, 0]
    glass = np.clip(np.minimum(o[:, 1] + P, 560) - np.maximum(o[:, 1], 380), 0, P) / P      # share of glass columns per tile
    assert {float(g) for k in (1, 2) for g in glass[lab == k]} == {0.0, 1.0}, "one region on glass, one on tissue"
    for D in (512, 2048):
        tissue = er.standin_features(len(o), D, 7)
        white = er.standin_features(1, D, 8)[0]
        f = ((1 - glass)[:, None] * tissue + glass[:, None] * white).astype(np.float32)
        cmap, decided = er.prototype_map_ref(f, lab, K, o, P, d, h, w)
        covered = cmap >= 0
        undecided = int((covered & ~decided).sum())
        print(f"D = {D}: {undecided} undecided cells of {cmap.size}")
        assert covered.all() and undecided <= 0.01 * cmap.size, (D, undecided)
        assert set(np.unique(cmap)) <= {1, 2}


# ---- tile labels ------------------------------------------------------------------------------------------------------
def test_tile_labels_on_hand_made_maps(built_lib):
    from deephisto_amd.embeddings import tile_labels
    h, w, P, S, d = 160, 192, 32, 32, 16
    truth = np.full((h // d, w // d), -1, np.int32)
    truth[0:3, 0:4] = 2
    truth[3:, 6:] = 4
    # centres (y + 16, x + 16): (0, 0) -> cell (1, 1); (32, 48) -> the centre pixel (48, 64) sits ON the border of cells 2|3 and 3|4
    # and belongs to the cell that starts there: (3, 4), unlabelled; (40, 80) -> (56, 96) -> cell (3, 6)
    o = np.array([[0, 0], [32, 48], [40, 80], [128, 160], [16, 40]], np.int32)
    emb = _emb(o, h, w, P, S)
    assert tile_labels(emb, truth, d).tolist() == [2, -1, 4, 4, 2]
    assert tile_labels(emb, torch.from_numpy(truth), d).dtype == np.int32
    with pytest.raises(ValueError):
        tile_labels(emb, truth[:-1], d)
    # a map that h // d cuts short of the last tile's centre: that tile is unlabelled, not an index error
    emb2 = _emb(np.array([[0, 0], [111, 0]], np.int32), 143, 64, 32, 32)     # centre row 127 lies past the 2 x 48 rows of the map
    assert tile_labels(emb2, np.zeros((143 // 48, 64 // 48), np.int32), 48).tolist() == [0, -1]


# ---- files ------------------------------------------------------------------------------------------------------------
def test_slide_embeddings_npz_round_trip(built_lib, tmp_path):
    from deephisto_amd.embeddings import SlideEmbeddings
    from oracle import tiling
    h, w, P, S = 300, 420, 96, 64
    o = tiling.tile_origins(h, w, P, S)
    for logits in (False, True):
        emb = _emb(o, h, w, P, S, D=128, logits=logits, layer=2, arch="resnet50", compute_dtype="bf16", n_padded=len(o) + 3)
        path = tmp_path / f"emb{int(logits)}.npz"
        emb.save(path)
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == {"features", "origins", "tile_index", "meta"} | ({"logits"} if logits else set())
            assert z["meta"].dtype.kind == "U"
        got = SlideEmbeddings.load(path)
        assert torch.equal(got.features, emb.features) and np.array_equal(got.origins, o) and got.origins.dtype == np.int32
        assert np.array_equal(got.tile_index, emb.tile_index) and got.tile_index.dtype == np.int64
        assert (got.logits is None) == (not logits) and (not logits or torch.equal(got.logits, emb.logits))
        for k in ("patch_size", "stride", "h", "w", "layer", "arch", "compute_dtype", "n_unique", "n_padded"):
            assert getattr(got, k) == getattr(emb, k), k
        assert got.n_unique == len(o) and got.n_padded == len(o) + 3 and got.width == 128
    with pytest.raises(ValueError, match="return_logits"):
        SlideEmbeddings.load(tmp_path / "emb0.npz").class_map()
    np.savez(tmp_path / "other.npz", meta=np.array("{}"))
    with pytest.raises(ValueError):
        SlideEmbeddings.load(tmp_path / "other.npz")


def test_prototype_classifier_npz_round_trip(built_lib, tmp_path):
    from deephisto_amd.embeddings import PrototypeClassifier
    pc = PrototypeClassifier(4, normalize=False, scale=2.5)
    with pytest.raises(ValueError):
        pc.save(tmp_path / "none.npz")
    with pytest.raises(ValueError):
        pc.scores(torch.zeros((1, 64)))
    pc.prototypes = torch.arange(4 * 64, dtype=torch.float32).reshape(4, 64)
    pc.counts, pc.empty_classes = np.array([3, 0, 9, 1]), [1]
    pc.save(tmp_path / "pc.npz")
    with np.load(tmp_path / "pc.npz", allow_pickle=False) as z:
        assert set(z.files) == {"prototypes", "counts", "meta"}
    got = PrototypeClassifier.load(tmp_path / "pc.npz")
    assert (got.n_classes, got.normalize, got.scale, got.empty_classes) == (4, False, 2.5, [1])
    assert torch.equal(got.prototypes, pc.prototypes) and got.counts.tolist() == [3, 0, 9, 1]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            PrototypeClassifier(bad)


@pytest.mark.parametrize("h,w,P,S,B,n_unique,n_padded", [(700, 900, 96, 64, 16, 154, 160), (700, 900, 96, 64, 11, 154, 154)])
def test_grid_rebuilt_from_stored_geometry_is_the_samplers_padded_list(built_lib, h, w, P, S, B, n_unique, n_padded):
    from deephisto_amd import tiles
    from deephisto_amd.plan import TileGrid
    want, n_u = tiles.tile_grid(h, w, P, S, B)
    assert (n_u, len(want)) == (n_unique, n_padded)
    grid = TileGrid.from_geometry(h, w, P, S, n_unique, n_padded)
    assert (grid.n_unique, grid.patch_size, grid.h, grid.w) == (n_unique, P, h, w)
    assert grid.origins.dtype == np.int32 and np.array_equal(grid.origins, want)
    with pytest.raises(ValueError, match="does not reproduce the tile grid"):
        TileGrid.from_geometry(h, w, P, S, n_unique - 1, n_padded)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_extract_embeddings_refuses_what_is_out_of_scope(built_lib):
    from deephisto_amd.embeddings import extract_embeddings
    from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler, FullImageRndSampler
    from deephisto_amd.stain import StainNormalizer
    from oracle import synth

    class Streamed(FullImageDenseSampler):
        resident = property(lambda self: False)

    host = synth.synth_slide(200, 260, 1)
    dense = FullImageDenseSampler(host, layer=1, patch_size=64, batch_size=4, stride=64, device="cpu")
    streamed = Streamed(host, layer=1, patch_size=64, batch_size=4, stride=64, device="cpu")
    rnd = object.__new__(FullImageRndSampler)
    model = object()
    with pytest.raises(ValueError, match="resident"):
        extract_embeddings(streamed, model)
    with pytest.raises(ValueError, match="resident"):
        extract_embeddings(streamed, model, stain=StainNormalizer("macenko"))
    with pytest.raises(ValueError, match="dense sampler"):
        extract_embeddings(rnd, model)
    with pytest.raises(ValueError, match="test-time augmentation"):
        extract_embeddings(dense, model, tta="d4")
    with pytest.raises(ValueError, match="ResNet18HIP or ResNet50HIP"):
        extract_embeddings(dense, model)


@pytest.mark.parametrize("other", [["--random_sampler"], ["--ondisk"], ["--tta", "flips"], ["--proba"]])
@pytest.mark.parametrize("flag", ["--save_embeddings", "--prototypes"])
def test_cli_refuses_embeddings_off_the_dense_resident_route(built_lib, tmp_path, capsys, flag, other):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    (tmp_path / "x.npz").write_bytes(b"")
    args = ap.parse_args(["--synthetic", "300", "300", "--weights", "", flag, str(tmp_path / "x.npz"), *other])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert flag in capsys.readouterr().err


def test_cli_prototypes_without_anno_needs_the_file(built_lib, tmp_path, capsys):
    from deephisto_amd.examples.predict_full_patched import _build_parser, _check_args
    ap = _build_parser()
    args = ap.parse_args(["--synthetic", "300", "300", "--weights", "", "--prototypes", str(tmp_path / "missing.npz")])
    with pytest.raises(SystemExit):
        _check_args(ap, args)
    assert "no such file" in capsys.readouterr().err


def test_bad_dims_are_refused_by_name_before_any_gpu_call(built_lib):
    """D and K outside the limits come back as DH_EINVAL with the argument's name, from null pointers: no GPU call was made."""
    err = lambda: built_lib.dh_last_error().decode()   # noqa: E731
    for D in (0, 32, 100, 4160, 8192, -64):
        assert built_lib.dh_embed_normalize(None, 4, D, None, None) == -22 and f"D = {D}" in err()
        assert built_lib.dh_embed_scores(None, 4, D, None, 5, 1.0, None, None) == -22 and f"D = {D}" in err()
        assert built_lib.dh_embed_class_sums(None, None, 4, D, 5, None, None, None, None) == -22 and f"D = {D}" in err()
        assert built_lib.dh_embed_class_work_size(4, D, 5) == -1 and f"D = {D}" in err()
    for K in (0, 65, -1):
        assert built_lib.dh_embed_scores(None, 4, 512, None, K, 1.0, None, None) == -22 and f"K = {K}" in err()
        assert built_lib.dh_embed_class_sums(None, None, 4, 512, K, None, None, None, None) == -22 and f"K = {K}" in err()
        assert built_lib.dh_embed_class_work_size(4, 512, K) == -1 and f"K = {K}" in err()
    assert built_lib.dh_embed_scores(None, -1, 512, None, 5, 1.0, None, None) == -22 and "n = -1" in err()
    # good dimensions, null pointers: still refused on the host; n = 0 needs none
    assert built_lib.dh_embed_normalize(None, 4, 512, None, None) == -22 and "null" in err()
    assert built_lib.dh_embed_scores(None, 4, 512, None, 5, 1.0, None, None) == -22 and "null" in err()
    assert built_lib.dh_embed_class_sums(None, None, 4, 512, 5, None, None, None, None) == -22 and "null" in err()
    assert built_lib.dh_embed_normalize(None, 0, 512, None, None) == 0
    assert built_lib.dh_embed_scores(None, 0, 512, None, 5, 1.0, None, None) == 0
    misaligned = C.c_void_p(4)
    assert built_lib.dh_embed_scores(misaligned, 4, 512, misaligned, 5, 1.0, misaligned, None) == -22 and "aligned" in err()
    # the work size: partials [chunks][K][D] and the chunk counts behind them
    assert built_lib.dh_embed_class_work_size(1, 64, 1) == 65
    assert built_lib.dh_embed_class_work_size(er.CHUNK_ROWS + 1, 512, 5) == 2 * 5 * 513
    from deephisto_amd import embeddings
    assert embeddings.CHUNK_ROWS == er.CHUNK_ROWS
    header = (Path(__file__).resolve().parents[1] / "include" / "deephisto_hip.h").read_text()
    assert f"#define DH_EMBED_CHUNK_ROWS {er.CHUNK_ROWS}\n" in header


def test_features_entries_check_arguments_like_forward_tiles(built_lib):
    """Null handle / unfinalized network / bad patch / too many tiles: refused on the host, as the forward_tiles siblings refuse them."""
    err = lambda: built_lib.dh_last_error().decode()   # noqa: E731
    h18, h50 = C.c_void_p(), C.c_void_p()
    assert built_lib.dh_resnet18_create(C.byref(h18), 5, 1) == 0 and built_lib.dh_resnet50_create(C.byref(h50), 5) == 0
    try:
        one = C.c_void_p(16)
        assert built_lib.dh_resnet18_features_tiles(None, one, 300, 300, one, 4, 96, one, None, None) == -22
        assert built_lib.dh_resnet18_features_tiles(h18, one, 300, 300, one, 4, 96, one, None, None) == -22 and "finalize" in err()
        assert built_lib.dh_resnet18_features_tiles(h18, one, 300, 300, one, 4, 96, None, one, None) == -22
        assert built_lib.dh_resnet50_features_tiles(None, one, 300, 300, one, 4, 96, one, None, None) == -22
        assert built_lib.dh_resnet50_features_tiles(h50, one, 300, 300, one, 4, 96, one, None, None) == -22 and "finalize" in err()
    finally:
        built_lib.dh_resnet18_destroy(h18)
        built_lib.dh_resnet50_destroy(h50)


# ---- the exchange of feature rows -------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _toy_rows(tile_index, D=512):
    t = tile_index.astype(np.float64)[:, None]
    return np.sin(t * 0.37 + np.arange(D)[None, :] * 0.011).astype(np.float32)


def _kept_list(n_unique):
    return np.nonzero(np.random.default_rng(n_unique).random(n_unique) < 0.6)[0].astype(np.int64)


def _worker(rank, world, port, n_unique, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deephisto_amd.predict import exchange_logits, shard_range
    kept = _kept_list(n_unique)
    n_work = len(kept)
    lo, hi = shard_range(n_work, world, rank)
    local = torch.zeros((-(-n_work // world), 512))
    local[:hi - lo] = torch.from_numpy(_toy_rows(kept[lo:hi]))
    full = exchange_logits(local, n_work)
    q.put((rank, lo, hi, full.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_ragged_shards_of_feature_rows_come_back_in_tile_order():
    """Two gloo ranks, a kept list of odd length: the one exchange the embeddings use returns the 512-wide rows of the kept tiles in
    tile order on both ranks."""
    n_unique, world, port = 131, 2, _free_port()
    kept = _kept_list(n_unique)
    assert len(kept) % 2 == 1, "the shards must be ragged"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_unique, q)) for r in range(world)]
    [p.start() for p in procs]
    got = [q.get(timeout=120) for _ in range(world)]
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    want = _toy_rows(kept)
    spans = sorted((lo, hi) for _, lo, hi, _ in got)
    assert spans[0][0] == 0 and spans[0][1] == spans[1][0] and spans[1][1] == len(kept) and spans[0][1] - spans[0][0] != spans[1][1] - spans[1][0]
    for _, _, _, full in got:
        assert full.shape == want.shape and np.array_equal(full, want)
