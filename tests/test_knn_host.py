"""The nearest-neighbour layer without a GPU (deephisto_amd/neighbours.py): the host's list surgery, the
vote rule of the reference, the classifier's argument checks and its file format, and the two entries' names and refusals."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import knn_ref as kr  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
INF = np.inf


# ---- drop_self ----------------------------------------------------------------------------------------------------------
HAND_INDEX = np.array([[7, 3, 9, 4],      # own index first
                       [3, 8, 5, 1],      # own index in the middle
                       [2, 6, 0, 11],     # own index absent: the last entry goes
                       [4, 9, -1, -1],    # padding present, own index held
                       [6, -1, -1, -1]],  # padding present, own index absent
                      dtype=np.int32)
HAND_DIST = np.array([[0.0, 1.0, 2.0, 3.0],
                      [0.5, 0.5, 0.5, 2.0],
                      [1.0, 2.0, 3.0, 4.0],
                      [0.0, 0.25, INF, INF],
                      [1.5, INF, INF, INF]], dtype=np.float32)
HAND_OWN = np.array([7, 5, 10, 4, 2], dtype=np.int32)
WANT_INDEX = np.array([[3, 9, 4], [3, 8, 1], [2, 6, 0], [9, -1, -1], [6, -1, -1]], dtype=np.int32)
WANT_DIST = np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 2.0], [1.0, 2.0, 3.0], [0.25, INF, INF], [1.5, INF, INF]], dtype=np.float32)


def test_drop_self_on_hand_made_rows():
    from deephisto_amd.neighbours import drop_self
    index, dist = drop_self(HAND_INDEX, HAND_DIST, HAND_OWN)
    assert isinstance(index, np.ndarray) and index.dtype == np.int32 and dist.dtype == np.float32
    assert np.array_equal(index, WANT_INDEX) and np.array_equal(dist, WANT_DIST)
    ti, td = drop_self(torch.from_numpy(HAND_INDEX), torch.from_numpy(HAND_DIST), torch.from_numpy(HAND_OWN))
    assert ti.dtype == torch.int32 and td.dtype == torch.float32
    assert np.array_equal(ti.numpy(), WANT_INDEX) and np.array_equal(td.numpy(), WANT_DIST)
    ti, _ = drop_self(torch.from_numpy(HAND_INDEX), torch.from_numpy(HAND_DIST), HAND_OWN.tolist())   # own as a plain list
    assert np.array_equal(ti.numpy(), WANT_INDEX)
    one_i, one_d = drop_self(HAND_INDEX[:, :1], HAND_DIST[:, :1], HAND_OWN)   # k + 1 = 1: nothing is left
    assert one_i.shape == (5, 0) and one_d.shape == (5, 0)
    with pytest.raises(ValueError, match="do not fit"):
        drop_self(HAND_INDEX, HAND_DIST[:, :3], HAND_OWN)
    with pytest.raises(ValueError, match="do not fit"):
        drop_self(HAND_INDEX, HAND_DIST, HAND_OWN[:4])


# ---- the vote rule --------------------------------------------------------------------------------------------------------
def test_votes_ref_on_hand_cases_of_the_tie_rule():
    labels = np.array([0, 0, 1, 1, 2, -1, 7], dtype=np.int32)   # bank rows 5 and 6 cast no vote among 3 classes
    index = np.array([[0, 2, 3],        # 1 x class 0, 2 x class 1: class 1
                      [2, 0, 4],        # one each: the first in the list, class 1
                      [4, 2, 0],        # one each: class 2
                      [0, 2, 3, ][::-1],   # 3, 2, 0: class 1 twice
                      [5, 6, -1],       # nobody votes
                      [5, 4, 9],        # 9 is outside the bank: class 2 alone
                      [2, 0, 1],        # class 1 first, class 0 twice: the count decides, class 0
                      [0, 2, -1]],      # a tie ahead of the padding: class 0
                     dtype=np.int32)
    votes, label = kr.votes_ref(index, labels, 3)
    assert label.tolist() == [1, 1, 2, 1, -1, 2, 0, 0]
    assert votes.tolist() == [[1, 2, 0], [1, 1, 1], [1, 1, 1], [1, 2, 0], [0, 0, 0], [0, 0, 1], [2, 1, 0], [1, 1, 0]]
    assert votes.dtype == np.int32 and label.dtype == np.int32
    # two against two: the class of the nearest neighbour
    votes, label = kr.votes_ref(np.array([[2, 0, 1, 3]]), labels, 2)
    assert votes.tolist() == [[2, 2]] and label.tolist() == [1]
    votes, label = kr.votes_ref(np.array([[4, 4, 4]]), labels, 2)   # class 2 is not one of two classes
    assert votes.tolist() == [[0, 0]] and label.tolist() == [-1]


def test_topk_ref_and_check_knn_agree_on_a_small_case():
    rng = np.random.default_rng(3)
    q, b = rng.standard_normal((6, 64)).astype(np.float32), rng.standard_normal((9, 64)).astype(np.float32)
    b[4] = b[2]          # a pair of duplicates
    b[7, 5] = np.nan     # a row that never enters
    d64 = kr.assign_ref(q, b)
    index, dist = kr.topk_ref(d64.astype(np.float32), 12, m0=100)
    kr.check_knn(d64, index, dist, 64, 12, m0=100)
    assert np.all(index[:, 8:] == -1) and np.all(np.isposinf(dist[:, 8:])) and not np.any(index == 107)
    for i in range(6):   # the duplicates sit next to each other, lower index first
        p = int(np.flatnonzero(index[i] == 102)[0])
        assert index[i, p + 1] == 104 and dist[i, p] == dist[i, p + 1]
    swapped = index.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    with pytest.raises(AssertionError):
        kr.check_knn(d64, swapped, dist, 64, 12, m0=100)


# ---- the classifier -------------------------------------------------------------------------------------------------------
def test_knn_classifier_argument_checks(built_lib):
    from deephisto_amd.embeddings import SlideEmbeddings
    from deephisto_amd.neighbours import KNNClassifier, nearest_rows, similar_tiles, tile_at
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_classes must be in"):
            KNNClassifier(bad)
        with pytest.raises(ValueError, match="k must be in"):
            KNNClassifier(4, k=bad)
    knn = KNNClassifier(4)
    assert (knn.n_classes, knn.k, knn.normalize, knn.bank) == (4, 5, True, None)
    with pytest.raises(ValueError, match="no bank to save"):
        knn.save("nowhere.npz")
    with pytest.raises(ValueError, match="needs a fitted bank"):
        knn.leave_one_out()
    with pytest.raises(RuntimeError, match="must live in GPU memory"):
        knn.fit(torch.zeros((3, 64)), [0, 1, 2])
    with pytest.raises(RuntimeError, match="must live in GPU memory"):
        nearest_rows(torch.zeros((3, 64)), torch.zeros((3, 64)), 2)
    with pytest.raises(ValueError, match="an empty list"):
        knn.fit([], [])
    emb = SlideEmbeddings(torch.zeros((4, 64)), [[0, 0], [0, 64], [64, 0], [64, 64]], np.arange(4), patch_size=96, stride=64,
                          h=160, w=160, n_unique=4, row_range=(0, 4))
    with pytest.raises(ValueError, match="one rank's rows only"):
        knn.fit(emb, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="one rank's rows only"):
        similar_tiles(emb, 0)
    # a pixel goes to the first tile whose footprint holds it
    assert [tile_at(emb, q) for q in (2, (0, 0), (70, 10), (70, 70), (159, 159), (95, 64))] == [2, 0, 0, 0, 3, 0]
    for bad in (4, -1, (160, 0), (0, 200)):
        with pytest.raises(ValueError, match="tiles|covers"):
            tile_at(emb, bad)


def test_knn_classifier_npz_round_trip(tmp_path):
    from deephisto_amd.embeddings import PrototypeClassifier
    from deephisto_amd.neighbours import KNNClassifier
    rng = np.random.default_rng(8)
    knn = KNNClassifier(5, k=7, normalize=False)
    knn.bank = torch.from_numpy(rng.standard_normal((11, 64)).astype(np.float32))
    knn.labels = torch.from_numpy(rng.integers(0, 5, 11).astype(np.int32))
    knn.counts = np.bincount(knn.labels.numpy(), minlength=5).astype(np.int64)
    path = tmp_path / "bank.npz"
    knn.save(path)
    with np.load(path, allow_pickle=False) as z:   # nothing pickled
        assert sorted(z.files) == ["bank", "counts", "labels", "meta"] and '"deephisto_amd.KNNClassifier/1"' in str(z["meta"])
    back = KNNClassifier.load(path)
    assert (back.n_classes, back.k, back.normalize) == (5, 7, False)
    assert torch.equal(back.bank, knn.bank) and torch.equal(back.labels, knn.labels) and back.labels.dtype == torch.int32
    assert np.array_equal(back.counts, knn.counts) and back.counts.dtype == np.int64
    pc = PrototypeClassifier(5)
    pc.prototypes, pc.counts = torch.zeros((5, 64)), np.zeros(5, np.int64)
    pc.save(tmp_path / "protos.npz")
    with pytest.raises(ValueError, match="not a KNNClassifier file"):
        KNNClassifier.load(tmp_path / "protos.npz")


# ---- the entries ----------------------------------------------------------------------------------------------------------
def test_header_and_signatures_name_the_two_entries(built_lib):
    from deephisto_amd import _lib
    header = (REPO / "include" / "deephisto_hip.h").read_text()
    for name in ("dh_embed_knn", "dh_embed_knn_votes"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(built_lib, name)
    assert len(_lib.SIGNATURES["dh_embed_knn"][1]) == 11 and len(_lib.SIGNATURES["dh_embed_knn_votes"][1]) == 9


def test_bad_arguments_are_refused_by_name_before_any_gpu_call(built_lib):
    knn, votes, err = built_lib.dh_embed_knn, built_lib.dh_embed_knn_votes, built_lib.dh_last_error
    p = C.c_void_p(4096)
    for args, what in (((p, 4, p, 4, 96, 1, 0, 0, p, p, None), b"D = 96"),
                       ((p, 4, p, 4, 64, 0, 0, 0, p, p, None), b"k = 0"),
                       ((p, 4, p, 4, 64, 65, 0, 0, p, p, None), b"k = 65"),
                       ((p, -1, p, 4, 64, 1, 0, 0, p, p, None), b"n = -1"),
                       ((p, 4, p, -1, 64, 1, 0, 0, p, p, None), b"m = -1"),
                       ((p, 4, p, 4, 64, 1, -1, 0, p, p, None), b"m0 + m"),
                       ((p, 4, p, 4, 64, 1, 2 ** 31 - 4, 0, p, p, None), b"m0 + m"),
                       ((None, 4, p, 4, 64, 1, 0, 0, p, p, None), b"null query_dev"),
                       ((p, 4, None, 4, 64, 1, 0, 0, p, p, None), b"null query_dev"),
                       ((p, 4, p, 4, 64, 1, 0, 0, None, p, None), b"null query_dev"),
                       ((p, 4, p, 4, 64, 1, 0, 0, p, None, None), b"null query_dev"),
                       ((C.c_void_p(4100), 4, p, 4, 64, 1, 0, 0, p, p, None), b"not 16-byte aligned"),
                       ((p, 4, C.c_void_p(4104), 4, 64, 1, 0, 0, p, p, None), b"not 16-byte aligned"),
                       ((p, 4, p, 4, 64, 1, 0, 0, C.c_void_p(4098), p, None), b"not 4-byte aligned"),
                       ((p, 4, p, 4, 64, 1, 0, 0, p, C.c_void_p(4097), None), b"not 4-byte aligned")):
        assert knn(*args) == -22 and b"dh_embed_knn:" in err() and what in err(), (args, err())
    assert knn(None, 0, None, 0, 64, 1, 0, 0, None, None, None) == 0           # n == 0: a no-op that needs no pointer
    assert knn(p, 4, None, 0, 64, 1, 2 ** 31 - 1, 1, p, p, None) == 0          # m == 0 with merge changes nothing
    for args, what in (((p, 4, 0, p, 4, 4, p, p, None), b"k = 0"),
                       ((p, 4, 65, p, 4, 4, p, p, None), b"k = 65"),
                       ((p, 4, 5, p, 4, 0, p, p, None), b"n_classes = 0"),
                       ((p, 4, 5, p, 4, 65, p, p, None), b"n_classes = 65"),
                       ((p, -1, 5, p, 4, 4, p, p, None), b"n = -1"),
                       ((p, 4, 5, p, -1, 4, p, p, None), b"m = -1"),
                       ((None, 4, 5, p, 4, 4, p, p, None), b"null index_dev"),
                       ((p, 4, 5, None, 4, 4, p, p, None), b"null index_dev"),
                       ((p, 4, 5, p, 4, 4, None, p, None), b"null index_dev"),
                       ((p, 4, 5, p, 4, 4, p, None, None), b"null index_dev"),
                       ((p, 4, 5, p, 4, 4, C.c_void_p(4098), p, None), b"not 4-byte aligned")):
        assert votes(*args) == -22 and b"dh_embed_knn_votes:" in err() and what in err(), (args, err())
    assert votes(None, 0, 5, None, 0, 4, None, None, None) == 0


def test_cli_refuses_bad_knn_flag_combinations(built_lib, tmp_path, capsys):
    from deephisto_amd.examples.predict_full_patched import main
    base = ["--synthetic", "300", "420", "--layer", "1", "--weights", "", "--patch_size", "96", "--stride", "64"]
    from deephisto_amd.neighbours import KNNClassifier
    bank = str(tmp_path / "bank.npz")
    for name, n_classes, width in (("three.npz", 3, 512), ("narrow.npz", 5, 64)):   # banks that do not fit 5 classes x 512 floats
        knn = KNNClassifier(n_classes)
        knn.bank, knn.labels, knn.counts = torch.zeros((2, width)), torch.zeros(2, dtype=torch.int32), np.zeros(n_classes, np.int64)
        knn.save(tmp_path / name)
    for extra, what in ((["--knn", "5"], "--knn needs --knn_bank"),
                        (["--knn", "5", "--knn_bank", str(tmp_path / "three.npz")], "3 classes x 512 floats do not fit"),
                        (["--knn", "5", "--knn_bank", str(tmp_path / "narrow.npz")], "5 classes x 64 floats do not fit"),
                        (["--knn_bank", bank], "--knn_bank needs --knn"),
                        (["--knn", "0", "--knn_bank", bank], "--knn must be in 1 .. 63"),
                        (["--knn", "64", "--knn_bank", bank], "--knn must be in 1 .. 63"),
                        (["--knn", "5", "--knn_bank", bank], "no such file"),
                        (["--knn_per_class", "10"], "--knn_per_class needs --knn"),
                        (["--knn", "5", "--knn_bank", bank, "--knn_per_class", "10"], "--knn_per_class caps a fit"),
                        (["--knn", "5", "--knn_bank", bank, "--tta", "d4"], "--knn"),
                        (["--knn", "5", "--knn_bank", bank, "--random_sampler"], "--knn"),
                        (["--similar_k", "4"], "--similar_k and --similar_json need --similar_to"),
                        (["--similar_json", "x.json"], "--similar_k and --similar_json need --similar_to"),
                        (["--similar_to", "12"], "--similar_to takes Y,X"),
                        (["--similar_to", "a,b"], "--similar_to takes Y,X"),
                        (["--similar_to", "300,10"], "outside the slide"),
                        (["--similar_to", "10,420"], "outside the slide"),
                        (["--similar_to=-1,10"], "outside the slide"),
                        (["--similar_to", "10,10", "--similar_k", "64"], "--similar_k must be in 1 .. 63"),
                        (["--similar_to", "10,10", "--fine"], "--similar_to")):
        with pytest.raises(SystemExit):
            main(base + ["--out_dir", str(tmp_path)] + extra)
        assert what in capsys.readouterr().err, extra
