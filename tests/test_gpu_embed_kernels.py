"""GPU: the three embedding kernels (deephisto_amd/csrc/embed.hip) against tests/helpers/embed_ref.py.

Seeded normal matrices with one all-zero row and one row with a single non-zero (n >= 3).  D in {64, 512, 2048}, K in {1, 5, 64},
n in {1, 63, 65, 1025, 2049}: a wave, a workgroup's 32-row tile and two borders of the 1024-row chunks are straddled."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import embed_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

DS, KS, NS = (64, 512, 2048), (1, 5, 64), (1, 63, 65, 1025, 2049)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE: dict = {}


def _features(n, D):
    """float32[n, D], the same for every test that asks (computed once and never written)."""
    if (n, D) not in _CACHE:
        f = np.random.default_rng(1000 * D + n).standard_normal((n, D)).astype(np.float32)
        if n >= 3:
            f[n // 2] = 0
            f[n - 1] = 0
            f[n - 1, D // 3] = 1.75
        f.setflags(write=False)
        _CACHE[n, D] = f
    return _CACHE[n, D]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_normalize(dev, D, n):
    from deephisto_amd.embeddings import normalize_rows
    f = _features(n, D)
    x = torch.from_numpy(f).to(dev)
    guard = torch.full((n + 1, D), 7.0, dtype=torch.float32, device=dev)
    out = normalize_rows(x, out=guard[:n])
    want = er.normalize_ref(f)
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert np.all(err <= er.normalize_bound(D) * np.abs(want)), f"max {np.max(err[want != 0] / np.abs(want[want != 0])) / er.U:.2f} u"
    assert torch.all(guard[n] == 7.0)
    if n >= 3:
        assert not got[n // 2].any(), "the zero row stays zero"
        assert got[n - 1, D // 3] == 1.0 and np.count_nonzero(got[n - 1]) == 1
    inplace = x.clone()
    assert normalize_rows(inplace, out=inplace) is inplace
    assert np.array_equal(_bits(inplace), _bits(out)), "in place equals out of place"
    if n > 8:   # a row's result depends on that row alone
        assert np.array_equal(_bits(normalize_rows(x[7:])), _bits(out[7:]))
        assert np.array_equal(_bits(normalize_rows(x[n - 1:])), _bits(out[n - 1:]))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_scores(dev, D, K, n):
    from deephisto_amd.embeddings import prototype_scores
    f = _features(n, D)
    p = np.random.default_rng(7 * D + K).standard_normal((K, D)).astype(np.float32)
    scale = -1.5 if K == 5 else 1.0 if K == 1 else 0.125
    x, pd = torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev)
    got_t = prototype_scores(x, pd, scale)
    assert got_t.shape == (n, K)
    want, bound = er.scores_ref(f, p, scale)
    err = np.abs(got_t.cpu().numpy().astype(np.float64) - want)
    assert np.all(err <= bound), f"max err / bound = {np.max(err[bound > 0] / bound[bound > 0]):.4f}"
    if n >= 3:
        assert not got_t[n // 2].any()
    # row-invariance: alone, inside the full launch, at a shifted offset
    for i in sorted({0, n // 2, n - 1}):
        assert np.array_equal(_bits(prototype_scores(x[i:i + 1], pd, scale)), _bits(got_t[i:i + 1])), f"row {i} alone"
    for s in (7, 33):
        if n > s:
            assert np.array_equal(_bits(prototype_scores(x[s:], pd, scale)), _bits(got_t[s:])), f"shifted by {s}"
    assert np.array_equal(_bits(prototype_scores(x, pd, scale)), _bits(got_t))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_class_sums(dev, D, K, n):
    from deephisto_amd.embeddings import class_sums
    f = _features(n, D)
    x = torch.from_numpy(f).to(dev)
    rng = np.random.default_rng(n + K)
    lab = rng.integers(-1, K + 1, n).astype(np.int32)        # -1 and K are ignored
    if K >= 3:
        lab[lab == 1] = -1                                     # one class left empty
    want, counts = er.class_sums_ref(f, lab, K)
    got, cnt = class_sums(x, lab, K)
    assert cnt.dtype == torch.int64 and cnt.cpu().numpy().tolist() == counts.tolist()
    assert np.array_equal(_bits(got), want.view(np.uint32)), f"{int((_bits(got) != want.view(np.uint32)).sum())} elements differ"
    if K >= 3:
        assert counts[1] == 0 and not got[1].any()
    again, cnt2 = class_sums(x, torch.from_numpy(lab).to(dev), K)
    assert np.array_equal(_bits(again), _bits(got)) and torch.equal(cnt2, cnt)
    # all rows in one class (the last)
    one = np.full(n, K - 1, np.int32)
    want1, counts1 = er.class_sums_ref(f, one, K)
    got1, cnt1 = class_sums(x, one, K)
    assert cnt1.cpu().numpy().tolist() == counts1.tolist() and counts1[K - 1] == n
    assert np.array_equal(_bits(got1), want1.view(np.uint32))


def test_prototype_classifier_on_the_kernels(dev):
    """fit / scores through the three kernels against the float64 pipeline, an empty class listed, scores of a zero prototype 0."""
    from deephisto_amd.embeddings import PrototypeClassifier
    n, D, K = 1025, 512, 5
    f = np.abs(_features(n, D))
    lab = np.random.default_rng(0).integers(-1, K, n).astype(np.int32)
    lab[lab == 2] = -1
    pc = PrototypeClassifier(K).fit(torch.from_numpy(f).to(dev), lab)
    assert pc.empty_classes == [2] and pc.counts.tolist() == [int((lab == k).sum()) for k in range(K)]
    x = er.normalize_ref(f)
    mean = np.stack([x[lab == k].sum(0) / max(1, (lab == k).sum()) for k in range(K)])
    proto = er.normalize_ref(mean)
    assert np.allclose(pc.prototypes.cpu().numpy(), proto, rtol=0, atol=(D + 4) * er.U * 4)
    sc = pc.scores(torch.from_numpy(f).to(dev)).cpu().numpy()
    want, bound = er.scores_ref(x, proto, 1.0)
    assert np.all(np.abs(sc - want) <= bound + 8 * (D + 4) * er.U)     # + the two normalisations and the class mean ahead of the scores
    assert not sc[:, 2].any()
