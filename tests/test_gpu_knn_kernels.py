"""GPU: dh_embed_knn and dh_embed_knn_votes (deephisto_amd/neighbours.py) against tests/helpers/knn_ref.py.

The sweep against float64: n = 70 query rows (two workgroups of 64 rows, the second ragged), a bank of m in {1, 5, 64, 65, 200} rows (both
sides of the 64-row panel, fewer rows than k, more rows than k), D in {64, 192}, k in {1, 5, 64}, and one case at D = 2048.  Every
row is held to the float64 distances by the gate g = (D + 4) u of the distance's error model (knn_ref.check_knn); what must be
equal bit for bit (dh_embed_assign, passes with merge, the launch geometry, duplicates) is compared bit for bit."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import knn_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

N, M = 70, 200
INF = np.inf


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE: dict = {}


def _case(D, n=N, m=M):
    """(float32[n, D] queries, float32[m, D] bank, float64[n, m] distances): once per shape, never written."""
    if (D, n, m) not in _CACHE:
        rng = np.random.default_rng(7000 + D + n)
        q, b = rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((m, D)).astype(np.float32)
        d = kr.assign_ref(q, b)
        for a in (q, b, d):
            a.setflags(write=False)
        _CACHE[D, n, m] = (q, b, d)
    return _CACHE[D, n, m]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _same(a, b):
    """Two (index, dist) results are the same integers and the same float bits."""
    return torch.equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---- against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 64))
@pytest.mark.parametrize("m", (1, 5, 64, 65, 200))
@pytest.mark.parametrize("D", (64, 192))
def test_knn_against_float64(dev, D, m, k):
    from deephisto_amd.neighbours import nearest_rows
    q, b, d64 = _case(D)
    m0 = 1000 if k == 5 else 0
    index = torch.full((N + 1, k), -77, dtype=torch.int32, device=dev)
    dist = torch.full((N + 1, k), -5.0, dtype=torch.float32, device=dev)
    idx, dst = nearest_rows(_t(q, dev), _t(b[:m], dev), k, index[:N], dist[:N], m0=m0)
    kr.check_knn(d64[:, :m], idx.cpu().numpy(), dst.cpu().numpy(), D, k, m0)
    assert bool((index[N] == -77).all()) and bool((dist[N] == -5.0).all()), "the guard row behind n is untouched"
    if m < k:
        assert bool((idx[:, m:] == -1).all()) and bool(torch.isposinf(dst[:, m:]).all()) and bool((idx[:, :m] >= m0).all())
    assert _same(nearest_rows(_t(q, dev), _t(b[:m], dev), k, m0=m0), (idx, dst)), "a second launch gives the same bits"


def test_knn_against_float64_at_2048(dev):
    from deephisto_amd.neighbours import nearest_rows
    q, b, d64 = _case(2048, 33, 130)
    idx, dst = nearest_rows(_t(q, dev), _t(b, dev), 8)
    kr.check_knn(d64, idx.cpu().numpy(), dst.cpu().numpy(), 2048, 8)


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 5, 16, 17, 64))
def test_k1_is_dh_embed_assign(dev, m):
    from deephisto_amd.clustering import nearest_centres
    from deephisto_amd.neighbours import nearest_rows
    q, b, _ = _case(192)
    x, c = _t(q, dev), _t(b[:m], dev)
    lab, d1 = nearest_centres(x, c, k0=3)
    idx, dst = nearest_rows(x, c, 1, m0=3)
    assert torch.equal(idx[:, 0], lab) and np.array_equal(_bits(dst[:, 0]), _bits(d1))


def test_k1_is_dh_embed_assign_in_passes(dev):
    from deephisto_amd.clustering import nearest_centres
    from deephisto_amd.neighbours import nearest_rows
    q, b, _ = _case(64)
    x, c = _t(q, dev), _t(b, dev)
    lab = torch.empty(N, dtype=torch.int32, device=dev)
    d1 = torch.empty(N, dtype=torch.float32, device=dev)
    for k0 in range(0, M, 64):
        nearest_centres(x, c[k0:k0 + 64], lab, d1, k0=k0, merge=k0 > 0)
    idx, dst = nearest_rows(x, c, 1)
    assert torch.equal(idx[:, 0], lab) and np.array_equal(_bits(dst[:, 0]), _bits(d1))


@pytest.mark.parametrize("k", (1, 5, 16, 17, 64))     # 16 | 17: the two list capacities the kernel is built for
def test_passes_with_merge_are_the_single_call(dev, k):
    from deephisto_amd.neighbours import nearest_rows
    q, b, d64 = _case(192)
    x, c = _t(q, dev), _t(b, dev)
    whole = nearest_rows(x, c, k, m0=11)
    kr.check_knn(d64, whole[0].cpu().numpy(), whole[1].cpu().numpy(), 192, k, 11)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    dst = torch.empty((N, k), dtype=torch.float32, device=dev)
    for lo, hi in ((0, 64), (64, 128), (128, 200)):
        nearest_rows(x, c[lo:hi], k, idx, dst, m0=11 + lo, merge=lo > 0)
    assert _same((idx, dst), whole)
    for lo, hi in ((128, 200), (0, 64), (64, 128)):     # the order of the passes does not matter either
        nearest_rows(x, c[lo:hi], k, idx, dst, m0=11 + lo, merge=lo != 128)
    assert _same((idx, dst), whole)
    with pytest.raises(ValueError, match="merge"):
        nearest_rows(x, c, k, merge=True)


def test_indices_up_to_the_int32_limit(dev):
    from deephisto_amd.neighbours import nearest_rows
    q, b, _ = _case(64)
    x, c = _t(q, dev), _t(b, dev)
    low = nearest_rows(x, c, 5)
    m0 = 2 ** 31 - 1 - M
    high = nearest_rows(x, c, 5, m0=m0)
    assert np.array_equal(high[0].cpu().numpy().astype(np.int64), low[0].cpu().numpy().astype(np.int64) + m0)
    assert np.array_equal(_bits(high[1]), _bits(low[1]))


@pytest.mark.parametrize("D,k", ((64, 5), (64, 64), (2048, 8)))
def test_launch_independence(dev, D, k):
    """Rows 5..40 alone, one row alone, and the rows moved to another place in a longer matrix: the same k pairs."""
    from deephisto_amd.neighbours import nearest_rows
    q, b, _ = _case(D) if D == 64 else _case(D, 33, 130)
    n = len(q)
    x, c = _t(q, dev), _t(b, dev)
    whole = nearest_rows(x, c, k)
    part = nearest_rows(x[5:31], c, k)
    assert _same(part, (whole[0][5:31], whole[1][5:31]))
    one = nearest_rows(x[17:18], c, k)
    assert _same(one, (whole[0][17:18], whole[1][17:18]))
    longer = torch.cat([x[20:], x, x[:3]], dim=0).contiguous()
    moved = nearest_rows(longer, c, k)
    assert _same((moved[0][n - 20:2 * n - 20], moved[1][n - 20:2 * n - 20]), whole)
    assert _same((moved[0][:n - 20], moved[1][:n - 20]), (whole[0][20:], whole[1][20:]))


def test_duplicates_zero_distances_and_nan(dev):
    from deephisto_amd.neighbours import nearest_rows
    D, h, k = 64, 100, 9
    q, b, _ = _case(D)
    q, half = q.copy(), b[:h].copy()
    half[40] = np.nan                       # a NaN bank row (both of its copies) is never returned
    q[7] = half[12]                         # a query that is a bank row
    q[30] = np.nan                          # a NaN query row
    q[31, 3] = np.inf                       # every distance of this row is +inf
    bank = np.concatenate([half, half])     # every row twice: rows j and j + h
    idx, dst = nearest_rows(_t(q, dev), _t(bank, dev), k)
    idx, dst = idx.cpu().numpy(), dst.cpu().numpy()
    assert idx[7, 0] == 12 and idx[7, 1] == 12 + h and dst[7, 0] == 0.0 and dst[7, 1] == 0.0 and not np.signbit(dst[7, 0])
    for r in (30, 31):
        assert np.all(idx[r] == -1) and np.all(np.isposinf(dst[r])), "a row without a finite distance is all padding"
    ok = np.ones(N, bool)
    ok[[30, 31]] = False
    assert not np.isin(idx, (40, 40 + h)).any()
    for i in np.flatnonzero(ok):            # the two copies sit next to each other with equal distance bits, the lower index first
        for p in range(k):
            if idx[i, p] < h and p + 1 < k:
                assert idx[i, p + 1] == idx[i, p] + h and dst[i, p + 1].view(np.uint32) == dst[i, p].view(np.uint32)
            if idx[i, p] >= h:
                assert p > 0 and idx[i, p - 1] == idx[i, p] - h
    good = np.delete(np.arange(2 * h), (40, 40 + h))
    d64 = kr.assign_ref(q[ok], bank[good])
    remap = np.full(2 * h, -1)
    remap[good] = np.arange(len(good))
    kr.check_knn(d64, remap[idx[ok]], dst[ok], D, k)


def test_zero_sizes(dev):
    from deephisto_amd.neighbours import nearest_rows
    q, b, _ = _case(64)
    x, c = _t(q, dev), _t(b, dev)
    idx, dst = nearest_rows(x[:0], c, 4)
    assert idx.shape == (0, 4) and dst.shape == (0, 4)
    idx, dst = nearest_rows(x, c[:0], 4)                              # an empty bank fills the padding
    assert bool((idx == -1).all()) and bool(torch.isposinf(dst).all())
    held = nearest_rows(x, c[:9], 4)
    before = (held[0].clone(), held[1].clone())
    nearest_rows(x, c[:0], 4, held[0], held[1], m0=9, merge=True)      # an empty pass changes nothing
    assert _same(held, before)


# ---- refusals by name -------------------------------------------------------------------------------------------------------
def _raw(built_lib, dev, D=64, k=3, m=4, m0=0, query="ok", bank="ok", index="ok", dist="ok", n=4):
    x = torch.zeros((n + 1, max(D, 64)), dtype=torch.float32, device=dev)
    c = torch.zeros((8, max(D, 64)), dtype=torch.float32, device=dev)
    ix = torch.zeros((n + 1, 64), dtype=torch.int32, device=dev)
    ds = torch.zeros((n + 1, 64), dtype=torch.float32, device=dev)
    ptr = {"ok": lambda t: t.data_ptr(), "null": lambda t: None, "odd": lambda t: t.data_ptr() + 4, "odd1": lambda t: t.data_ptr() + 2}
    rc = built_lib.dh_embed_knn(ptr[query](x), n, ptr[bank](c), m, D, k, m0, 0, ptr[index](ix), ptr[dist](ds), None)
    torch.cuda.synchronize()
    assert not ix.any() and not ds.any(), "a refused call launches nothing"
    return rc, built_lib.dh_last_error().decode()


@pytest.mark.parametrize("kw,what", (
    (dict(D=96), "D = 96"), (dict(D=32), "D = 32"), (dict(D=4160), "D = 4160"), (dict(k=0), "k = 0"), (dict(k=65), "k = 65"),
    (dict(m=-1), "m = -1"), (dict(n=-1), "n = -1"), (dict(m0=-1), "m0 + m"), (dict(m0=2 ** 31 - 4), "m0 + m"),
    (dict(query="null"), "null"), (dict(bank="null"), "null"), (dict(index="null"), "null"), (dict(dist="null"), "null"),
    (dict(query="odd"), "16-byte aligned"), (dict(bank="odd"), "16-byte aligned"),
    (dict(index="odd1"), "4-byte aligned"), (dict(dist="odd1"), "4-byte aligned")))
def test_refuses_by_name(built_lib, dev, kw, what):
    rc, msg = _raw(built_lib, dev, **kw)
    assert rc == -22 and "dh_embed_knn:" in msg and what in msg


# ---- the votes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 4, 64))
@pytest.mark.parametrize("k", (1, 5, 8))
def test_votes_are_the_reference_bit_for_bit(dev, k, C):
    from deephisto_amd.neighbours import neighbour_votes
    n, m = 1030, 300
    rng = np.random.default_rng(100 * k + C)
    index = rng.integers(-1, m + 20, (n, k)).astype(np.int32)            # -1 and indices past the bank among them
    index[5] = -1
    labels = rng.integers(-1, C + 2, m).astype(np.int32)                 # -1 and labels past the classes among them
    got_v, got_l = neighbour_votes(_t(index, dev), _t(labels, dev), C)
    want_v, want_l = kr.votes_ref(index, labels, C)
    assert got_v.dtype == torch.int32 and got_l.dtype == torch.int32
    assert np.array_equal(got_v.cpu().numpy(), want_v) and np.array_equal(got_l.cpu().numpy(), want_l)
    assert want_l[5] == -1 and (want_v.sum(1) <= k).all() and (want_l >= 0).sum() > n // 8, "the case does vote, and not always"


def test_votes_refusals_by_name(built_lib, dev):
    ix = torch.zeros((4, 5), dtype=torch.int32, device=dev)
    lb = torch.zeros(6, dtype=torch.int32, device=dev)
    vt = torch.zeros((4, 64), dtype=torch.int32, device=dev)
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    for args, what in (((p(ix), 4, 0, p(lb), 6, 4, p(vt), p(out), None), "k = 0"),
                       ((p(ix), 4, 65, p(lb), 6, 4, p(vt), p(out), None), "k = 65"),
                       ((p(ix), 4, 5, p(lb), 6, 0, p(vt), p(out), None), "n_classes = 0"),
                       ((p(ix), 4, 5, p(lb), 6, 65, p(vt), p(out), None), "n_classes = 65"),
                       ((p(ix), 4, 5, p(lb), -1, 4, p(vt), p(out), None), "m = -1"),
                       ((None, 4, 5, p(lb), 6, 4, p(vt), p(out), None), "null"),
                       ((p(ix), 4, 5, p(lb), 6, 4, p(vt), p(out) + 2, None), "4-byte aligned")):
        assert built_lib.dh_embed_knn_votes(*args) == -22
        msg = built_lib.dh_last_error().decode()
        assert "dh_embed_knn_votes:" in msg and what in msg
