"""Host planner of FullImageRndSampler's device index logic (deephisto_amd/coverage.py).  CPU only.

The planner replaces the reference's per-batch whole-map NumPy work (full_samplers.py:105-153) by rank-space
arithmetic: S(m) in closed form, `np.random.choice(replace=False, p)` emulated on ranks, the RNG consumed in the
reference's order.  Everything here is checked against NumPy itself and against oracle/random_sampler.py, driven
by a NumPy stand-in for the device map."""
import numpy as np
import pytest

from deephisto_amd import coverage as cv
from oracle import random_sampler


def test_s_segments_equal_sequential_cumsum_small_n():
    for n in range(1, 20001):
        seg = cv.SSegments(n)
        want = np.cumsum(np.full(n, 1.0 / n))
        got = seg(np.arange(1, n + 1))
        assert np.array_equal(got, want), n
        assert seg(0) == 0.0


def test_s_segments_equal_sequential_cumsum_large_n():
    rs = np.random.RandomState(1)
    ns = sorted(set(rs.randint(20001, 10 ** 7, size=22).tolist()) | {3125 * 3125, 10 ** 7})
    assert len(ns) >= 20
    for n in ns:
        seg = cv.SSegments(n)
        assert len(seg) <= 64                                   # ~two pieces per binade
        want = np.cumsum(np.full(n, 1.0 / n))
        assert np.array_equal(seg(np.arange(1, n + 1)), want), n


def _masks():
    rs = np.random.RandomState(11)
    out = []
    for density in (1.0, 0.6, 0.05, 0.003):                   # dense ... sparse
        N = int(rs.randint(5000, 200000))
        out.append(rs.rand(N) < density)
    for k in (64, 65, 70, 80, 99):                              # < 100 eligible cells: duplicate-retry rounds
        N = int(rs.randint(1000, 200000))
        m = np.zeros(N, bool)
        m[rs.choice(N, k, replace=False)] = True
        out.append(m)
    return out


@pytest.mark.parametrize("seed", [0, 1, 7, 123])
def test_choice_ranks_equal_numpy_choice_and_rng_state(seed):
    stats = cv.ChoiceStats()
    for i, mask in enumerate(_masks()):
        n = int(mask.sum())
        assert n >= 64
        p = mask.astype(np.int64)
        p = p / np.sum(p)                                       # the reference's probmap: int array / int sum
        np.random.seed(seed * 1000 + i)
        want = np.random.choice(mask.size, 64, replace=False, p=p)
        state_want = np.random.get_state()
        np.random.seed(seed * 1000 + i)
        ranks = cv.choice_ranks(n, 64, stats)
        state_got = np.random.get_state()
        np.testing.assert_array_equal(np.flatnonzero(mask)[ranks], want)
        assert state_got[1].tolist() == state_want[1].tolist() and state_got[2] == state_want[2]
    assert stats.retry_rounds > 0


def test_choice_ranks_whole_pool_is_a_permutation():
    np.random.seed(3)
    p = np.full(64, 1.0 / 64)
    want = np.random.choice(64, 64, replace=False, p=p)
    np.random.seed(3)
    np.testing.assert_array_equal(cv.choice_ranks(64, 64), want)
    with pytest.raises(ValueError):
        cv.choice_ranks(10, 11)


@pytest.mark.parametrize("d", [1, 5, 7, 16, 32])
def test_batched_jitter_draws_consume_the_stream_like_scalar_calls(d):
    np.random.seed(5)
    want = [np.random.randint(d) for _ in range(128)]
    nxt = np.random.random_sample()
    np.random.seed(5)
    got = np.random.randint(d, size=128)
    assert got.tolist() == want and np.random.random_sample() == nxt


GEOMETRIES = [   # h, w, patch, batch, dense_level, speedup, np seed
    (4096, 4096, 224, 64, 2, 16, 0),
    (3000, 5000, 96, 7, 3, 8, 1),
    (512, 640, 96, 4, 1, 16, 1),      # the committed fixture's geometry (this seed takes the forced top-up)
]


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}_{g[2]}_{g[3]}_dl{g[4]}_{g[5]}")
def test_planner_reproduces_oracle_to_full_coverage(geom):
    h, w, P, B, dl, d, seed = geom
    np.random.seed(seed)
    want = list(random_sampler.random_batches(h, w, P, B, dl, d))
    nxt_want = np.random.random_sample()
    np.random.seed(seed)
    planner = cv.CoveragePlanner(B, d, h // d, w // d)
    cmap = cv.NumpyCoverageMap(h, w, P, d, dl)
    got = list(cv.plan_batches(planner, cmap))
    assert len(got) == len(want) and got[-1][1] == 1.0
    for (o_w, f_w), (o_g, f_g) in zip(want, got):
        np.testing.assert_array_equal(o_g, o_w)
        assert f_g == f_w
    assert np.random.random_sample() == nxt_want
    assert planner.stats.batches == len(want)
    GEOM_STATS[geom] = planner.stats


GEOM_STATS: dict = {}


def test_planner_exercised_retries_and_forced_batches():
    """Across the geometries above (replayed here if run alone), the duplicate-retry rounds and the forced top-up
    both occurred."""
    retry = forced = 0
    for geom in GEOMETRIES:
        st = GEOM_STATS.get(geom)
        if st is None:
            h, w, P, B, dl, d, seed = geom
            np.random.seed(seed)
            planner = cv.CoveragePlanner(B, d, h // d, w // d)
            for _ in cv.plan_batches(planner, cv.NumpyCoverageMap(h, w, P, d, dl)):
                pass
            st = planner.stats
        retry += st.retry_rounds
        forced += st.forced_batches
    assert retry > 0 and forced > 0


def test_forced_top_up_pool_includes_full_cells():
    """The top-up may mark a cell that is already hit dense_level times; it then joins the pool (reference :107-112)."""
    np.random.seed(2)
    want = list(random_sampler.random_batches(160, 160, 32, 8, 1, 16))
    np.random.seed(2)
    planner = cv.CoveragePlanner(8, 16, 10, 10)
    got = list(cv.plan_batches(planner, cv.NumpyCoverageMap(160, 160, 32, 16, 1)))
    assert len(got) == len(want) and planner.stats.forced_batches > 0 and planner.stats.forced_cells > 0
    for (a, fa), (b, fb) in zip(want, got):
        np.testing.assert_array_equal(a, b)
        assert fa == fb


def test_planner_refuses_a_map_smaller_than_the_batch():
    with pytest.raises(ValueError, match="smaller than the batch"):
        cv.CoveragePlanner(64, 16, 7, 9)


def test_planner_module_is_numpy_only():
    import ast
    from pathlib import Path
    tree = ast.parse(Path(cv.__file__).read_text())
    mods = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    mods |= {(n.module or "").split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert mods <= {"numpy", "__future__"}, mods
