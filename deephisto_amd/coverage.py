"""Host planner of the coverage-driven random sampler (FullImageRndSampler, device index logic).

The reference (patch_samplers/full_samplers.py:105-153) draws each batch with

    p = np.where(accum >= dense_level, 0, 1); <top-up while fewer than B cells>; p = p / np.sum(p)
    idx = np.random.choice(dh * dw, B, replace=False, p=p.flatten())
    y/x jitter: np.random.randint(d) twice per index

which scans the whole map for every batch.  The probability map only holds 0 and c = 1/n (n eligible cells), and
NumPy's `choice(replace=False, p)` is, round by round: draw `rand(B - found)`, zero the found entries, `cdf = cumsum(p)`
(sequential float64), `cdf /= cdf[-1]`, `searchsorted(x, 'right')`, keep first occurrences.  Adding 0.0 never changes a
running sum, so cdf[i] = S(m_i) / S(M), where m_i is the number of still-eligible cells at or before cell i and S(m) is
the sequential float64 sum of m copies of c.  The draw for a uniform x is therefore "the eligible cell of rank m* - 1",
m* the smallest m with fl(S(m) / S(M)) > x -- integer work in rank space plus the closed form of S below.  The device
(`DeviceCoverageMap`, csrc/coverage.hip) owns the map and turns ranks into cells; this module draws every random number
in the reference's order, so the global NumPy stream is consumed exactly as the reference consumes it.

S(m) is piecewise linear: inside a binade s stays on a fixed ulp grid, and after the first step in the binade every
addition of c rounds to the same increment (a round-half-to-even tie can only change that first step).  So there are
about two pieces per binade (~50 at n = 10^7), each found with real float adds at its start.

Pure NumPy; no torch and no GPU here.
"""
from __future__ import annotations

import numpy as np

_F64 = np.float64


class SSegments:
    """Piecewise form of S(m) = fl(...fl(fl(c + c) + c)... + c) (m terms, c = fl(1/n)) for 0 <= m <= n.

    Piece k covers m in [m0[k], m0[k+1]) with S(m) = s0[k] + (m - m0[k]) * inc[k], all exact in float64."""

    def __init__(self, n: int):
        if n < 1:
            raise ValueError("n must be >= 1")
        self.n = int(n)
        c = 1.0 / self.n          # == (int array / int sum) of the reference: the correctly rounded float64 1/n
        self.c = c
        m0, s0, inc = [0], [0.0], [0.0]
        m, s = 0, 0.0
        while m < self.n:
            # first point of a new binade (or the start): one honest add
            p0 = s + c
            m += 1
            m0.append(m); s0.append(p0); inc.append(0.0)
            if m >= self.n:
                break
            p1 = p0 + c
            if np.frexp(p1)[1] != np.frexp(p0)[1]:   # p1 already in the next binade: p0 was a one-point piece
                s = p0
                continue
            # p0 -> p1 was the first step inside this binade; from p1 on every step adds the same increment
            p2 = p1 + c
            step = p2 - p1                             # exact (Sterbenz)
            top = np.ldexp(1.0, int(np.frexp(p1)[1]))   # first value of the next binade
            # the largest j with p1 + j * step < top and m + 1 + j <= n
            j = int((top - p1) // step)
            while j > 0 and p1 + j * step >= top:
                j -= 1
            while p1 + (j + 1) * step < top:
                j += 1
            j = min(j, self.n - (m + 1))
            m0.append(m + 1); s0.append(p1); inc.append(step)
            m += 1 + j
            s = p1 + j * step
        self.m0 = np.asarray(m0, dtype=np.int64)
        self.s0 = np.asarray(s0, dtype=_F64)
        self.inc = np.asarray(inc, dtype=_F64)

    def __len__(self):
        return len(self.m0)

    def __call__(self, m):
        """S(m), elementwise over an integer array (or scalar) 0 <= m <= n."""
        m = np.asarray(m, dtype=np.int64)
        k = np.searchsorted(self.m0, m, side="right") - 1
        return self.s0[k] + (m - self.m0[k]).astype(_F64) * self.inc[k]


class ChoiceStats:
    """What the planner did (tests use it to prove which paths ran)."""

    def __init__(self):
        self.batches = 0
        self.retry_rounds = 0      # choice rounds beyond the first (duplicate draws)
        self.forced_batches = 0    # batches with the forced top-up (fewer than B eligible cells)
        self.forced_cells = 0      # cells added by the top-up

    def __repr__(self):
        return (f"ChoiceStats(batches={self.batches}, retry_rounds={self.retry_rounds}, "
                f"forced_batches={self.forced_batches}, forced_cells={self.forced_cells})")


_SEG_CACHE: dict = {}


def segments(n: int) -> SSegments:
    s = _SEG_CACHE.get(n)
    if s is None:
        if len(_SEG_CACHE) > 64:
            _SEG_CACHE.clear()
        s = _SEG_CACHE[n] = SSegments(n)
    return s


def _first_rank_above(seg: SSegments, x: np.ndarray, M: int) -> np.ndarray:
    """For each uniform x: the smallest m in [1, M] with fl(S(m) / S(M)) > x, as a 0-based rank m - 1."""
    SM = seg(M)
    lo = np.zeros(x.shape, np.int64)            # invariant: cdf(lo) <= x  (cdf(0) = 0 <= x)
    hi = np.full(x.shape, M, np.int64)          # invariant: cdf(hi) > x   (cdf(M) = 1 > x)
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            return hi - 1
        mid = (lo + hi) // 2
        above = (seg(mid) / SM) > x
        hi = np.where(open_ & above, mid, hi)
        lo = np.where(open_ & ~above, mid, lo)


def choice_ranks(n: int, size: int, stats: ChoiceStats | None = None) -> np.ndarray:
    """Ranks (0..n-1, among the n equally likely cells in row-major order) that
    `np.random.choice(N, size, replace=False, p=<1/n on n cells, 0 elsewhere>)` returns, in its order, consuming
    `np.random.random_sample` exactly as it does (duplicate-retry rounds included)."""
    if size > n:
        raise ValueError(f"cannot choose {size} of {n} cells without replacement")
    seg = segments(n)
    found: list[int] = []
    rounds = 0
    while len(found) < size:
        x = np.random.random_sample(size - len(found))
        M = n - len(found)
        r = _first_rank_above(seg, x, M)             # ranks among the cells not found yet
        if found:                                    # -> ranks among all n cells (skip the found ones, in order)
            f = np.sort(np.asarray(found, np.int64))
            # the r-th cell not in f: the smallest t with t - #(f <= t) == r
            t = r.copy()
            for fv in f:
                t = t + (t >= fv)
            r = t
        _, first = np.unique(r, return_index=True)
        first.sort()
        found.extend(int(v) for v in r[first])
        rounds += 1
    if stats is not None:
        stats.retry_rounds += rounds - 1
    return np.asarray(found, dtype=np.int64)


class CoveragePlanner:
    """Replays the reference's per-batch RNG order against a coverage map behind a narrow interface.

    `cmap` provides: `dh`, `dw`, `size` (= dh * dw), `eligible` / `filled` (counts after the last step),
    `eligible_cells()` (int64 flat indices of the cells with count < dense_level; only called when fewer than B),
    and `step(idx, explicit, jitter)`: idx are ranks among the eligible cells (explicit = False) or flat cell
    indices (explicit = True), jitter int[B, 2] (jy, jx); it applies the batch and returns (origins, filled, eligible)
    or queues it (the caller then reads the counters).  Per batch:
      1. forced top-up (`np.random.randint(0, dh, size=1)`, `np.random.randint(0, dw, size=1)` until B cells),
      2. the choice (`choice_ranks`),
      3. 2B jitter draws (`np.random.randint(d, size=2B)` == 2B scalar `randint(d)` calls: y, x per index)."""

    def __init__(self, batch_size: int, speedup: int, dh: int, dw: int):
        self.B, self.d, self.dh, self.dw = int(batch_size), int(speedup), int(dh), int(dw)
        if self.dh * self.dw < self.B:
            raise ValueError(f"coverage map of {self.dh}x{self.dw} cells is smaller than the batch ({self.B}): "
                             "the reference's top-up would never end")
        self.stats = ChoiceStats()

    def plan(self, eligible: int, eligible_cells=None):
        """(idx, explicit, jitter int32[B,2]) for the next batch.  `eligible_cells` is a callable returning the flat
        indices of the eligible cells, called only when eligible < B."""
        B, st = self.B, self.stats
        st.batches += 1
        if eligible < B:
            cells = set(int(v) for v in np.asarray(eligible_cells()).ravel())
            n0 = len(cells)
            while len(cells) < B:
                y = np.random.randint(0, self.dh, size=1)
                x = np.random.randint(0, self.dw, size=1)
                cells.add(int(y[0]) * self.dw + int(x[0]))
            st.forced_batches += 1
            st.forced_cells += len(cells) - n0
            pool = np.asarray(sorted(cells), dtype=np.int64)
            idx = pool[choice_ranks(len(pool), B, st)]
            explicit = True
        else:
            idx = choice_ranks(int(eligible), B, st)
            explicit = False
        jit = np.random.randint(self.d, size=2 * B).astype(np.int32).reshape(B, 2)
        return idx, explicit, jit


class NumpyCoverageMap:
    """Host restatement of the device map (reference semantics); the planner's stand-in where no GPU is present."""

    def __init__(self, h, w, patch, speedup, dense_level):
        self.h, self.w, self.P, self.d, self.dl = int(h), int(w), int(patch), int(speedup), int(dense_level)
        self.dh, self.dw = self.h // self.d, self.w // self.d
        self.size = self.dh * self.dw
        self.accum = np.zeros((self.dh, self.dw), np.int32)
        self.filled, self.eligible = 0, self.size

    def eligible_cells(self):
        return np.flatnonzero(self.accum.ravel() < self.dl)

    def origins(self, cells, jitter):
        d, P = self.d, self.P
        pd2 = P // d // 2
        cells = np.asarray(cells, np.int64)
        y = (cells // self.dw - pd2) * d + jitter[:, 0]
        x = (cells % self.dw - pd2) * d + jitter[:, 1]
        return np.stack([np.clip(y, 0, self.h - P), np.clip(x, 0, self.w - P)], 1).astype(np.int32)

    def step(self, idx, explicit, jitter):
        cells = np.asarray(idx, np.int64) if explicit else self.eligible_cells()[np.asarray(idx, np.int64)]
        o = self.origins(cells, jitter)
        d, P = self.d, self.P
        for y, x in o:
            self.accum[y // d:(y + P) // d, x // d:(x + P) // d] += 1
        self.filled = int(np.count_nonzero(self.accum))
        self.eligible = int(np.count_nonzero(self.accum < self.dl))
        return o, self.filled / self.size, self.eligible


def plan_batches(planner: CoveragePlanner, cmap):
    """Yield (origins int32[B,2], filled) to full coverage, driving `cmap` (e.g. NumpyCoverageMap) synchronously."""
    filled, eligible = 0.0, cmap.eligible
    while filled < 1:
        idx, explicit, jit = planner.plan(eligible, cmap.eligible_cells)
        o, filled, eligible = cmap.step(idx, explicit, jit)
        yield o, filled
