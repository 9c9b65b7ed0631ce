"""NumPy restatement of the nearest-neighbour layer (deephisto_amd/neighbours.py, dh_embed_knn, dh_embed_knn_votes; DESIGN.md
section 4.21), in float64.

The error model is that of dh_embed_assign (cluster_ref): every float32 distance lies within (1 +- g) of the float64 distance of
the same float32 inputs, g = cluster_ref.gate(D).  From it, for the j-th entry of a row's list: the k-th order statistic of
numbers that each move by at most a factor (1 +- g) moves by at most that factor, so the float32 j-th smallest distance f_j obeys
(1 - g) e_j <= f_j <= (1 + g) e_j with e_j the exact j-th smallest; and the exact distance x_j of the row the kernel returned at
place j obeys f_j / (1 + g) <= x_j <= f_j / (1 - g).  Together: (1 - g) / (1 + g) <= x_j / e_j <= (1 + g) / (1 - g).  Exact
ordered equality with float64 is NOT asserted: two neighbours may be closer than the gate resolves."""
import numpy as np

import cluster_ref

assign_ref = cluster_ref.assign_ref


def check_knn(d64, index, dist, D, k, m0=0):
    """Holds int[n, k] `index` / float[n, k] `dist` of a launch against float64 distances d64[n, m], every row: the indices are
    distinct and in [m0, m0 + m) or the (-1, +inf) padding, which fills exactly the places past the finite candidates; the stored
    pairs ascend lexicographically; each stored distance is within g relative of the exact distance of its index; the exact
    distance of the j-th returned row is within [(1 - g) / (1 + g), (1 + g) / (1 - g)] of the j-th smallest exact distance."""
    index, dist = np.asarray(index, np.int64), np.asarray(dist, np.float64)
    n, m = d64.shape
    g = cluster_ref.gate(D)
    lo, hi = (1 - g) / (1 + g), (1 + g) / (1 - g)
    assert index.shape == (n, k) and dist.shape == (n, k)
    for i in range(n):
        finite = np.sort(d64[i][np.isfinite(d64[i])])
        have = min(k, len(finite))
        idx, dd = index[i], dist[i]
        assert np.all(idx[have:] == -1) and np.all(np.isposinf(dd[have:])), f"row {i}: padding expected from place {have}: {idx}, {dd}"
        idx, dd = idx[:have], dd[:have]
        assert np.all((idx >= m0) & (idx < m0 + m)), f"row {i}: indices outside [{m0}, {m0 + m}): {idx}"
        assert len(np.unique(idx)) == have, f"row {i}: an index twice: {idx}"
        step_d, step_i = np.diff(dd), np.diff(idx)
        assert np.all((step_d > 0) | ((step_d == 0) & (step_i > 0))), f"row {i}: pairs do not ascend: {dd}, {idx}"
        exact = d64[i, idx - m0]
        assert np.all(np.abs(dd - exact) <= g * exact), f"row {i}: a stored distance is off its exact one by more than {D + 4} u"
        want = finite[:have]
        assert np.all((exact >= lo * want) & (exact <= hi * want)), f"row {i}: a returned row is not among the nearest within the gate"


def topk_ref(d32, k, m0=0):
    """(int32[n, k], float32[n, k]): the k smallest (distance, index) pairs per row of float32 distances, with the padding; for
    bit-exact comparisons where the float32 distances themselves are at hand."""
    d32 = np.asarray(d32, np.float32)
    n, m = d32.shape
    index, dist = np.full((n, k), -1, np.int32), np.full((n, k), np.inf, np.float32)
    for i in range(n):
        cand = [j for j in range(m) if d32[i, j] < np.inf]
        cand.sort(key=lambda j: (d32[i, j], j))
        for p, j in enumerate(cand[:k]):
            index[i, p], dist[i, p] = m0 + j, d32[i, j]
    return index, dist


def votes_ref(index, bank_labels, n_classes):
    """(int32[n, C] votes, int32[n] labels) by a plain loop: one vote per neighbour in stored order; an index of -1 or outside
    [0, m) and a label outside [0, C) cast none; the label is the class with the most votes, at equal votes the one whose first
    member comes earliest in the list, -1 when nobody voted."""
    index, bank_labels = np.asarray(index, np.int64), np.asarray(bank_labels, np.int64)
    n, m, C = index.shape[0], len(bank_labels), int(n_classes)
    votes, label = np.zeros((n, C), np.int32), np.full(n, -1, np.int32)
    for i in range(n):
        first = {}
        for p, j in enumerate(index[i]):
            if not 0 <= j < m or not 0 <= bank_labels[j] < C:
                continue
            c = int(bank_labels[j])
            votes[i, c] += 1
            first.setdefault(c, p)
        if first:
            label[i] = min(first, key=lambda c: (-votes[i, c], first[c]))
    return votes, label
