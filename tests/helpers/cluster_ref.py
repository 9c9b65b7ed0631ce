"""NumPy restatement of the clustering layer (deephisto_amd/clustering.py, dh_embed_assign), in float64.

The error model of the kernel's distance (one float32 subtract, then a chain of fused multiply-adds of non-negative terms): purely
relative, to first order (D + 2) u of the float64 distance of the same float32 inputs; the gate `gate(D)` = (D + 4) u adds 2 u for
the second-order terms.  From it: the winner's exact distance is within (1 + g) / (1 - g) of the smallest, and where a row's
second-nearest exact distance exceeds its nearest by more than that factor (`lloyd_ref` asks for its square), float32 and float64
must pick the same centre."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of float32


def gate(D):
    return (D + 4) * U


def assign_ref(feat, centres):
    """float64[n, K]: the squared Euclidean distances of the float32 inputs, centre by centre (n x D temporaries only)."""
    x, c = np.asarray(feat, np.float64), np.asarray(centres, np.float64)
    d = np.empty((x.shape[0], c.shape[0]))
    for k in range(c.shape[0]):
        t = x - c[k]
        d[:, k] = np.einsum("ij,ij->i", t, t)
    return d


def check_assign(d64, label, dist, D, k0=0):
    """Holds (label, dist) of a launch against float64 distances d64[n, K], every row: the label in [k0, k0 + K), the chosen centre's
    exact distance within (1 + g) / (1 - g) of the smallest, the stored distance within g relative of the chosen centre's exact
    one.  Returns the worst |dist - exact| / exact in units of u."""
    label, dist = np.asarray(label, np.int64), np.asarray(dist, np.float64)
    n, K = d64.shape
    g = gate(D)
    assert label.shape == (n,) and dist.shape == (n,)
    assert np.all((label >= k0) & (label < k0 + K)), f"labels outside [{k0}, {k0 + K}): {np.unique(label)}"
    chosen = d64[np.arange(n), label - k0]
    best = d64.min(axis=1)
    bad = chosen > best * (1 + g) / (1 - g)
    assert not bad.any(), f"{int(bad.sum())} rows chose a centre farther than the gate allows, first row {int(np.argmax(bad))}"
    err = np.abs(dist - chosen)
    assert np.all(err <= g * chosen), f"worst |dist - d64| / d64 = {np.max(err[chosen > 0] / chosen[chosen > 0]) / U:.2f} u, gate {D + 4} u"
    return float(np.max(err[chosen > 0] / chosen[chosen > 0]) / U) if (chosen > 0).any() else 0.0


def lexmin(dists, labels):
    """The lexicographic (dist, label) minimum per row over several launches' results (lists of float32[n] and int[n])."""
    bd, bl = np.array(dists[0], copy=True), np.array(labels[0], copy=True)
    for d, l in zip(dists[1:], labels[1:]):
        take = (d < bd) | ((d == bd) & (l < bl))
        bd, bl = np.where(take, d, bd), np.where(take, l, bl)
    return bd, bl


# ---- k-means ----------------------------------------------------------------------------------------------------------------
BLOB_SIZES = (400, 310, 200, 120)   # 1030 rows: past the 1024-row chunk of dh_embed_class_sums


def blobs(D=64, sizes=BLOB_SIZES, seed=5, spread=1.0, separation=6.0):
    """(float32[n, D] rows in shuffled order, int64[n] blob of each row, float32[len(sizes), D] blob centres): normal blobs of the
    given sizes and spread around normal centres scaled by `separation` (centre distance ~ separation * sqrt(2 D) >> spread * sqrt(D))."""
    rng = np.random.default_rng(seed)
    centres = separation * rng.standard_normal((len(sizes), D))
    which = np.repeat(np.arange(len(sizes)), sizes)
    x = centres[which] + spread * rng.standard_normal((len(which), D))
    perm = rng.permutation(len(which))
    return x[perm].astype(np.float32), which[perm].astype(np.int64), centres.astype(np.float32)


def blob_init(centres):
    """float32[4, D] initial centres that make Lloyd work for its result without cutting a blob twice: blobs 0 and 1 start at
    their own centres; centre 2 starts midway between blobs 2 and 3 and centre 3 as far beyond blob 3, so the first assignment
    cuts blob 3 in half (once, with the two centres a blob distance apart: near-ties are rare and the seed has none), the first
    update pulls centre 2 back to blob 2, the second assignment makes blob 3 whole and the third changes nothing."""
    c = np.asarray(centres, np.float64)
    init = c.copy()
    init[2] = c[2] + 0.5 * (c[3] - c[2])
    init[3] = c[3] + 0.5 * (c[3] - c[2])
    return np.ascontiguousarray(init, dtype=np.float32)


def canonical_ref(counts):
    """Old cluster numbers by descending size, ties by the lower old number (a plain sort, to check the module's lexsort)."""
    return np.array(sorted(range(len(counts)), key=lambda k: (-int(counts[k]), k)), dtype=np.int64)


def _first_max(d):
    return int(np.argmax(d))


def lloyd_ref(x, init, max_iter=50, check_margin=True):
    """float64 Lloyd from explicit initial centres under the rules of clustering.KMeans: first minimum at equal distances; an empty
    cluster's centre becomes the row of largest distance (first maximum, then counted as 0), in ascending cluster order; stop
    when no label changes; clusters renumbered by descending size.

    At every assignment with pairwise distinct centres it ASSERTS that each row's second-nearest distance exceeds its nearest by
    more than ((1 + g) / (1 - g))^2, and at every reseeding that the largest distance exceeds the runner-up by the same factor:
    under the kernel's error model a float32 run must then take the same decisions.  Returns a dict: labels (canonical), centres
    (float64, canonical), counts, inertia, n_iter, converged."""
    x = np.asarray(x, np.float64)
    centres = np.asarray(init, np.float64).copy()
    n, D = x.shape
    K = len(centres)
    factor = ((1 + gate(D)) / (1 - gate(D))) ** 2

    def assign(c):
        d = assign_ref(x, c)
        lab = d.argmin(axis=1)
        distinct = len(np.unique(c, axis=0)) == K
        if check_margin and K > 1 and distinct:
            two = np.partition(d, 1, axis=1)
            assert np.all(two[:, 1] > two[:, 0] * factor), "a row's two nearest centres are closer than the float32 gate resolves"
        return lab, d[np.arange(n), lab]

    lab, dist = assign(centres)
    n_iter, converged = 0, False
    for _ in range(max_iter):
        cnt = np.bincount(lab, minlength=K)
        centres = np.stack([x[lab == k].sum(0) / max(1, cnt[k]) for k in range(K)])
        d = dist.copy()
        for k in np.flatnonzero(cnt == 0):
            row = _first_max(d)
            if check_margin:
                top = np.sort(d)[-2:]
                assert top[1] > top[0] * factor, "the two farthest rows are closer than the float32 gate resolves"
            centres[k] = x[row]
            d[row] = 0.0
        new, dist = assign(centres)
        changed = int((new != lab).sum())
        lab = new
        n_iter += 1
        if changed == 0:
            converged = True
            break
    cnt = np.bincount(lab, minlength=K)
    order = canonical_ref(cnt)
    new_of_old = np.empty(K, np.int64)
    new_of_old[order] = np.arange(K)
    return dict(labels=new_of_old[lab], centres=centres[order], counts=cnt[order], inertia=float(dist.sum()), n_iter=n_iter,
                converged=converged)


# ---- the map ----------------------------------------------------------------------------------------------------------------
def footprints(origins, P, d, h, w):
    for y, x in np.asarray(origins, np.int64):
        yield slice(y // d, min((y + P) // d, h // d)), slice(x // d, min((x + P) // d, w // d))


def cluster_map_ref(origins, labels, K, P, d, h, w, fill_class=-1):
    """int64[h // d, w // d]: per cell the cluster with the most covering tiles (first maximum), `fill_class` where no tile of
    `origins` covers the cell or none of the covering tiles has a label in [0, K)."""
    votes = np.zeros((h // d, w // d, K), np.int64)
    for lb, (ys, xs) in zip(np.asarray(labels, np.int64), footprints(origins, P, d, h, w)):
        if 0 <= lb < K:
            votes[ys, xs, lb] += 1
    return np.where(votes.sum(2) > 0, votes.argmax(2), fill_class).astype(np.int64)
