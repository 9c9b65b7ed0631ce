"""NumPy restatement of the embedding kernels (deephisto_amd/csrc/embed.hip).

`class_sums_ref` repeats dh_embed_class_sums' summation ORDER in float32, so it must agree bit for bit; `normalize_ref`, `scores_ref` and
`prototype_map_ref` are float64 and come with the bounds the GPU tests hold the kernels to."""
import numpy as np

CHUNK_ROWS = 1024   # DH_EMBED_CHUNK_ROWS
U = 2.0 ** -24      # unit roundoff of float32


def class_sums_ref(feat, label, K, chunk_rows=CHUNK_ROWS):
    """(float32[K, D], int64[K]): rows with a label in [0, K) summed per class.  A chunk's partial starts at 0 and adds its rows in
    ascending order; the result starts at 0 and adds the partials of all chunks in ascending chunk order; float32 throughout."""
    feat = np.asarray(feat, np.float32)
    label = np.asarray(label)
    n, D = feat.shape
    sums = np.zeros((K, D), np.float32)
    counts = np.zeros(K, np.int64)
    for c0 in range(0, n, chunk_rows):
        part = np.zeros((K, D), np.float32)
        lab = label[c0:c0 + chunk_rows]
        for k in range(K):
            rows = np.nonzero(lab == k)[0]
            counts[k] += len(rows)
            acc = part[k]
            for r in rows:                      # one float32 add per row, in row order
                acc = acc + feat[c0 + r]
            part[k] = acc
        sums = sums + part
    return sums, counts


def normalize_ref(feat):
    """float64: row / sqrt(sum row^2); rows whose sum of squares is 0 stay zero."""
    x = np.asarray(feat, np.float64)
    s = np.sqrt((x * x).sum(1, keepdims=True))
    return np.divide(x, s, out=np.zeros_like(x), where=s > 0)


def normalize_bound(D):
    """Relative error allowed per element: the squares' sum in any order gives gamma_D, the square root halves it, the divide adds u;
    the gate is twice that."""
    return (D + 4) * U


def scores_ref(feat, proto, scale):
    """(float64[n, K] scores, float64[n, K] bound): scale * feat @ proto.T and (D + 2) u |scale| sum |f| |p|."""
    f, p = np.asarray(feat, np.float64), np.asarray(proto, np.float64)
    D = f.shape[1]
    return scale * (f @ p.T), (D + 2) * U * abs(scale) * (np.abs(f) @ np.abs(p).T)


def footprints(origins, P, d, h, w):
    for y, x in np.asarray(origins, np.int64):
        yield slice(y // d, min((y + P) // d, h // d)), slice(x // d, min((x + P) // d, w // d))


def prototype_map_ref(feat, label, K, origins, P, d, h, w, scale=1.0):
    """The float64 pipeline of PrototypeClassifier(K).fit(feat, label).predict_map(...): normalise, class means, normalise, scores,
    accumulation over the tiles' footprints, first maximum.  Returns (int64[h // d, w // d] map, -1 where no tile covers the cell;
    bool mask of the covered cells whose top two accumulated scores differ by MORE than the scores' bound summed over the cell's
    tiles: the cells a float32 pipeline must reproduce)."""
    x = normalize_ref(feat)
    label = np.asarray(label)
    mean = np.zeros((K, x.shape[1]))
    for k in range(K):
        rows = label == k
        if rows.any():
            mean[k] = x[rows].sum(0) / rows.sum()
    proto = normalize_ref(mean)
    sc, bound = scores_ref(x, proto, scale)
    canvas = np.zeros((h // d, w // d, K))
    slack = np.zeros((h // d, w // d))
    hits = np.zeros((h // d, w // d), np.int64)
    for i, (ys, xs) in enumerate(footprints(origins, P, d, h, w)):
        canvas[ys, xs] += sc[i]
        slack[ys, xs] += bound[i].max()
        hits[ys, xs] += 1
    cmap = np.where(hits > 0, canvas.argmax(2), -1)
    if K > 1:
        top = np.sort(canvas, axis=2)
        decided = (top[..., -1] - top[..., -2]) > slack
    else:
        decided = np.ones_like(hits, bool)
    return cmap, decided & (hits > 0)


def standin_features(n, D, seed):
    """Seeded stand-ins for pooled ResNet features: non-negative (they follow a ReLU), a shared mean direction plus per-tile detail."""
    rng = np.random.default_rng(seed)
    base = np.abs(rng.standard_normal(D))
    return (base + 0.5 * np.abs(rng.standard_normal((n, D)))).astype(np.float32)


def tile_labels_ref(xy, ring_start, ring_class, origins, P, d, h, w):
    """int32[n]: the class of the annotation rings (deephisto_amd.scoring.annotation_rings) at the centre ((cx + 0.5) d, (cy + 0.5) d)
    of the cell under each tile's centre pixel (y + P // 2, x + P // 2), by the even-odd rule of dh_rasterize_regions in float64; -1
    where no ring, or rings of several classes, hold it, and where the cell lies past the h // d x w // d map."""
    out = np.full(len(origins), -1, np.int32)
    for i, (y, x) in enumerate(np.asarray(origins, np.int64)):
        cy, cx = (y + P // 2) // d, (x + P // 2) // d
        if cy >= h // d or cx >= w // d:
            continue
        px, py = (cx + 0.5) * d, (cy + 0.5) * d
        found = set()
        for r in range(len(ring_class)):
            a = np.asarray(xy[ring_start[r]:ring_start[r + 1]], np.float64)
            b = np.roll(a, -1, axis=0)
            cross = (a[:, 1] > py) != (b[:, 1] > py)
            with np.errstate(divide="ignore", invalid="ignore"):
                xi = a[:, 0] + (py - a[:, 1]) * (b[:, 0] - a[:, 0]) / (b[:, 1] - a[:, 1])
            if np.count_nonzero(cross & (px < xi)) % 2:
                found.add(int(ring_class[r]))
        if len(found) == 1:
            out[i] = found.pop()
    return out
