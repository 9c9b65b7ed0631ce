"""NumPy restatement of the fine accumulation: the expanded list, the reference's `+=` loop over it with
patch 32, and the mean / count / argmax rules of the probability maps over it."""
import numpy as np


def expand_positions(origins, patch):
    """Brute force: one (y + 32 i, x + 32 j) per tile and position, tile-major, i along y outermost, j along x."""
    s = patch // 32
    return np.asarray([(y + 32 * i, x + 32 * j) for y, x in np.asarray(origins).reshape(-1, 2).tolist()
                       for i in range(s) for j in range(s)], dtype=np.int32).reshape(-1, 2)


def owner(c, d, y, patch):
    """The position along one axis that the formula gives cell `c` of a tile at `y` (the caller knows the tile covers the cell)."""
    return min(-(-((c + 1) * d - y) // 32) - 1, patch // 32 - 1)


def accumulate(h, w, d, patch, origins, cam, canvas=None):
    """float32[h//d, w//d, n_cls]: `canvas[y//d:(y+32)//d, x//d:(x+32)//d] += row` over the expanded list, in list order."""
    rows = np.asarray(cam, dtype=np.float32).reshape(-1, np.shape(cam)[-1])
    canvas = np.zeros([h // d, w // d, rows.shape[1]], dtype=np.float32) if canvas is None else canvas.copy()
    for (y, x), v in zip(expand_positions(origins, patch).tolist(), rows):
        canvas[y // d:(y + 32) // d, x // d:(x + 32) // d, :] += v
    return canvas


def softmax(v):
    v = np.asarray(v, dtype=np.float32)
    e = np.exp(v - v.max())
    s = np.float32(0)
    for x in e:   # in class order
        s = np.float32(s + x)
    return e / s


def mean(h, w, d, patch, origins, probs, fill=-1):
    """dict(proba, count, class_map, confidence) of per-position probability rows `probs` (taken as they are) over the expanded
    list: sums and hit counts in list order, proba = sum / float32(count), first maximum, 0 / `fill` where nothing covers."""
    rows = np.asarray(probs, dtype=np.float32).reshape(-1, np.shape(probs)[-1])
    total = np.zeros([h // d, w // d, rows.shape[1]], dtype=np.float32)
    count = np.zeros([h // d, w // d], dtype=np.int32)
    for (y, x), v in zip(expand_positions(origins, patch).tolist(), rows):
        total[y // d:(y + 32) // d, x // d:(x + 32) // d, :] += v
        count[y // d:(y + 32) // d, x // d:(x + 32) // d] += 1
    covered = count > 0
    proba = np.zeros_like(total)
    proba[covered] = total[covered] / count[covered][:, None].astype(np.float32)
    class_map = np.argmax(proba, axis=2).astype(np.int64)
    confidence = np.take_along_axis(proba, class_map[..., None], axis=2)[..., 0]
    class_map[~covered] = fill
    return dict(proba=proba, count=count, class_map=class_map, confidence=confidence)
