"""NumPy restatement of the tile quality rule for the tests: np.pad(mode="edge") for the Laplacian,
boolean masks, decisions in Python ints.  Nothing here calls the library."""
import math

import numpy as np

BLUR, INK = 2, 4
DEFAULTS = dict(ink_chroma=40, ink_margin=16, dark_max=40)


def luma(img):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def chroma(img):
    return img.max(axis=-1).astype(np.int64) - img.min(axis=-1).astype(np.int64)


def tissue_mask(img, t):
    return chroma(img) > t


def ink_mask(img, ink_chroma=40, ink_margin=16, dark_max=40):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return ((chroma(img) > ink_chroma) & (g - np.minimum(r, b) >= ink_margin)) | (img.max(axis=-1).astype(np.int64) <= dark_max)


def laplacian(img):
    """L of every pixel of `img`, whose border is the slide's border: neighbours outside repeat the edge pixel."""
    y = np.pad(luma(img), 1, mode="edge")
    return 4 * y[1:-1, 1:-1] - y[:-2, 1:-1] - y[2:, 1:-1] - y[1:-1, :-2] - y[1:-1, 2:]


def tile_stats(img, origins, P, t, **ink):
    """int64[n, 4]: (n_t, S1, S2, n_ink) of the P x P windows of the slide `img` at `origins`."""
    lap, tis, nk = laplacian(img), tissue_mask(img, t), ink_mask(img, **{**DEFAULTS, **ink})
    out = np.zeros((len(origins), 4), np.int64)
    for i, (y, x) in enumerate(np.asarray(origins).tolist()):
        L, m = lap[y:y + P, x:x + P], tis[y:y + P, x:x + P]
        out[i] = (int(m.sum()), int(L[m].sum()), int((L[m] * L[m]).sum()), int(nk[y:y + P, x:x + P].sum()))
    return out


def window_stats(win, P, t, top, bottom, left, right, **ink):
    """(n_t, S1, S2, n_ink) of ONE tile from `win`, the tile plus its one-pixel halo as far as the slide has one: `top`, `bottom`,
    `left`, `right` say on which sides `win` carries a halo row / column (a side without one is a slide border)."""
    full = np.pad(win, ((0 if top else 1, 0 if bottom else 1), (0 if left else 1, 0 if right else 1), (0, 0)), mode="edge")
    assert full.shape[:2] == (P + 2, P + 2)
    y = luma(full)
    L = (4 * y[1:-1, 1:-1] - y[:-2, 1:-1] - y[2:, 1:-1] - y[1:-1, :-2] - y[1:-1, 2:])
    core = full[1:-1, 1:-1]
    m = tissue_mask(core, t)
    return np.array([int(m.sum()), int(L[m].sum()), int((L[m] * L[m]).sum()), int(ink_mask(core, **{**DEFAULTS, **ink}).sum())],
                    np.int64)


def max_ink_pixels(max_ink_fraction, P):
    return math.floor(max_ink_fraction * P * P)


def reason(n_t, s1, s2, n_ink, min_sharpness, max_ink):
    n_t, s1, s2, n_ink = int(n_t), int(s1), int(s2), int(n_ink)
    blur = min_sharpness > 0 if n_t == 0 else n_t * s2 - s1 * s1 < min_sharpness * n_t * n_t
    return (BLUR if blur else 0) | (INK if n_ink > max_ink else 0)


def flags(stats, min_sharpness, max_ink):
    """(reason uint8[n], keep int32[n]) of int64[n, 4] stats, row by row in Python ints."""
    r = np.array([reason(*row, min_sharpness, max_ink) for row in np.asarray(stats).tolist()], np.uint8).reshape(-1)
    return r, (r == 0).astype(np.int32)


def painted(h, w, seed):
    """Pink noise (R 200..255, G 100..160, B 170..230) with the top-right quarter box-blurred 5 x 5, the bottom-left quarter
    flat blue (20, 60, 200) and the bottom-right quarter flat (10, 10, 10); the top-left quarter stays sharp.  Returns
    (uint8[h, w, 3], areas) with areas = name -> (y0, y1, x0, x1)."""
    rng = np.random.default_rng(seed)
    img = np.stack([rng.integers(200, 256, (h, w)), rng.integers(100, 161, (h, w)), rng.integers(170, 231, (h, w))], 2).astype(np.uint8)
    hy, hx = h // 2, w // 2
    areas = dict(sharp=(0, hy, 0, hx), blur=(0, hy, hx, w), blue=(hy, h, 0, hx), black=(hy, h, hx, w))
    img[:hy, hx:] = box_blur(img, 5)[:hy, hx:]
    img[hy:, :hx] = (20, 60, 200)
    img[hy:, hx:] = (10, 10, 10)
    return img, areas


def box_blur(img, k):
    """k x k box mean of a uint8 image, edge-replicated, rounded half up."""
    p = k // 2
    a = np.pad(img.astype(np.int64), ((p, p), (p, p), (0, 0)), mode="edge")
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1, 3), np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    h, w = img.shape[:2]
    box = s[k:k + h, k:k + w] - s[:h, k:k + w] - s[k:k + h, :w] + s[:h, :w]
    return ((2 * box + k * k) // (2 * k * k)).astype(np.uint8)


def inside(origins, P, area, h, w):
    """Boolean: which P x P tiles lie wholly inside `area` = (y0, y1, x0, x1) of an h x w slide, with one pixel of margin for the
    Laplacian's halo wherever the area ends inside the slide (at the slide's border the halo repeats the area's own pixels)."""
    y0, y1, x0, x1 = area
    y0, x0, y1, x1 = y0 + (y0 > 0), x0 + (x0 > 0), y1 - (y1 < h), x1 - (x1 < w)
    o = np.asarray(origins)
    return (o[:, 0] >= y0) & (o[:, 0] + P <= y1) & (o[:, 1] >= x0) & (o[:, 1] + P <= x1)


def filtered_map(logits_unfiltered, origins, n_unique, kept, P, d, h, w, fill, dedupe=False):
    """The oracle of the filtered class map: the UNFILTERED run's logits, kept rows only, in grid order (the corner's padding
    duplicates follow the corner), float32 +=, argmax, uncovered cells filled."""
    n_cls = logits_unfiltered.shape[1]
    rows = list(kept)
    if not dedupe and len(kept) and kept[-1] == n_unique - 1:
        rows += list(range(n_unique, len(origins)))
    canvas = np.zeros((h // d, w // d, n_cls), np.float32)
    cover = np.zeros((h // d, w // d), bool)
    for i in rows:
        y, x = int(origins[i, 0]), int(origins[i, 1])
        canvas[y // d:(y + P) // d, x // d:(x + P) // d] += logits_unfiltered[i]
        cover[y // d:(y + P) // d, x // d:(x + P) // d] = True
    out = np.argmax(canvas, axis=2).astype(np.int64)
    out[~cover] = fill
    return out


def boundary_cases():
    """Tile decisions at the bounds of the int64 comparison: (n_t, S1, S2, n_ink, min_sharpness, max_ink_pixels) each."""
    n, m = 2 ** 20, 1020 * 1020
    cases = []
    for ms in (0, 1, 5, 200, m - 1, m):
        for mi in (0, 1, n - 1, n):
            cases += [(n, 1020 * n, n * m, n, ms, mi), (n, -1020 * n, n * m, 0, ms, mi),       # every L = +-1020: variance 0
                      (n, 0, n * m, mi, ms, mi), (n, 0, n * m - 1, mi + 1, ms, mi),            # variance 1020^2 and just below
                      (n, 0, n * ms, 1, ms, mi), (n, 0, max(n * ms - 1, 0), 1, ms, mi),        # equality at the threshold, one below
                      (4, 2, 21, 0, ms, mi), (4, 2, 20, 0, ms, mi), (4, -2, 21, 5, ms, mi),      # 4 * S2 - 4 against ms * 16
                      (1, 1020, m, 0, ms, mi), (1, -7, 49, 1, ms, mi),                         # one pixel: variance 0
                      (0, 0, 0, 0, ms, mi), (0, 0, 0, mi + 1, ms, mi)]                         # no tissue pixel
    return cases
