"""NumPy restatement, in int64, of the area resampling of DESIGN.md section 4.14, written from its formula:

    oh = (h den) // num, ow = (w den) // num
    wy(y, j) = max(0, min((j+1) den, (y+1) num) - max(j den, y num)), wx the same in x
    S = sum_j sum_i wy wx src[j][i][c],  D = num^2,  out = (2 S + D) // (2 D)

A weight table per axis, two matrix products in int64, one rounding.  The tables are banded (an output index touches at most
num / den + 2 source indices), so each product is taken over runs of CHUNK output indices and the source window under them: the
same sums, without the zeros.  The row helpers compute a few output rows of a very tall slide from just the source rows under
them."""
from fractions import Fraction

import numpy as np

CHUNK = 64


def factor(f):
    f = Fraction(f)
    return f.numerator, f.denominator


def weights(n_src: int, n_out: int, num: int, den: int, first_out: int = 0, first_src: int = 0) -> np.ndarray:
    """int64[n_out, n_src]: the weight of source index first_src + j (columns) in output index first_out + y (rows)."""
    y = (first_out + np.arange(n_out, dtype=np.int64))[:, None]
    j = (first_src + np.arange(n_src, dtype=np.int64))[None, :]
    return np.maximum(0, np.minimum((j + 1) * den, (y + 1) * num) - np.maximum(j * den, y * num))


def size(h: int, w: int, f) -> tuple:
    num, den = factor(f)
    return (h * den) // num, (w * den) // num


def source_rows(f, y0: int, y1: int) -> tuple:
    """The source indices [j0, j1) under the output indices [y0, y1)."""
    num, den = factor(f)
    return (y0 * num) // den, -((-y1 * num) // den)


def _along_axis0(a: np.ndarray, f, y0: int, y1: int, first_src: int = 0) -> np.ndarray:
    """int64[y1 - y0, k]: the weighted sums of int64[n, k] `a` (source indices first_src ..) for the output indices y0 .. y1 - 1."""
    num, den = factor(f)
    out = np.empty((y1 - y0, a.shape[1]), np.int64)
    for c0 in range(y0, y1, CHUNK):
        c1 = min(c0 + CHUNK, y1)
        j0, j1 = source_rows(f, c0, c1)
        assert first_src <= j0 and j1 - first_src <= a.shape[0]
        out[c0 - y0:c1 - y0] = weights(j1 - j0, c1 - c0, num, den, c0, j0) @ a[j0 - first_src:j1 - first_src]
    return out


def resample_rows(src_rows: np.ndarray, j0: int, f, y0: int, y1: int) -> np.ndarray:
    """Output rows [y0, y1), all columns, from the source rows j0 .. of the slide (at least source_rows(f, y0, y1))."""
    num, _ = factor(f)
    n, w = src_rows.shape[:2]
    ow = size(1, w, f)[1]
    s = _along_axis0(src_rows.astype(np.int64).reshape(n, w * 3), f, y0, y1, j0).reshape(y1 - y0, w, 3)
    s = _along_axis0(np.ascontiguousarray(s.transpose(1, 0, 2)).reshape(w, -1), f, 0, ow).reshape(ow, y1 - y0, 3).transpose(1, 0, 2)
    d = num * num
    return ((2 * s + d) // (2 * d)).astype(np.uint8)


def resample(a: np.ndarray, f) -> np.ndarray:
    """uint8[oh, ow, 3] of uint8[h, w, 3] `a`."""
    return resample_rows(a, 0, f, 0, size(a.shape[0], a.shape[1], f)[0])
