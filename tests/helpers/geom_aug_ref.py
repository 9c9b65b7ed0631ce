"""NumPy restatement of the rotated and rescaled gather (dh_tile_gather_affine_aug) in int64, and the
same window sampled bilinearly in plain float64.  The device results are compared with the restatement bit for bit; with stain
parameter rows it chains the restatement of the jitter in stain_aug_ref.py."""
import numpy as np

import stain_aug_ref as A

from deephisto_amd import stain as S


def coordinates(origins, P, rows, flip_h=False, flip_v=False):
    """int64[n, P, P] X and Y in Q16 of every OUTPUT pixel: X = Cx + m00 U2 + m01 V2, Y = Cy + m10 U2 + m11 V2 with the flips
    applied first, U2 = 2 sx + 1 - P, V2 = 2 sr + 1 - P, Cx = ((2 x0 + P) << 15) - 2^15."""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    m = np.asarray(rows, dtype=np.int64).reshape(len(o), 4)
    k = np.arange(P, dtype=np.int64)
    u2 = (2 * (P - 1 - k if flip_h else k) + 1 - P)[None, None, :]
    v2 = (2 * (P - 1 - k if flip_v else k) + 1 - P)[None, :, None]
    cy = (((2 * o[:, 0] + P) << 15) - (1 << 15))[:, None, None]
    cx = (((2 * o[:, 1] + P) << 15) - (1 << 15))[:, None, None]
    x = cx + m[:, 0, None, None] * u2 + m[:, 1, None, None] * v2
    y = cy + m[:, 2, None, None] * u2 + m[:, 3, None, None] * v2
    return x, y


def _tap(img, yy, xx):
    """int64[..., 3]: the bytes at integer positions (yy, xx), 0 outside the image."""
    h, w = img.shape[:2]
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    px = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
    return np.where(inside[..., None], px, 0), inside


def blend(img, origins, P, rows, flip_h=False, flip_v=False):
    """(uint8[n, P, P, 3] the interpolated value v of every output pixel; bool[n, P, P]: a tap of non-zero weight lies inside the
    slide -- the others are written as 0 and not transformed)."""
    img = img if hasattr(img, "shape") else np.asarray(img)   # an array, or a virtual image (slide_scale.py): .shape and img[yy, xx]
    x, y = coordinates(origins, P, rows, flip_h, flip_v)
    xi, yi = x >> 16, y >> 16                                   # arithmetic shifts: floor
    fx, fy = ((x >> 8) & 255)[..., None], ((y >> 8) & 255)[..., None]
    (a, ia), (b, ib) = _tap(img, yi, xi), _tap(img, yi, xi + 1)
    (c, ic), (d, id_) = _tap(img, yi + 1, xi), _tap(img, yi + 1, xi + 1)
    top, bot = a * (256 - fx) + b * fx, c * (256 - fx) + d * fx
    v = (top * (256 - fy) + bot * fy + 32768) >> 16
    assert v.min() >= 0 and v.max() <= 255
    nx, ny = fx[..., 0] > 0, fy[..., 0] > 0
    live = ia | (nx & ib) | (ny & ic) | (nx & ny & id_)
    return v.astype(np.uint8), live


def gather(img, origins, P, rows, flip_h=False, flip_v=False, nchw=False, params=None):
    """float32[n, P, P, 3] (or [n, 3, P, P]): what the kernel writes.  `params` None: float32(v) / float32(255); int32[n, 12]
    rows of stain.jitter_params: v through the jitter chain first.  Exactly 0 where no tap of non-zero weight is inside."""
    v, live = blend(img, origins, P, rows, flip_h, flip_v)
    if params is not None:
        v = S.output_lut()[np.clip(A.raw_index(v, params), 0, S.LUT_SIZE - 1)]
    out = np.where(live[..., None], v.astype(np.float32) / np.float32(255), np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if nchw else out


def sample_float64(img, origins, P, theta_deg, s):
    """(float64[n, P, P, 3] plain bilinear samples of the zero-extended image at the un-quantised points
    x = x0 + P/2 - 1/2 + s (cos U - sin V), y = y0 + P/2 - 1/2 + s (sin U + cos V), U = sx + 1/2 - P/2, V = sr + 1/2 - P/2;
    the float64 (x, y) themselves)."""
    img = np.asarray(img)
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 2)
    th = np.deg2rad(np.asarray(theta_deg, dtype=np.float64)).reshape(-1, 1, 1)
    s = np.asarray(s, dtype=np.float64).reshape(-1, 1, 1)
    k = np.arange(P, dtype=np.float64) + 0.5 - P / 2.0
    u, v = k[None, None, :], k[None, :, None]
    x = o[:, 1, None, None] + P / 2.0 - 0.5 + s * (np.cos(th) * u - np.sin(th) * v)
    y = o[:, 0, None, None] + P / 2.0 - 0.5 + s * (np.sin(th) * u + np.cos(th) * v)
    xi, yi = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - xi)[..., None], (y - yi)[..., None]
    a, b = _tap(img, yi, xi)[0], _tap(img, yi, xi + 1)[0]
    c, d = _tap(img, yi + 1, xi)[0], _tap(img, yi + 1, xi + 1)[0]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy, x, y
