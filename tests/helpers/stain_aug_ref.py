"""NumPy restatement of the stain-jitter gather (dh_tile_gather_stain_aug) and the same jitter in plain
float64.  The restatement is int64 arithmetic on the tables of deephisto_amd.stain; the device results are compared with it bit
for bit."""
import numpy as np

from deephisto_amd import stain as S


def source_pixels(img, origins, P, flip_h=False, flip_v=False):
    """(uint8[n, P, P, 3] source bytes of every OUTPUT pixel, 0 outside the slide; bool[n, P, P] inside the slide)."""
    img = img if hasattr(img, "shape") else np.asarray(img)   # an array, or a virtual image (slide_scale.py): .shape and img[yy, xx]
    h, w = img.shape[:2]
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    r = np.arange(P)
    yy = o[:, 0, None] + (P - 1 - r if flip_v else r)[None, :]
    xx = o[:, 1, None] + (P - 1 - r if flip_h else r)[None, :]
    inside = ((yy >= 0) & (yy < h))[:, :, None] & ((xx >= 0) & (xx < w))[:, None, :]
    px = img[np.clip(yy, 0, h - 1)[:, :, None], np.clip(xx, 0, w - 1)[:, None, :]]
    return np.where(inside[..., None], px, 0).astype(np.uint8), inside


def raw_index(px, params):
    """int64[n, P, P, 3]: o_c >> shift before the clamp, o_c = A_c . T + b_c with tile t's row of int32[n, 12] `params`."""
    p = np.asarray(params, dtype=np.int64).reshape(len(px), 12)
    t = S.od_table().astype(np.int64)[px]
    o = np.einsum("ncd,nyxd->nyxc", p[:, :9].reshape(-1, 3, 3), t) + p[:, None, None, 9:]
    return o >> S.APPLY_SHIFT


def gather(img, origins, P, params, flip_h=False, flip_v=False, nchw=False):
    """float32[n, P, P, 3] (or [n, 3, P, P]): what the kernel writes, float32(v') / float32(255), exactly 0 outside the slide."""
    px, inside = source_pixels(img, origins, P, flip_h, flip_v)
    v = S.output_lut()[np.clip(raw_index(px, params), 0, S.LUT_SIZE - 1)]
    out = np.where(inside[..., None], v.astype(np.float32) / np.float32(255), np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if nchw else out


def plain(img, origins, P, flip_h=False, flip_v=False, nchw=False):
    """The un-jittered gather (dh_tile_gather_aug): float32(byte) / float32(255), 0 outside."""
    px, inside = source_pixels(img, origins, P, flip_h, flip_v)
    out = np.where(inside[..., None], px.astype(np.float32) / np.float32(255), np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if nchw else out


def jitter_float64(img, he, alpha, beta):
    """uint8 image: the jitter as it is usually coded, OD = -ln((v + 1) / 256), OD' = OD + HE ((alpha - 1) * pinv(HE) OD + beta),
    v' = clamp(round(256 exp(-OD')) - 1)."""
    he = np.asarray(he, dtype=np.float64)
    od = -np.log((np.asarray(img).reshape(-1, 3).astype(np.float64) + 1.0) / 256.0)
    c = od @ np.linalg.pinv(he).T
    od2 = od + ((np.asarray(alpha) - 1.0) * c + np.asarray(beta)) @ he.T
    return np.clip(np.rint(256.0 * np.exp(-od2)) - 1.0, 0, 255).astype(np.uint8).reshape(np.asarray(img).shape)
