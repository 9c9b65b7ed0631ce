"""Rotation and scale augmentation of training patches, fused into the batch gather.

Every patch gets its own angle `theta` and scale `s` (source pixels per output pixel: s > 1 zooms out) about its own centre.
The slide is resident in HBM, so the gather cuts the patch already rotated and rescaled, with real tissue in the corners, in
the pass that also does the `/255`, the layout, the flips and the stain jitter (`dh_tile_gather_affine_aug`).  The host side
below (the augmenter's private stream and the fixed-point parameter rows) needs no GPU.
"""
from __future__ import annotations

import numbers

import numpy as np

COEF_BITS = 15                  # m = round(2^15 s [[cos, -sin], [sin, cos]]): the doubled, centred coordinates carry the 16th bit
COEF_MAX = 1 << 16              # |m| <= 2^16, because s <= 2
FRAC_BITS = 16                  # source coordinates are Q16
WEIGHT_BITS = 8                 # bilinear weights: the top 8 fraction bits
SCALE_MIN, SCALE_MAX = 0.5, 2.0
MAX_PATCH = 4096                # |U2|, |V2| <= P - 1 < 2^12: every product m * U2 stays below 2^28


def overflow_bounds(patch: int = MAX_PATCH, side: int = 2 ** 31 - 1) -> dict:
    """Worst-case magnitude of every intermediate of the kernel for patches up to `patch` on a slide whose origins are any
    int32, as Python ints, each with the limit it has to stay below (beside stain.overflow_bounds, which covers the jitter)."""
    product = COEF_MAX * (patch - 1)                               # m * U2
    centre = (2 * side + patch) << COEF_BITS                       # |Cx|: needs int64
    return {
        "coef_product": (product, 2 ** 31),
        "centre": (centre, 2 ** 63),
        "source_coordinate": (centre + 2 * product, 2 ** 63),     # X, Y in Q16, compared with h and w before any narrowing
        "row_blend": (255 * 256, 2 ** 32),                         # a (256 - fx) + b fx
        "pixel_blend": (255 * 65536 + 32768, 2 ** 32),             # top (256 - fy) + bot fy + 2^15
    }


def _real(x, name, lo, hi):
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not lo <= float(x) <= hi:   # NaN fails the comparison too
        raise ValueError(f"{name} must be a number in [{lo}, {hi}], not {x!r}")
    return float(x)


def affine_params(theta_deg, s) -> np.ndarray:
    """int32[n, 4]: per tile m = round(2^15 s [[cos, -sin], [sin, cos]]) row-major (m00, m01, m10, m11); `theta_deg` in degrees,
    `s` in [0.5, 2] source pixels per output pixel.  theta = 0, s = 1 gives exactly (32768, 0, 0, 32768); theta = 90, s = 1
    gives (0, -32768, 32768, 0), an exact quarter turn."""
    theta = np.atleast_1d(np.asarray(theta_deg, dtype=np.float64))
    s = np.atleast_1d(np.asarray(s, dtype=np.float64))
    if theta.ndim != 1 or s.ndim != 1:
        raise ValueError(f"theta_deg and s must be scalars or float64[n], not {list(theta.shape)} and {list(s.shape)}")
    theta, s = np.broadcast_arrays(theta, s)
    if not np.all(np.isfinite(theta)):
        raise ValueError("theta_deg must be finite")
    if not np.all((s >= SCALE_MIN) & (s <= SCALE_MAX)):   # NaN fails too
        raise ValueError(f"s must lie in [{SCALE_MIN}, {SCALE_MAX}] (source pixels per output pixel)")
    rad = np.deg2rad(theta)
    c, sn = s * np.cos(rad), s * np.sin(rad)
    m = np.rint(np.stack([c, -sn, sn, c], 1) * (1 << COEF_BITS))
    return np.clip(m, -COEF_MAX, COEF_MAX).astype(np.int32)   # |s cos| <= 2: the clip never moves a value


IDENTITY_ROW = (1 << COEF_BITS, 0, 0, 1 << COEF_BITS)


class GeometricAugmenter:
    """Per-patch rotation and magnification jitter for training: theta ~ U(-rotate_deg, rotate_deg) degrees and
    s ~ U(scale[0], scale[1]) source pixels per output pixel, about the patch's own centre.  The draws come from a private
    PCG64 stream: NumPy's and torch's global streams, which carry the samplers' reference-exact order and the flip coins, are
    never touched, and neither is a StainAugmenter's stream."""

    def __init__(self, rotate_deg: float = 180.0, scale=(1.0, 1.0), seed: int = 0):
        self.rotate_deg = _real(rotate_deg, "rotate_deg", 0.0, 180.0)
        try:
            lo, hi = scale
        except (TypeError, ValueError):
            raise ValueError(f"scale must be a (min, max) pair with {SCALE_MIN} <= min <= max <= {SCALE_MAX}, not {scale!r}") from None
        lo, hi = _real(lo, "scale[0]", SCALE_MIN, SCALE_MAX), _real(hi, "scale[1]", SCALE_MIN, SCALE_MAX)
        if lo > hi:
            raise ValueError(f"scale must be a (min, max) pair with {SCALE_MIN} <= min <= max <= {SCALE_MAX}, not {scale!r}")
        self.scale = (lo, hi)
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError(f"seed must be a non-negative integer, not {seed!r}")
        self.seed = int(seed)
        self._rng = np.random.Generator(np.random.PCG64(self.seed))

    def __repr__(self):
        return f"GeometricAugmenter(rotate_deg={self.rotate_deg}, scale={self.scale}, seed={self.seed})"

    def draw(self, n: int) -> tuple[np.ndarray, np.ndarray]:
        """(theta_deg float64[n], s float64[n]) from one uniform draw of n x 2 numbers, columns (theta, s)."""
        u = self._rng.uniform(size=(int(n), 2))
        return self.rotate_deg * (2.0 * u[:, 0] - 1.0), self.scale[0] + (self.scale[1] - self.scale[0]) * u[:, 1]

    def rows(self, n: int) -> np.ndarray:
        """int32[n, 4]: `affine_params` of one `draw(n)`."""
        return affine_params(*self.draw(n))
