"""Macenko stain normalisation of an HBM-resident slide, integer-exact on the device.

The method is Macenko et al. (2009) with the usual constants, restated so that everything a pixel contributes is an integer:
optical density comes from a 256-entry fixed-point table, the stained-pixel moments, the angle histogram, the two concentration
histograms and the applied slide are integer functions of the bytes (csrc/stain.hip), and the handful of numbers in between
(covariance, eigenvectors, percentiles, pseudo-inverse, the 3 x 3 matrix) are float64 on the host, computed from exact integers
with IEEE operations only (+ - * / sqrt, cos and sin of the table angles), so every rank of a sharded run computes the same.

The host math below (table builders, fit from moments, percentile from a histogram, the matrix) needs no GPU.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import numbers
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from .geom_aug import overflow_bounds as _affine_overflow_bounds

# ---- fixed-point widths and bin counts -------------------------------------------------------------
OD_BITS = 12                    # optical density: T[v] = round(-ln((v + 1) / 256) * 2^12), 0 .. 22713
OD_MAX = 22713                  # T[0] = round(ln(256) * 4096)
EVEC_BITS = 14                  # eigenvector components: round(e * 2^14), |.| <= 2^14
DIR_BITS = 14                   # bin-boundary directions: round((cos, sin) * 2^14)
ANGLE_BINS = 1024               # over the full circle [-pi, pi): 0.3516 degrees each
COEF_BITS = 12                  # pseudo-inverse and apply matrix: round(m * 2^12)
COEF_MAX = 1 << 19              # |fixed-point entry| the kernels accept (|m| <= 128)
CONC_BINS = 2048                # per stain
CONC_SHIFT = OD_BITS + COEF_BITS - 8    # bin width 2^-8 = 0.0039; the last bin collects c >= 8 - 2^-8, the first c < 2^-8
CONC_WIDTH = 2.0 ** -8
APPLY_SHIFT = COEF_BITS         # OD' index in units of 2^-12
BIAS_BITS = OD_BITS + COEF_BITS # the jitter's bias, in the units of matrix x table
BIAS_MAX = 1 << 30              # |fixed-point bias| the jitter gather accepts (|b| <= 64 in optical density)
LUT_SIZE = 24576                # OD' in [0, 6): v' = 0 from OD' = ln(512 / 3) = 5.14 on
MIN_STAINED = 16                # fewer stained pixels: identity fit
MAX_PIXELS = (2 ** 63 - 1) // (OD_MAX * OD_MAX)   # 17 878 897 106 pixels: the 64-bit product sums cannot overflow below it
MIN_EIGENVALUE = 1e-10          # OD^2: a second eigenvalue at or below it is a degenerate plane (one colour, one stain line)
MIN_DET = 1e-6                  # det(HE^T HE) = sin^2 of the angle between the stain vectors

TARGET_HE = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))
TARGET_MAXC = (1.9705, 1.0308)


def od_table() -> np.ndarray:
    """int32[256]: T[v] = round(-ln((v + 1) / 256) * 2^OD_BITS); T[255] = 0, decreasing in v."""
    v = np.arange(256, dtype=np.float64)
    t = np.rint(-np.log((v + 1.0) / 256.0) * (1 << OD_BITS)).astype(np.int32)
    t[255] = 0
    return t


def stained_vmax(beta: float) -> int:
    """The largest byte value whose float64 optical density is >= beta (-1: none).  OD decreases in v, so a pixel is stained
    (all three channel ODs >= beta) exactly when max(R, G, B) <= stained_vmax(beta)."""
    v = np.arange(256, dtype=np.float64)
    ok = np.nonzero(-np.log((v + 1.0) / 256.0) >= beta)[0]
    return int(ok[-1]) if len(ok) else -1


def angle_boundaries() -> np.ndarray:
    """int32[ANGLE_BINS, 2]: direction (x, y) = round((cos, sin)(theta_k) * 2^DIR_BITS) of the lower edge theta_k = -pi +
    2 pi k / ANGLE_BINS of bin k.  One quadrant is computed and rotated by exact quarter turns, so entry 256 q is the axis."""
    n4 = ANGLE_BINS // 4
    a = np.arange(n4, dtype=np.float64) * (2.0 * math.pi / ANGLE_BINS)
    x = np.rint(np.cos(a) * (1 << DIR_BITS)).astype(np.int32)
    y = np.rint(np.sin(a) * (1 << DIR_BITS)).astype(np.int32)
    return np.concatenate([np.stack([-x, -y], 1), np.stack([y, -x], 1), np.stack([x, y], 1), np.stack([-y, x], 1)]).astype(np.int32)


def output_lut() -> np.ndarray:
    """uint8[LUT_SIZE]: v' = clamp(round(256 exp(-OD')) - 1, 0, 255) at the centre OD' = (k + 0.5) / 2^12 of entry k."""
    od = (np.arange(LUT_SIZE, dtype=np.float64) + 0.5) / (1 << APPLY_SHIFT)
    return np.clip(np.rint(256.0 * np.exp(-od)) - 1.0, 0, 255).astype(np.uint8)


def overflow_bounds(npix: int = MAX_PIXELS) -> dict:
    """Worst-case magnitude of every accumulator and product of the kernels on a slide of `npix` pixels, over all 8-bit inputs
    (all-black pixels: every channel OD_MAX), as Python ints, each with the limit it has to stay below."""
    proj = 3 * (1 << EVEC_BITS) * OD_MAX                      # |E . T|, every component at its cap
    return {
        "count": (npix, 2 ** 63),
        "sum": (npix * OD_MAX, 2 ** 63),
        "product_sum": (npix * OD_MAX * OD_MAX, 2 ** 63),
        "lane_product": (OD_MAX * OD_MAX, 2 ** 32),            # formed as uint32 x uint32 -> uint64
        "projection": (proj, 2 ** 31),                         # int32
        "cross_product": (2 * (1 << DIR_BITS) * proj, 2 ** 63),
        "concentration": (3 * COEF_MAX * OD_MAX, 2 ** 63),
        "applied_od": (3 * COEF_MAX * OD_MAX, 2 ** 63),
        "jittered_od": (3 * COEF_MAX * OD_MAX + BIAS_MAX, 2 ** 63),   # the jitter gather: matrix . T + bias (section 4.12)
        "histogram_bin": (npix, 2 ** 64),
        # an LDS copy is shared by at most one workgroup of a grid of 2 048 (or every lane has one group of 16 pixels)
        "lds_bin": (npix // 2048 + 16 * 256 + 16, 2 ** 32),
        # the rotated and rescaled gather in front of the jitter (section 4.13): coordinates and the bilinear blend
        **{f"affine_{k}": v for k, v in _affine_overflow_bounds().items()},
    }


def percentile_from_hist(hist, q: float, lo: float, width: float) -> float:
    """The q-th percentile of the values counted in `hist` (bin k covers [lo + k width, lo + (k + 1) width)).

    Rule, on integer cumulative counts: with n = sum(hist), the target rank is t = min(n, max(1, ceil(q n / 100))) (exact
    rational arithmetic on q as given); the bin is the smallest k whose cumulative count reaches t; the value is
    lo + width * (k + (t - before - 0.5) / hist[k]) with `before` the cumulative count below bin k: the t-th value, had the
    bin's values been spread evenly over it."""
    h = [int(v) for v in np.asarray(hist).reshape(-1)]
    n = sum(h)
    if n <= 0 or min(h) < 0:
        raise ValueError("hist must hold non-negative counts, at least one of them positive")
    t = min(n, max(1, math.ceil(Fraction(q) * n / 100)))
    before = 0
    for k, c in enumerate(h):
        if before + c >= t:
            return lo + width * (k + (t - before - 0.5) / c)
        before += c
    raise AssertionError("unreachable")


def _jacobi_eigh3(a):
    """Eigenvalues (descending) and unit eigenvectors (rows) of a symmetric 3 x 3 matrix by cyclic Jacobi rotations: float64
    + - * / sqrt only, so the result is the same bits wherever it runs."""
    a = [[float(a[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(64):
        off = a[0][1] ** 2 + a[0][2] ** 2 + a[1][2] ** 2
        if off <= 1e-300 or off <= 1e-32 * (a[0][0] ** 2 + a[1][1] ** 2 + a[2][2] ** 2):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if a[p][q] == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                akp, akq = a[k][p], a[k][q]
                a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
            for k in range(3):
                apk, aqk = a[p][k], a[q][k]
                a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    order = sorted(range(3), key=lambda i: (-a[i][i], i))
    return [a[i][i] for i in order], [[v[k][i] for k in range(3)] for i in order]


def plane_from_moments(moments) -> tuple[np.ndarray | None, list]:
    """(int32[2, 3] fixed-point eigenvectors of the two largest eigenvalues of the OD covariance, or None for a degenerate
    plane; the three eigenvalues in OD^2).  `moments`: the ten integers of dh_stain_moments.  The covariance entries are
    (n S_ij - S_i S_j) / (n (n - 1)) / 2^24, the numerator an exact integer.  Sign rule: an eigenvector whose fixed-point dot
    product with the channel sums (S_r, S_g, S_b) is negative is negated, so both mean projections are >= 0 and the stained
    pixels' angles gather around the first quadrant, away from the cut of the circle at +-pi."""
    m = [int(x) for x in moments]
    n, s, prod = m[0], m[1:4], {(0, 0): m[4], (0, 1): m[5], (0, 2): m[6], (1, 1): m[7], (1, 2): m[8], (2, 2): m[9]}
    if n < 2:
        return None, [0.0, 0.0, 0.0]
    scale = float(1 << (2 * OD_BITS))
    cov = [[((n * prod[(min(i, j), max(i, j))] - s[i] * s[j]) / (n * (n - 1))) / scale for j in range(3)] for i in range(3)]
    lam, vec = _jacobi_eigh3(cov)
    if not all(math.isfinite(x) for x in lam) or lam[1] <= MIN_EIGENVALUE:
        return None, lam
    eq = np.array([[int(round(c * (1 << EVEC_BITS))) for c in vec[k]] for k in range(2)], dtype=np.int64)
    for k in range(2):
        if sum(int(eq[k, c]) * s[c] for c in range(3)) < 0:
            eq[k] = -eq[k]
    return eq.astype(np.int32), lam


def stain_vectors(evec_q: np.ndarray, phi_min: float, phi_max: float) -> np.ndarray | None:
    """float64[3, 2] unit stain vectors from the two extreme angles in the plane of the fixed-point eigenvectors; the one with
    the larger red component is haematoxylin and comes first.  None when they are (nearly) parallel."""
    e = np.asarray(evec_q, dtype=np.float64) / (1 << EVEC_BITS)
    cols = []
    for phi in (phi_min, phi_max):
        v = e[0] * math.cos(phi) + e[1] * math.sin(phi)
        nv = math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        if nv == 0.0:
            return None
        cols.append(v / nv)
    if cols[0][0] < cols[1][0]:
        cols.reverse()
    he = np.stack(cols, 1)
    return he if _gram_det(he) > MIN_DET else None


def _gram_det(he) -> float:
    a, b, d = float(he[:, 0] @ he[:, 0]), float(he[:, 0] @ he[:, 1]), float(he[:, 1] @ he[:, 1])
    return a * d - b * b


def pinv32(he) -> np.ndarray:
    """float64[2, 3]: (HE^T HE)^-1 HE^T in closed form."""
    he = np.asarray(he, dtype=np.float64).reshape(3, 2)
    a, b, d = float(he[:, 0] @ he[:, 0]), float(he[:, 0] @ he[:, 1]), float(he[:, 1] @ he[:, 1])
    det = a * d - b * b
    return np.stack([(d * he[:, 0] - b * he[:, 1]) / det, (a * he[:, 1] - b * he[:, 0]) / det])


def quantize_coef(m, what: str) -> np.ndarray:
    """int32 fixed-point copy round(m * 2^COEF_BITS); an entry beyond COEF_MAX is refused by name."""
    q = np.rint(np.asarray(m, dtype=np.float64) * (1 << COEF_BITS))
    if not np.all(np.isfinite(q)) or np.abs(q).max() > COEF_MAX:
        raise ValueError(f"{what}: an entry exceeds {COEF_MAX >> COEF_BITS} in magnitude (stain vectors too close to parallel?)")
    return q.astype(np.int32)


def jitter_params(he, alpha, beta) -> np.ndarray:
    """int32[n, 12]: per tile the fixed-point matrix A = I + HE diag(alpha - 1) pinv(HE) (9 entries, row-major, 2^COEF_BITS) and
    bias b = HE beta (3 entries, 2^BIAS_BITS) of the stain jitter OD' = A OD + b = OD + HE ((alpha - 1) * c + beta) with
    c = pinv(HE) OD the pixel's two concentrations.  `he`: the slide's 3 x 2 stain basis, haematoxylin
    first; `alpha`, `beta`: float64[n, 2].  alpha = 1, beta = 0 gives exactly (2^COEF_BITS I, 0)."""
    he = np.asarray(he, dtype=np.float64)
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    if he.shape != (3, 2) or not np.all(np.isfinite(he)):
        raise ValueError("he must be a finite 3 x 2 stain basis")
    if alpha.ndim != 2 or alpha.shape[1] != 2 or beta.shape != alpha.shape:
        raise ValueError(f"alpha and beta must both be float64[n, 2], not {list(alpha.shape)} and {list(beta.shape)}")
    n = alpha.shape[0]
    out = np.empty((n, 12), dtype=np.int32)
    if n == 0:
        return out
    pinv = pinv32(he)
    a = np.eye(3)[None] + np.einsum("ck,nk,kd->ncd", he, alpha - 1.0, pinv)
    out[:, :9] = quantize_coef(a, "jitter matrix").reshape(n, 9)
    b = np.rint((beta @ he.T) * (1 << BIAS_BITS))
    if not np.all(np.isfinite(b)) or np.abs(b).max() > BIAS_MAX:
        raise ValueError(f"jitter bias: an entry exceeds {BIAS_MAX >> BIAS_BITS} in magnitude")
    out[:, 9:] = b.astype(np.int32)
    return out


class StainAugmenter:
    """Per-patch stain jitter for training (Tellez et al. 2018, in the slide's own Macenko basis): every patch's haematoxylin
    and eosin concentrations c become alpha * c + beta with alpha ~ U(1 - sigma_alpha, 1 + sigma_alpha) and
    beta ~ U(-sigma_beta, sigma_beta) per stain.  The draws come from a private PCG64 stream: NumPy's and torch's global
    streams, which carry the samplers' reference-exact order and the flip coins, are never touched."""

    def __init__(self, sigma_alpha: float = 0.2, sigma_beta: float = 0.0, seed: int = 0):
        self.sigma_alpha = _real(sigma_alpha, "sigma_alpha", 0.0, 0.9)
        self.sigma_beta = _real(sigma_beta, "sigma_beta", 0.0, 0.5)
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError(f"seed must be a non-negative integer, not {seed!r}")
        self.seed = int(seed)
        self._rng = np.random.Generator(np.random.PCG64(self.seed))

    def __repr__(self):
        return f"StainAugmenter(sigma_alpha={self.sigma_alpha}, sigma_beta={self.sigma_beta}, seed={self.seed})"

    def draw(self, n: int) -> tuple[np.ndarray, np.ndarray]:
        """(alpha float64[n, 2], beta float64[n, 2]) from one uniform draw of n x 4 numbers, columns (aH, aE, bH, bE)."""
        u = 2.0 * self._rng.uniform(size=(int(n), 4)) - 1.0
        return 1.0 + self.sigma_alpha * u[:, :2], self.sigma_beta * u[:, 2:]


def stain_basis(slide, stain=None, fit=None):
    """float64[3, 2] basis in which `slide`'s patches are jittered, or None when the slide has none (identity fit: all glass, a
    degenerate plane).  `slide` as it is resident: after `stain` (a StainNormalizer) mapped it, with `fit` the fit that
    normalisation found, the basis is the normaliser's target; otherwise one default Macenko fit of the slide."""
    if stain is not None:
        return None if fit is None or fit.identity else np.array(stain.target_he, dtype=np.float64)
    f = StainNormalizer().fit(slide)
    return None if f.identity else np.array(f.HE, dtype=np.float64)


@dataclass
class StainFit:
    """What `StainNormalizer.fit` learns about a slide.  `identity`: too few stained pixels or a degenerate plane (all glass,
    one colour): `apply` returns the pixels unchanged, and HE / maxC are None."""
    HE: list | None                 # 3 x 2, unit columns, haematoxylin first
    maxC: list | None               # 2: the 99th percentile of each concentration over the stained pixels
    n_stained: int
    moments: list                   # the ten integers of dh_stain_moments
    angle_min: float | None
    angle_max: float | None
    identity: bool = False
    reason: str = ""
    beta: float = 0.15
    alpha: float = 1.0
    eigenvalues: list = field(default_factory=list)

    def to_json(self) -> str:
        return json.dumps({k: getattr(self, k) for k in self.__dataclass_fields__})

    @classmethod
    def from_json(cls, text: str) -> "StainFit":
        d = json.loads(text)
        unknown = set(d) - set(cls.__dataclass_fields__)
        if unknown:
            raise ValueError(f"not a StainFit: unknown fields {sorted(unknown)}")
        return cls(**d)


def _identity_fit(moments, reason, beta, alpha, lam=()) -> StainFit:
    return StainFit(None, None, int(moments[0]), [int(x) for x in moments], None, None, True, reason, beta, alpha, list(lam))


def apply_matrix(fit: StainFit, target_he=TARGET_HE, target_maxc=TARGET_MAXC) -> np.ndarray:
    """float64[3, 3]: HE_target diag(maxC_target / maxC) pinv(HE), the map from a pixel's OD to its normalised OD."""
    he_t = np.asarray(target_he, dtype=np.float64).reshape(3, 2)
    ratio = np.asarray(target_maxc, dtype=np.float64).reshape(2) / np.asarray(fit.maxC, dtype=np.float64)
    return (he_t * ratio[None, :]) @ pinv32(fit.HE)


def _check_target(target):
    if target is None:
        return np.array(TARGET_HE, dtype=np.float64), np.array(TARGET_MAXC, dtype=np.float64)
    if isinstance(target, StainFit):
        if target.identity:
            raise ValueError(f"target must not be an identity StainFit ({target.reason})")
        target = (target.HE, target.maxC)
    try:
        he, mc = target
        he, mc = np.array(he, dtype=np.float64), np.array(mc, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"target must be None, a StainFit or a (HE 3x2, maxC 2) pair, not {target!r}") from None
    if he.shape != (3, 2) or mc.shape != (2,) or not np.all(np.isfinite(he)) or not np.all(np.isfinite(mc)) or np.any(mc <= 0):
        raise ValueError("target must be None, a StainFit or a (HE 3x2, maxC 2) pair of finite numbers with maxC > 0")
    return he, mc


# ---- device entries ---------------------------------------------------------------------------------------------------------
_TABLES: dict = {}


def _tables(dev):
    """(od table, boundary table, output lut) on `dev`, uploaded once, and the od table on the host for the entries' check."""
    import torch
    key = (dev.type, dev.index)
    if key not in _TABLES:
        od = od_table()
        _TABLES[key] = (torch.from_numpy(od).to(dev), torch.from_numpy(angle_boundaries()).to(dev),
                        torch.from_numpy(output_lut()).to(dev), od)
    return _TABLES[key]


def _slide(slide):
    from .tissue import _check_slide
    slide = _check_slide(slide)
    if not slide.is_contiguous():
        slide = slide.contiguous()
        if slide.data_ptr() % 16:
            slide = _aligned_copy(slide)
    npix = int(slide.shape[0]) * int(slide.shape[1])
    if npix == 0:
        raise ValueError("slide is empty")
    if npix > MAX_PIXELS:
        raise ValueError(f"slide of {npix} pixels exceeds max_pixels = {MAX_PIXELS}: the 64-bit product sums could overflow")
    return slide


def _aligned_copy(t):
    import torch
    return torch.empty_like(t, memory_format=torch.contiguous_format).copy_(t)


def _i32(a, shape):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != shape:
        raise ValueError(f"expected int32{list(shape)}, got {list(a.shape)}")
    return a


def stain_moments(slide, vmax: int) -> np.ndarray:
    """np.uint64[10] over the pixels with max(R, G, B) <= vmax: count, 3 sums and 6 product sums of T (synchronises)."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    slide = _slide(slide)
    od_dev, _, _, od = _tables(slide.device)
    out = torch.empty(10, dtype=torch.int64, device=slide.device)
    check(lib().dh_stain_moments(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), od_dev.data_ptr(),
                                 od.ctypes.data_as(C.c_void_p), int(vmax), out.data_ptr(), _stream(slide.device)),
          "dh_stain_moments")
    return out.cpu().numpy().view(np.uint64)


def angle_histogram(slide, vmax: int, evec_q) -> np.ndarray:
    """np.uint64[ANGLE_BINS]: angle bins of the stained pixels' projections onto the fixed-point eigenvectors (synchronises)."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    slide = _slide(slide)
    e = _i32(evec_q, (2, 3))
    od_dev, dirs, _, od = _tables(slide.device)
    out = torch.empty(ANGLE_BINS, dtype=torch.int64, device=slide.device)
    check(lib().dh_stain_angle_hist(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), od_dev.data_ptr(),
                                    od.ctypes.data_as(C.c_void_p), int(vmax), e.ctypes.data_as(C.c_void_p), dirs.data_ptr(),
                                    ANGLE_BINS, out.data_ptr(), _stream(slide.device)), "dh_stain_angle_hist")
    return out.cpu().numpy().view(np.uint64)


def conc_histogram(slide, vmax: int, pinv_q) -> np.ndarray:
    """np.uint64[2, CONC_BINS]: per stain, the concentration bins of the stained pixels (synchronises)."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    slide = _slide(slide)
    p = _i32(pinv_q, (2, 3))
    od_dev, _, _, od = _tables(slide.device)
    out = torch.empty((2, CONC_BINS), dtype=torch.int64, device=slide.device)
    check(lib().dh_stain_conc_hist(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), od_dev.data_ptr(),
                                   od.ctypes.data_as(C.c_void_p), int(vmax), p.ctypes.data_as(C.c_void_p), CONC_SHIFT, CONC_BINS,
                                   out.data_ptr(), _stream(slide.device)), "dh_stain_conc_hist")
    return out.cpu().numpy().view(np.uint64)


def apply_fixed(slide, matrix_q, out=None):
    """uint8[h, w, 3] on the device: every pixel through the fixed-point 3 x 3 matrix and the output table.  `out` may be the
    slide itself."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    if out is not None and (out.shape != slide.shape or out.dtype != torch.uint8 or out.device != slide.device):
        raise ValueError("out must be a uint8 tensor of the slide's shape on its device")
    src = _slide(slide)
    m = _i32(matrix_q, (3, 3))
    direct = out is not None and out.is_contiguous() and out.data_ptr() % 16 == 0 and (src is slide or out is not slide)
    dst = out if direct else (src if src is not slide else torch.empty_like(src))   # a private copy is normalised in place
    od_dev, _, lut, od = _tables(src.device)
    check(lib().dh_stain_apply(src.data_ptr(), int(src.shape[0]), int(src.shape[1]), od_dev.data_ptr(),
                               od.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), APPLY_SHIFT, lut.data_ptr(), LUT_SIZE,
                               dst.data_ptr(), _stream(src.device)), "dh_stain_apply")
    if out is None:
        return dst
    if not direct:
        out.copy_(dst)
    return out


def _real(x, name, lo, hi, hi_open=False):
    if (isinstance(x, bool) or not isinstance(x, numbers.Real) or not (lo <= float(x) < hi if hi_open else lo <= float(x) <= hi)):
        raise ValueError(f"{name} must be a number in [{lo}, {hi}{')' if hi_open else ']'}, not {x!r}")   # NaN fails the comparison too
    return float(x)


class StainNormalizer:
    """Opt-in stain normalisation of a resident slide.

    `method`: "macenko".  `beta` in [0, ln 256]: a pixel is stained when all three channel optical densities are >= beta.
    `alpha` in [0, 50): the stain vectors are the `alpha` and `100 - alpha` percentiles of the stained pixels' angles in the
    plane of the two leading eigenvectors.  `target`: None (the widely used constants TARGET_HE / TARGET_MAXC), a StainFit
    (another slide's fit) or a (HE 3 x 2, maxC 2) pair."""

    def __init__(self, method: str = "macenko", beta: float = 0.15, alpha: float = 1.0, target=None):
        if method != "macenko":
            raise ValueError(f"method must be 'macenko', not {method!r}")
        self.method = method
        self.beta = _real(beta, "beta", 0.0, math.log(256.0))
        self.alpha = _real(alpha, "alpha", 0.0, 50.0, hi_open=True)
        self.target_he, self.target_maxc = _check_target(target)
        self.vmax = stained_vmax(self.beta)

    def __repr__(self):
        return f"StainNormalizer(method={self.method!r}, beta={self.beta}, alpha={self.alpha})"

    def fit(self, slide) -> StainFit:
        """The three statistics passes and the host math between them (three read-backs)."""
        return fit_with(lambda: stain_moments(slide, self.vmax), lambda e: angle_histogram(slide, self.vmax, e),
                        lambda p: conc_histogram(slide, self.vmax, p), self.beta, self.alpha)

    def matrix_q(self, fit: StainFit) -> np.ndarray:
        """int32[3, 3]: the fixed-point matrix `apply` hands to the kernel."""
        return quantize_coef(apply_matrix(fit, self.target_he, self.target_maxc), "apply matrix")

    def apply(self, slide, fit: StainFit, out=None):
        """uint8[h, w, 3] on the device: `slide` mapped onto the target appearance (every pixel, glass included); the pixels
        unchanged under an identity fit.  `out`: where to write; it may be `slide` itself."""
        if fit.identity:
            if out is None:
                return slide.clone()
            if out is not slide:
                out.copy_(slide)
            return out
        return apply_fixed(slide, self.matrix_q(fit), out)

    def normalize(self, slide, info: dict | None = None):
        fit = self.fit(slide)
        if info is not None:
            info["fit"] = fit
        return self.apply(slide, fit)


def fit_with(moments_fn, angle_hist_fn, conc_hist_fn, beta: float = 0.15, alpha: float = 1.0) -> StainFit:
    """The fit as a function of the three integer statistics, each fetched by a callable (the device entries above, or a NumPy
    restatement in the tests): moments -> plane -> angle histogram -> stain vectors -> concentration histograms -> maxC."""
    mom = [int(x) for x in moments_fn()]
    if mom[0] < MIN_STAINED:
        return _identity_fit(mom, f"{mom[0]} stained pixels, fewer than {MIN_STAINED}", beta, alpha)
    evec_q, lam = plane_from_moments(mom)
    if evec_q is None:
        return _identity_fit(mom, "degenerate stain plane", beta, alpha, lam)
    hist = angle_hist_fn(evec_q)
    lo, width = -math.pi, 2.0 * math.pi / ANGLE_BINS
    phi_min = percentile_from_hist(hist, alpha, lo, width)
    phi_max = percentile_from_hist(hist, 100.0 - alpha, lo, width)
    he = stain_vectors(evec_q, phi_min, phi_max)
    if he is None:
        return _identity_fit(mom, "stain vectors are parallel", beta, alpha, lam)
    try:
        pinv_q = quantize_coef(pinv32(he), "pseudo-inverse")
    except ValueError as e:
        return _identity_fit(mom, str(e), beta, alpha, lam)
    chist = np.asarray(conc_hist_fn(pinv_q)).reshape(2, CONC_BINS)
    maxc = [percentile_from_hist(chist[s], 99.0, 0.0, CONC_WIDTH) for s in range(2)]
    if min(maxc) <= CONC_WIDTH:
        return _identity_fit(mom, "a stain has no concentration", beta, alpha, lam)
    return StainFit(he.tolist(), maxc, mom[0], mom, phi_min, phi_max, False, "", beta, alpha, list(lam))
