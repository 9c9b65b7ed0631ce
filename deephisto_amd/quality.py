"""Tile quality for whole-slide prediction: skip out-of-focus and ink-marked tiles.

Per pixel (R, G, B): luma `Y = (77 R + 150 G + 29 B + 128) >> 8`; chroma `c = max - min`; tissue when `c > t` (the tissue
filter's rule; `t = -1`: every pixel); ink when `(c > ink_chroma and G - min(R, B) >= ink_margin) or max(R, G, B) <= dark_max`.
`L = 4 Y - the four neighbours' Y` (a neighbour outside the slide is the edge pixel).  Per tile: `n_t` tissue pixels, `S1` and
`S2` = the sums of `L` and `L*L` over them, `n_ink` ink pixels.  A tile's sharpness is the variance of `L` over its tissue
pixels, `(n_t*S2 - S1*S1) / n_t^2`; it is rejected as blurred (reason bit 2) when that lies below `min_sharpness`, and as
ink-marked (bit 4) when `n_ink > floor(max_ink_fraction * P * P)`.  The sums, the flags and the compaction run in
libdeephisto_hip.so (csrc/quality.hip, csrc/quality_rule.h); everything is integer-exact, so every rank of a sharded run
computes the same kept list.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np
import torch

from ._lib import check, lib
from .tiles import _require_cuda, _stream
from .tissue import select_tiles

MAX_PATCH = 1024                 # qr::kMaxPatch: the int64 bound of the sharpness test
MAX_SHARPNESS = 1020 * 1020      # qr::kMaxSharpness: |L| <= 4 * 255
BLUR, INK = 2, 4                 # bits of the reason mask


def _int_in(name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an int in [{lo}, {hi}], not {v!r}")
    return int(v)


class QualityFilter:
    """Opt-in quality filter of `predict_full_patched`.  The defaults keep every tile: a user opts into each test.

    `min_sharpness`: an int in [0, 1 040 400], in grey levels squared: a tile whose Laplacian variance over its tissue pixels
    lies below it is rejected as out of focus (a tile without a tissue pixel: whenever `min_sharpness > 0`).
    `max_ink_fraction` in [0, 1]: a tile with more than floor(max_ink_fraction * P * P) ink pixels is rejected.
    `ink_chroma`, `ink_margin` (ints in [0, 255]) and `dark_max` (an int in [-1, 255]; -1 switches the dark clause off) are
    the ink rule's constants: in H&E green is the smallest channel of both pink and purple, so a saturated pixel whose green
    is not the smallest is blue or green marker, and a very dark pixel is black marker or a fold.  The defaults 40 / 16 / 40
    are conventional choices that have not been validated on real slides here, and red marker cannot be told from eosin by
    this rule.  `fill_class`: the class id written to map cells that no kept tile covers (-1: no class)."""

    def __init__(self, min_sharpness: int = 0, max_ink_fraction: float = 1.0, ink_chroma: int = 40, ink_margin: int = 16,
                 dark_max: int = 40, fill_class: int = -1):
        self.min_sharpness = _int_in("min_sharpness", min_sharpness, 0, MAX_SHARPNESS)
        if (isinstance(max_ink_fraction, bool) or not isinstance(max_ink_fraction, numbers.Real)
                or not 0.0 <= float(max_ink_fraction) <= 1.0):   # NaN fails the comparison too
            raise ValueError(f"max_ink_fraction must be a number in [0, 1], not {max_ink_fraction!r}")
        self.max_ink_fraction = float(max_ink_fraction)
        self.ink_chroma = _int_in("ink_chroma", ink_chroma, 0, 255)
        self.ink_margin = _int_in("ink_margin", ink_margin, 0, 255)
        self.dark_max = _int_in("dark_max", dark_max, -1, 255)
        if isinstance(fill_class, bool) or not isinstance(fill_class, numbers.Integral) or fill_class < -1:
            raise ValueError(f"fill_class must be a class id or -1, not {fill_class!r}")
        self.fill_class = int(fill_class)

    def max_ink_pixels(self, patch: int) -> int:
        return max_ink_pixels(self.max_ink_fraction, patch)

    def __repr__(self):
        return (f"QualityFilter(min_sharpness={self.min_sharpness}, max_ink_fraction={self.max_ink_fraction}, "
                f"ink_chroma={self.ink_chroma}, ink_margin={self.ink_margin}, dark_max={self.dark_max}, "
                f"fill_class={self.fill_class})")


def max_ink_pixels(max_ink_fraction: float, patch: int) -> int:
    """Ink pixels a P x P tile may hold: floor(max_ink_fraction * P * P)."""
    return math.floor(max_ink_fraction * patch * patch)


def check_fill_classes(tissue, quality) -> None:
    """Uncovered cells get one class: a tissue filter and a quality filter used together must name the same one."""
    if tissue is not None and quality is not None and tissue.fill_class != quality.fill_class:
        raise ValueError(f"tissue.fill_class ({tissue.fill_class}) and quality.fill_class ({quality.fill_class}) must be equal")


def _check_patch(patch: int) -> None:
    if not 0 < patch <= MAX_PATCH:
        raise ValueError(f"the quality filter takes a patch size in [1, {MAX_PATCH}], not {patch}")


def tile_quality_stats(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, threshold: int, filt: QualityFilter,
                       origins_host: np.ndarray | None = None) -> torch.Tensor:
    """int64[n, 4] on the device: (n_t, S1, S2, n_ink) of the patch x patch window at each (y, x) of `origins_dev`
    (int32[n, 2]); tissue is chroma > `threshold` (-1: every pixel).  `origins_host`: the same origins on the host, checked
    against the slide before any launch.  The slide needs no alignment."""
    _require_cuda(slide, "slide")
    if slide.dtype != torch.uint8 or slide.dim() != 3 or slide.shape[2] != 3 or not slide.is_contiguous():
        raise ValueError("slide must be a contiguous uint8[h, w, 3]")
    _require_cuda(origins_dev, "origins")
    if origins_dev.dtype != torch.int32 or origins_dev.dim() != 2 or origins_dev.shape[1] != 2 or not origins_dev.is_contiguous():
        raise ValueError("origins must be a contiguous int32[n, 2]")
    h, w, n = int(slide.shape[0]), int(slide.shape[1]), int(origins_dev.shape[0])
    host = None
    if origins_host is not None:
        host = np.ascontiguousarray(origins_host, dtype=np.int32).reshape(-1, 2)
        if host.shape[0] != n:
            raise ValueError(f"{n} device origins but {host.shape[0]} host origins")
    stats = torch.empty((n, 4), dtype=torch.int64, device=slide.device)
    check(lib().dh_quality_tile_stats(slide.data_ptr(), h, w, origins_dev.data_ptr() if n else None,
                                      host.ctypes.data_as(C.c_void_p) if host is not None else None, n, int(patch),
                                      int(threshold), filt.ink_chroma, filt.ink_margin, filt.dark_max,
                                      stats.data_ptr() if n else None, _stream(slide.device)), "dh_quality_tile_stats")
    return stats


def quality_flags(stats: torch.Tensor, filt: QualityFilter, patch: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(reason uint8[n], keep int32[n]) on the device from int64[n, 4] `stats` of tiles of side `patch`: reason is BLUR | INK
    as they apply, keep is 1 where it is 0."""
    _require_cuda(stats, "stats")
    if stats.dtype != torch.int64 or stats.dim() != 2 or stats.shape[1] != 4 or not stats.is_contiguous():
        raise ValueError("stats must be a contiguous int64[n, 4]")
    _check_patch(patch)
    n = int(stats.shape[0])
    reason = torch.empty(n, dtype=torch.uint8, device=stats.device)
    keep = torch.empty(n, dtype=torch.int32, device=stats.device)
    check(lib().dh_quality_flags(stats.data_ptr() if n else None, n, filt.min_sharpness, filt.max_ink_pixels(patch),
                                 reason.data_ptr() if n else None, keep.data_ptr() if n else None, _stream(stats.device)),
          "dh_quality_flags")
    return reason, keep


def sharpness(stats) -> np.ndarray:
    """float64[n]: the Laplacian variance (n_t*S2 - S1*S1) / n_t^2 of each row of int64[n, 4] `stats`, NaN where n_t == 0.
    For reporting only: the decision never divides."""
    s = (stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)).reshape(-1, 4)
    out = np.full(len(s), np.nan)
    for i, (n_t, s1, s2, _) in enumerate(s.tolist()):   # Python ints: the numerator is exact before the one division
        if n_t > 0:
            out[i] = (n_t * s2 - s1 * s1) / (n_t * n_t)
    return out


def score_quality(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, threshold: int, filt: QualityFilter,
                  origins_host: np.ndarray | None = None) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """The whole quality step: per-tile sums, flags, compaction (one read-back of the kept count).  Returns (kept indices
    int32[k], kept origins int32[k, 2], info) with info = threshold, min_sharpness, max_ink_pixels, n_tiles, n_kept,
    rejected_blur, rejected_ink and, on the host, stats (int64[n, 4]) and reason (uint8[n])."""
    _check_patch(patch)
    stats = tile_quality_stats(slide, origins_dev, patch, threshold, filt, origins_host)
    reason, keep = quality_flags(stats, filt, patch)
    idx, yx = select_tiles(keep, origins_dev, 1)
    reason_host = reason.cpu().numpy()
    info = dict(threshold=int(threshold), min_sharpness=filt.min_sharpness, max_ink_pixels=filt.max_ink_pixels(patch),
                n_tiles=int(origins_dev.shape[0]), n_kept=int(idx.shape[0]),
                rejected_blur=int(np.count_nonzero(reason_host & BLUR)), rejected_ink=int(np.count_nonzero(reason_host & INK)),
                stats=stats.cpu().numpy(), reason=reason_host)
    return idx, yx, info


def sharpness_summary(stats) -> dict:
    """Minimum, quartiles and maximum of the sharpness of the tiles that have one (what a user needs to pick `min_sharpness`)."""
    v = sharpness(stats)
    v = v[~np.isnan(v)]
    if not len(v):
        return dict(n=0, min=None, q1=None, median=None, q3=None, max=None)
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return dict(n=int(len(v)), min=float(q[0]), q1=float(q[1]), median=float(q[2]), q3=float(q[3]), max=float(q[4]))
