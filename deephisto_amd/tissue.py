"""Tissue mask for whole-slide prediction: skip the glass.

A pixel is tissue when its chroma `max(R,G,B) - min(R,G,B)` exceeds a threshold `t`; a tile is kept when its P x P window
holds at least `min_pixels = ceil(min_fraction * P * P)` tissue pixels.  The histogram, the per-tile counts, the compaction and
the fill of uncovered map cells run in libdeephisto_hip.so (csrc/tissue.hip); the Otsu choice of `t` is exact integer
arithmetic on the host.  Everything is integer-exact, so every rank of a sharded run computes the same kept list.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np
import torch

from ._lib import check, lib
from .tiles import _require_cuda, _stream


class TissueFilter:
    """Opt-in tissue filter of `predict_full_patched`.

    `threshold`: "otsu" (chosen per slide from the chroma histogram) or an int in [0, 255]; a pixel with chroma > threshold is
    tissue.  `min_fraction` in [0, 1]: the share of a tile's pixels that must be tissue for the tile to be classified.  The
    default 0.25 is a conventional choice that has not been validated on real slides here.  `fill_class`: the class id written
    to map cells that no kept tile covers (-1: no class; the colour lookup leaves it black)."""

    def __init__(self, threshold="otsu", min_fraction: float = 0.25, fill_class: int = -1):
        if isinstance(threshold, str):
            if threshold != "otsu":
                raise ValueError(f"threshold must be 'otsu' or an int in [0, 255], not {threshold!r}")
        elif isinstance(threshold, bool) or not isinstance(threshold, numbers.Integral) or not 0 <= threshold <= 255:
            raise ValueError(f"threshold must be 'otsu' or an int in [0, 255], not {threshold!r}")
        if (isinstance(min_fraction, bool) or not isinstance(min_fraction, numbers.Real)
                or not 0.0 <= float(min_fraction) <= 1.0):   # NaN fails the comparison too
            raise ValueError(f"min_fraction must be a number in [0, 1], not {min_fraction!r}")
        if isinstance(fill_class, bool) or not isinstance(fill_class, numbers.Integral) or fill_class < -1:
            raise ValueError(f"fill_class must be a class id or -1, not {fill_class!r}")
        self.threshold = threshold if isinstance(threshold, str) else int(threshold)
        self.min_fraction = float(min_fraction)
        self.fill_class = int(fill_class)

    def min_pixels(self, patch: int) -> int:
        return min_pixels(self.min_fraction, patch)

    def __repr__(self):
        return f"TissueFilter(threshold={self.threshold!r}, min_fraction={self.min_fraction}, fill_class={self.fill_class})"


def min_pixels(min_fraction: float, patch: int) -> int:
    """Tissue pixels a P x P tile needs: ceil(min_fraction * P * P)."""
    return math.ceil(min_fraction * patch * patch)


def otsu_threshold(hist) -> int:
    """Otsu's threshold of a 256-bin chroma histogram, exactly: the t in 0..254 with both classes non-empty that maximises
    (N*S0 - S*n0)^2 / (n0*n1) (proportional to the between-class variance; n0, S0: count and chroma sum of bins <= t; N, S:
    totals), compared by cross-multiplication in Python ints, the smallest t on a tie; 0 when fewer than two bins are
    non-empty."""
    h = [int(v) for v in np.asarray(hist).reshape(-1)]
    if len(h) != 256 or min(h) < 0:
        raise ValueError("hist must hold 256 non-negative counts")
    N = sum(h)
    S = sum(i * v for i, v in enumerate(h))
    best_t, best_num, best_den = 0, -1, 1
    n0 = s0 = 0
    for t in range(255):
        n0 += h[t]
        s0 += t * h[t]
        n1 = N - n0
        if n0 == 0 or n1 == 0:
            continue
        num, den = (N * s0 - S * n0) ** 2, n0 * n1
        if num * best_den > best_num * den:
            best_t, best_num, best_den = t, num, den
    return best_t


def _check_slide(slide: torch.Tensor) -> torch.Tensor:
    _require_cuda(slide, "slide")
    if slide.dtype != torch.uint8 or slide.dim() != 3 or slide.shape[2] != 3:
        raise ValueError("slide must be uint8[h, w, 3]")
    if slide.data_ptr() % 16:   # the kernels read 16-byte words
        slide = slide.clone()
    return slide


def chroma_histogram(slide: torch.Tensor) -> np.ndarray:
    """np.uint64[256]: how many pixels of the device-resident slide have each chroma value (synchronises)."""
    slide = _check_slide(slide)
    hist = torch.empty(256, dtype=torch.int64, device=slide.device)
    check(lib().dh_tissue_histogram(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), hist.data_ptr(),
                                    _stream(slide.device)), "dh_tissue_histogram")
    return hist.cpu().numpy().view(np.uint64)


def tile_tissue_counts(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, threshold: int,
                       origins_host: np.ndarray | None = None) -> torch.Tensor:
    """int32[n] on the device: tissue pixels (chroma > threshold) in the patch x patch window at each (y, x) of
    `origins_dev` (int32[n, 2]).  `origins_host`: the same origins on the host, checked against the slide before any launch."""
    slide = _check_slide(slide)
    _require_cuda(origins_dev, "origins")
    if origins_dev.dtype != torch.int32 or origins_dev.dim() != 2 or origins_dev.shape[1] != 2:
        raise ValueError("origins must be int32[n, 2]")
    h, w, n = int(slide.shape[0]), int(slide.shape[1]), int(origins_dev.shape[0])
    host = None
    if origins_host is not None:
        host = np.ascontiguousarray(origins_host, dtype=np.int32).reshape(-1, 2)
        if host.shape[0] != n:
            raise ValueError(f"{n} device origins but {host.shape[0]} host origins")
    words = (h * w + 63) // 64
    bitmap = torch.empty(words, dtype=torch.int64, device=slide.device)
    counts = torch.empty(n, dtype=torch.int32, device=slide.device)
    check(lib().dh_tissue_tile_counts(slide.data_ptr(), h, w, origins_dev.data_ptr(),
                                      host.ctypes.data_as(C.c_void_p) if host is not None else None, n, patch, int(threshold),
                                      bitmap.data_ptr(), words, counts.data_ptr(), _stream(slide.device)),
          "dh_tissue_tile_counts")
    return counts


def select_tiles(counts: torch.Tensor, origins_dev: torch.Tensor, min_pixels: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(kept indices int32[k], kept origins int32[k, 2]) on the device, in grid order: the tiles with counts >= min_pixels.
    k is read back (one synchronisation)."""
    _require_cuda(counts, "counts")
    _require_cuda(origins_dev, "origins")
    n = int(counts.shape[0])
    if counts.dtype != torch.int32 or origins_dev.dtype != torch.int32 or tuple(origins_dev.shape) != (n, 2):
        raise ValueError("counts must be int32[n] and origins int32[n, 2]")
    dev = counts.device
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    yx = torch.empty((n, 2), dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    k = C.c_int64()
    check(lib().dh_tissue_select(counts.data_ptr(), origins_dev.data_ptr(), n, int(min_pixels), idx.data_ptr(), yx.data_ptr(),
                                 status.data_ptr(), C.byref(k), _stream(dev)), "dh_tissue_select")
    return idx[:k.value], yx[:k.value]


def fill_uncovered(class_map: torch.Tensor, origins_dev: torch.Tensor, patch: int, downscale: int, h: int, w: int,
                   fill_class: int) -> torch.Tensor:
    """In place: the cells of int64[h//d, w//d] `class_map` that no footprint [y//d, (y+P)//d) x [x//d, (x+P)//d) of
    `origins_dev` covers become `fill_class` (coverage is computed, not inferred from the canvas)."""
    _require_cuda(class_map, "class_map")
    if class_map.dtype != torch.int64 or tuple(class_map.shape) != (h // downscale, w // downscale):
        raise ValueError("class_map must be int64[h//d, w//d]")
    n = int(origins_dev.shape[0])
    if n:
        _require_cuda(origins_dev, "origins")
    cover = torch.empty(class_map.numel(), dtype=torch.uint8, device=class_map.device)
    check(lib().dh_fill_uncovered(origins_dev.data_ptr() if n else None, n, patch, downscale, h, w, int(fill_class),
                                  cover.data_ptr(), class_map.data_ptr(), _stream(class_map.device)), "dh_fill_uncovered")
    return class_map


def score_tiles(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, filt: TissueFilter,
                origins_host: np.ndarray | None = None) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """The whole scoring step: threshold (Otsu when asked), per-tile counts, compaction.  Returns (kept indices int32[k],
    kept origins int32[k, 2], info) with info = threshold, min_pixels, n_tiles, n_kept and, after Otsu, histogram."""
    info: dict = {}
    if filt.threshold == "otsu":
        hist = chroma_histogram(slide)
        info["histogram"] = hist
        t = otsu_threshold(hist)
    else:
        t = filt.threshold
    mp = filt.min_pixels(patch)
    counts = tile_tissue_counts(slide, origins_dev, patch, t, origins_host)
    idx, yx = select_tiles(counts, origins_dev, mp)
    info.update(threshold=t, min_pixels=mp, n_tiles=int(origins_dev.shape[0]), n_kept=int(idx.shape[0]))
    return idx, yx, info
