"""Pyramid layers of an HBM-resident slide: integer-exact area downsampling on the device.

In the reference `layer=L` is the slide at 1/L of the scan's resolution: annotations are divided by L, `psim.layer_size(L)` is
that layer's size and `get_region_from_layer(L, ...)` takes that layer's coordinates.  `PyramidSlide` serves exactly that from an
array, a `.npy` file or a tensor; `area_resample` is the pass underneath (`dh_resample_area`, csrc/resample.hip), for any
rational factor num/den >= 1:

    oh = (h * den) // num, ow = (w * den) // num        (only output pixels whose footprint lies wholly inside the source)
    wy(y, j) = max(0, min((j+1) den, (y+1) num) - max(j den, y num)), wx the same in x     (sum to num per axis)
    S = sum_j sum_i wy wx src[j][i][c],  D = num^2,  out = (2 S + D) // (2 D)              (the exact mean, rounded half up, once)

The host math below (factor parsing, sizes, bounds, the division's host twin) needs no GPU.
"""
from __future__ import annotations

import numbers
from fractions import Fraction
from pathlib import Path

import numpy as np

MAX_NUM = 2048                  # 1 <= den <= num <= MAX_NUM
MAX_RATIO = 64                  # num <= MAX_RATIO * den
MAX_SIDE = 1 << 20              # h, w: a side times MAX_NUM stays inside int32

# the kernel's tiling constants (csrc/resample.hip: kThreads, kChunk, kSrcPx, kBandH)
THREADS = 256
STORE_GROUP = 16                # source bytes per lane and row; output rows leave in aligned groups of as many bytes
SRC_PX = THREADS * STORE_GROUP // 3   # 1365: the source pixels under one strip of output columns
BAND_H = 16                     # output rows per workgroup


def strip_width(num: int, den: int) -> int:
    """Output columns per workgroup at the (reduced) factor num/den: the most whose source footprint fits SRC_PX pixels."""
    return (SRC_PX - 2) * den // num


def parse_factor(factor) -> tuple[int, int]:
    """(num, den) in lowest terms of an int, a fractions.Fraction or a "NUM/DEN" string; anything else (a float above all: it
    would hide the rational) and a factor below 1 or outside the limits is refused by name."""
    if isinstance(factor, bool) or isinstance(factor, numbers.Real) and not isinstance(factor, numbers.Rational):
        raise TypeError(f"factor must be an int, a fractions.Fraction or a 'NUM/DEN' string, not the {type(factor).__name__} {factor!r} "
                        "(a float would hide the rational)")
    if isinstance(factor, str):
        parts = factor.split("/")
        if len(parts) not in (1, 2) or not all(p.strip().isdigit() for p in parts):
            raise ValueError(f"factor must be written 'NUM' or 'NUM/DEN' with positive integers, not {factor!r}")
        n, d = int(parts[0]), int(parts[1]) if len(parts) == 2 else 1
        if d == 0:
            raise ValueError(f"factor {factor!r} has a zero denominator")
        f = Fraction(n, d)
    elif isinstance(factor, numbers.Rational):
        f = Fraction(factor)
    else:
        raise TypeError(f"factor must be an int, a fractions.Fraction or a 'NUM/DEN' string, not {type(factor).__name__}")
    num, den = f.numerator, f.denominator
    if f < 1:
        raise ValueError(f"factor {num}/{den} is below 1: upsampling is not built")
    if num > MAX_NUM:
        raise ValueError(f"factor {num}/{den} is outside the limits: 1 <= den <= num <= {MAX_NUM} in lowest terms")
    if num > MAX_RATIO * den:
        raise ValueError(f"factor {num}/{den} is outside the limits: at most {MAX_RATIO}")
    return num, den


def resampled_size(h: int, w: int, factor) -> tuple[int, int]:
    """(oh, ow) = ((h den) // num, (w den) // num): the ragged remainder is dropped."""
    num, den = parse_factor(factor)
    if h < 0 or w < 0:
        raise ValueError(f"size {h} x {w} is negative")
    return (int(h) * den) // num, (int(w) * den) // num


def div_magic(d: int) -> int:
    """The 64-bit constant M = (2^64 - 1) // d + 1 by which the kernel divides by d (d = 2 num^2, or den >= 2)."""
    return ((1 << 64) - 1) // d + 1


def div_by_magic(n: int, magic: int) -> int:
    """The kernel's n // d for a 32-bit n, with its widths: two 32 x 32 -> 64 products of n with the halves of the constant."""
    assert 0 <= n < 1 << 32 and 0 < magic < 1 << 64
    mlo, mhi = magic & 0xFFFFFFFF, magic >> 32
    t = ((n * mlo) & ((1 << 64) - 1)) >> 32
    u = n * mhi + t
    assert u < 1 << 64
    return (u >> 32) & 0xFFFFFFFF


def overflow_bounds() -> dict:
    """Worst-case magnitude of every accumulator and product of the kernel over all 8-bit inputs and all factors inside the
    limits, as Python ints, each with the limit it has to stay below."""
    d = MAX_NUM * MAX_NUM
    return {
        "vertical_sum": (255 * MAX_NUM, 2 ** 32),                    # sum_j wy * byte: the weights of an axis sum to num
        "weighted_sum": (255 * d, 2 ** 32),                          # S
        "rounded_numerator": (2 * 255 * d + d, 2 ** 32),             # 2 S + D = 511 * 2048^2
        "magic_product": ((2 ** 32 - 1) * (2 ** 32 - 1) + (2 ** 32 - 1), 2 ** 64),   # n * mhi + ((n * mlo) >> 32)
        "magic_error": ((2 ** 32 - 1) * 2 * d, 2 ** 64),             # n * e, e = M * 2 D - 2^64 <= 2 D: the quotient is exact below 2^64
        "coordinate": (MAX_SIDE * (MAX_NUM - 1) + MAX_NUM, 2 ** 31),  # (i + 1) den, (x + 1) num + den - 1 with a reduced den < MAX_NUM
        "source_bytes": (3 * MAX_SIDE * MAX_SIDE, 2 ** 63),          # byte offsets are 64-bit
    }


# ---- device entry -----------------------------------------------------------------------------------------------------------
def _check_source(slide):
    import torch
    if not isinstance(slide, torch.Tensor):
        raise TypeError(f"slide must be a torch tensor, not {type(slide).__name__}")
    if not slide.is_cuda:
        raise ValueError(f"slide must live in GPU memory (got a {slide.device} tensor)")
    if slide.dtype != torch.uint8:
        raise ValueError(f"slide must be uint8, not {slide.dtype}")
    if slide.dim() != 3 or slide.shape[2] != 3:
        raise ValueError(f"slide must be uint8[h, w, 3], not {list(slide.shape)}")
    if not slide.is_contiguous():
        raise ValueError("slide must be contiguous")
    h, w = int(slide.shape[0]), int(slide.shape[1])
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"slide of {h} x {w} exceeds {MAX_SIDE} pixels a side")
    return h, w


def _overlap(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() and b0 < a0 + a.numel()


def area_resample(slide, factor, out=None):
    """uint8[oh, ow, 3] on the slide's device: `slide` (uint8[h, w, 3], contiguous, in GPU memory) area-averaged by `factor`
    (an int, a Fraction or "NUM/DEN", at least 1), every byte the exact mean rounded half up.  `out`: where to write, a
    contiguous uint8[oh, ow, 3] tensor on the same device that does not overlap the slide.  Factor 1 returns a copy."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    num, den = parse_factor(factor)
    h, w = _check_source(slide)
    oh, ow = (h * den) // num, (w * den) // num
    if oh == 0 or ow == 0:
        raise ValueError(f"a slide of {h} x {w} is smaller than the factor {num}/{den}: no whole output pixel")
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != slide.device
                or tuple(out.shape) != (oh, ow, 3) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8[{oh}, {ow}, 3] tensor on {slide.device}")
        if _overlap(slide, out):
            raise ValueError("out must not overlap the slide")
    if num == den:
        return slide.clone() if out is None else out.copy_(slide)
    src = slide if slide.data_ptr() % 16 == 0 else slide.clone()
    dst = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty((oh, ow, 3), dtype=torch.uint8, device=slide.device)
    check(lib().dh_resample_area(src.data_ptr(), h, w, num, den, dst.data_ptr(), oh, ow, _stream(slide.device)), "dh_resample_area")
    if out is None:
        return dst
    if dst is not out:
        out.copy_(dst)
    return out


class PyramidSlide:
    """`PSImage`-shaped reader whose layer L is the base at 1/L of its resolution, resident in HBM (the duck type of
    `psimage_compat.ArraySlide`, plus `layer_device`).

    `base`: a uint8[h, w, 3] host array, the path of a `.npy` file (memory-mapped) or a uint8[h, w, 3] tensor.  A layer is built
    on first use, straight from layer 1 (never from another layer: each is the single rounding of the true mean), and cached.
    Layer 1 of a device base is the base itself.  A host or memory-mapped base never goes to the device whole: it is uploaded
    in bands of at most `band_bytes` (a multiple of L rows, at least L), each band is resampled into its rows of the layer and
    the band buffer is reused, so HBM holds the layer plus one band.  `close()` drops the cached layers; the reader stays
    usable and builds them again on demand."""

    def __init__(self, base, device="cuda", band_bytes: int = 1 << 30):
        import torch
        if isinstance(band_bytes, bool) or not isinstance(band_bytes, numbers.Integral) or band_bytes < 1:
            raise ValueError(f"band_bytes must be a positive integer, not {band_bytes!r}")
        self.band_bytes = int(band_bytes)
        self._host = self._base_dev = None
        if isinstance(base, torch.Tensor):
            if base.dtype != torch.uint8 or base.dim() != 3 or base.shape[2] != 3:
                raise ValueError("slide tensor must be uint8[h, w, 3]")
            if base.is_cuda:
                self._base_dev, device = base.contiguous(), base.device
            else:
                self._host = base.contiguous().numpy()
        else:
            if isinstance(base, (str, Path)):
                if Path(base).suffix != ".npy":
                    raise ValueError(f"PyramidSlide reads arrays, tensors and .npy files, not '{base}' (a psimage file has layers of its own)")
                base = np.load(base, mmap_mode="r")
            a = base if isinstance(base, np.ndarray) else np.asarray(base)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("slide array must be uint8[h, w, 3]")
            self._host = a
        self.device = torch.device(device)
        shape = self._base_dev.shape if self._base_dev is not None else self._host.shape
        self.height, self.width = int(shape[0]), int(shape[1])
        self._layers: dict = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False          # the samplers open their sources in a `with`: the cached layers outlive it (close() drops them)

    def close(self):
        self._layers.clear()

    def _assert_layer(self, layer):
        if isinstance(layer, bool) or not isinstance(layer, numbers.Integral) or not 1 <= layer <= MAX_RATIO:
            raise ValueError(f"invalid layer {layer!r}: an integer in [1, {MAX_RATIO}]")

    def layer_size(self, layer):
        self._assert_layer(layer)
        return resampled_size(self.height, self.width, int(layer))

    def layer_device(self, layer):
        """uint8[oh, ow, 3] in HBM: layer `layer`, built on first use."""
        self._assert_layer(layer)
        layer = int(layer)
        if layer not in self._layers:
            oh, ow = self.layer_size(layer)
            if oh == 0 or ow == 0:
                raise ValueError(f"a slide of {self.height} x {self.width} has no layer {layer}: smaller than the factor")
            if self._base_dev is not None:
                self._layers[layer] = self._base_dev if layer == 1 else area_resample(self._base_dev, layer)
            else:
                self._layers[layer] = self._build_from_host(layer, oh, ow)
        return self._layers[layer]

    def band_rows(self, layer: int) -> int:
        """Source rows per uploaded band: the most that fit `band_bytes`, in whole groups of 16 `layer` rows where that many
        fit (the band's rows of the layer then start 16-byte aligned), else in whole multiples of `layer`, at least one."""
        fit = self.band_bytes // (3 * self.width)
        unit = STORE_GROUP * layer if fit >= STORE_GROUP * layer else layer
        return max(layer, fit // unit * unit)

    def _build_from_host(self, layer: int, oh: int, ow: int):
        import torch
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=self.device)
        rows = min(self.band_rows(layer), oh * layer)
        band = torch.empty((rows, self.width, 3), dtype=torch.uint8, device=self.device)
        for r0 in range(0, oh * layer, rows):       # the rows below oh * layer are the dropped remainder
            n = min(rows, oh * layer - r0)
            rows_host = self._host[r0:r0 + n]
            if not (rows_host.flags.writeable and rows_host.flags.c_contiguous):   # a read-only memory map: torch wants its own copy
                rows_host = np.array(rows_host)
            band[:n].copy_(torch.from_numpy(rows_host))
            if layer == 1:
                out[r0:r0 + n].copy_(band[:n])
            else:
                area_resample(band[:n], layer, out=out[r0 // layer:(r0 + n) // layer])
        return out

    def get_region_from_layer(self, layer, p0, p1):
        self._assert_layer(layer)
        if int(layer) == 1 and self._host is not None:
            return self._host[p0[0]:p1[0], p0[1]:p1[1], :]
        return self.layer_device(layer)[p0[0]:p1[0], p0[1]:p1[1], :].cpu().numpy()

    def get_region(self, p0, p1, target_hw=None):
        """`ArraySlide.get_region` applied to layer 1."""
        from .psimage_compat import ArraySlide
        reg = np.ascontiguousarray(self.get_region_from_layer(1, p0, p1))
        return ArraySlide(reg).get_region((0, 0), reg.shape[:2], target_hw)


def wrap_pyramid(source, device="cuda"):
    """`source` behind a PyramidSlide when it is an array, a tensor or a `.npy` path; anything else (a reader, a path that goes
    to psimage, which has layers of its own) as it is."""
    import torch
    if isinstance(source, (np.ndarray, torch.Tensor)) or isinstance(source, (str, Path)) and Path(source).suffix == ".npy":
        return PyramidSlide(source, device=device)
    return source
