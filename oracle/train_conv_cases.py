"""The single-convolution cases of the bf16 training engine (tests/test_gpu_conv_bf16_train.py) with their operands, float64 reference and
an independent float32 evaluation -- shared with tests/test_layer_reference_host.py, which shows on the CPU that the identical-fraction
floor demanded of the kernels is one a plain float32 evaluation of the same operands already meets.

A case is (ks, stride, conv cin -> cout, B, Hi) of a convolution the engine can produce, run forward (`dgrad` 0: x -> Z) or as data
gradient (`dgrad` 1: dZ -> dX, optionally + res, the gradient joining from another branch).  Operands: the input and res are standard
normal values rounded to bf16, w is normal at He scale sqrt(2 / (cin ks ks)), kept in float32 (the engine's master weights); the
reference uses w.bfloat16(), what the engine's packer makes of it.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr


class Case(NamedTuple):
    name: str
    ks: int
    stride: int
    cin: int
    cout: int
    B: int
    H: int          # the convolution's input size (square maps)
    dgrad: int
    res: bool
    imgs: int = 1   # images per tile of the variant the engine picks (only used to choose the reference images of a large batch)

    @property
    def Ho(self) -> int:
        return (self.H + 2 * (self.ks // 2) - self.ks) // self.stride + 1

    @property
    def accumulate(self) -> bool:
        """The strided 1x1 data gradient: the product is stored, then added into dX (two stored roundings)."""
        return bool(self.dgrad) and self.ks == 1 and self.stride == 2


CASES = [
    # stride-2 3x3 data gradient, one case per branch of the CLS == 4 candidate table of plan_dgrad_s2 (csrc/conv3_plan_host.h) (re = ce = H / 2 rows and columns
    # per parity class; tiles = ceil(B / imgs) * ceil(re / th) * ceil(ce / tw) * cin / 64; the first candidate with >= 256 tiles wins)
    Case("dgrad3_s2_16x16x1_mt2", 3, 2, 128, 128, 32, 40, 1, False, 1),   # ce = 20 > 8: 32 * 2 * 2 * 2 = 256 tiles; ragged 16 + 4
    Case("dgrad3_s2_8x8x2_mt1", 3, 2, 64, 128, 3, 24, 1, True, 2),        # ce = 12 > 8: 16x16x1 gives 3 tiles -> 8x8x2: 2 * 2 * 2 * 1 = 8; odd batch
    Case("dgrad3_s2_8x8x4_mt2", 3, 2, 512, 512, 125, 12, 1, False, 4),    # ce = 6 <= 8: 32 * 1 * 1 * 8 = 256 tiles; last group = one image
    Case("dgrad3_s2_small_8x8x2", 3, 2, 256, 512, 5, 4, 1, False, 2),     # ce = 2 <= 8: 8x8x4 gives 8 tiles -> 8x8x2: 3 * 1 * 1 * 4 = 12
    # stride-1 3x3 data gradient through the flipped + transposed operand (pick_stride1 over B x H x H x cin)
    Case("dgrad3_s1_64", 3, 1, 64, 64, 3, 16, 1, False, 2),               # 8x8x2, 128-pixel tiles: 8 tiles
    Case("dgrad3_s1_128", 3, 1, 128, 128, 4, 28, 1, False, 1),            # 16x16, 256-pixel tiles: 32 tiles
    Case("dgrad3_s1_512_res", 3, 1, 512, 512, 5, 7, 1, True, 2),          # 8x8x2: 24 tiles, odd map
    Case("dgrad3_s1_64_persistent", 3, 1, 64, 64, 32, 64, 1, False, 1),   # 16x32, 512-pixel tiles: 32 * 4 * 2 * 1 = 256 tiles
    # forward: raw Z
    Case("fwd3_s1_64", 3, 1, 64, 64, 3, 16, 0, False),
    Case("fwd3_s2_128", 3, 2, 128, 128, 3, 24, 0, False),                 # the non-downsample stride-2 variant, 8 x 16 tiles
    Case("fwd3_s2_256_512", 3, 2, 256, 512, 5, 14, 0, False),             # ... 8 x 8 x 2 images, odd output map, odd batch
    Case("fwd1_s1", 1, 1, 64, 256, 3, 24, 0, False),
    Case("fwd1_s2", 1, 2, 256, 512, 3, 14, 0, False),
    # 1x1 data gradient
    Case("dgrad1_s1_res", 1, 1, 64, 256, 3, 24, 1, True),
    Case("dgrad1_s1_2048", 1, 1, 512, 2048, 5, 7, 1, False),
    Case("dgrad1_s2_accumulate", 1, 2, 256, 512, 3, 14, 1, True),         # the accumulate path, under its own derived gate
]
BY_NAME = {c.name: c for c in CASES}


class Operands(NamedTuple):
    inp: torch.Tensor            # float32 NCHW, bf16-exact: x (forward) or dZ (data gradient)
    w: torch.Tensor              # float32 [cout][cin][ks][ks], NOT rounded
    res: torch.Tensor | None     # float32 NCHW [B][cin][H][H], bf16-exact


@functools.lru_cache(maxsize=2)
def operands(name: str) -> Operands:
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    bf = lambda t: t.bfloat16().float()  # noqa: E731
    shape = (c.B, c.cout, c.Ho, c.Ho) if c.dgrad else (c.B, c.cin, c.H, c.H)
    inp = bf(torch.randn(shape, generator=g))
    w = torch.randn(c.cout, c.cin, c.ks, c.ks, generator=g) * (2.0 / (c.cin * c.ks * c.ks)) ** 0.5
    res = bf(torch.randn(c.B, c.cin, c.H, c.H, generator=g)) if c.res else None
    return Operands(inp, w, res)


def select(c: Case) -> np.ndarray:
    """Images held against the float64 reference.  Up to 16 images: all.  A larger batch: the first 8, the images on both sides of every
    image-group boundary next to the middle, and the last whole group with the partial one behind it (the rest is checked for
    bit-equality between two runs only: the float64 transposed convolution of 125 images takes too long on a CPU)."""
    if c.B <= 16:
        return np.arange(c.B)
    g = (c.B // 2 // c.imgs) * c.imgs
    idx = np.r_[0:8, g - c.imgs - 1:g + c.imgs + 1, ((c.B - 1) // c.imgs - 1) * c.imgs:c.B]
    return np.unique(idx[(idx >= 0) & (idx < c.B)])


class Reference(NamedTuple):
    sel: np.ndarray
    want: np.ndarray             # float64 NCHW of the selected images, rounded once to bf16
    A: np.ndarray
    K: int
    prod: np.ndarray | None      # accumulate path: the exact product and its magnitude sum (lr.stored_product_gate_mask) ...
    A_prod: np.ndarray | None
    stored: np.ndarray           # ... and the value its two stored roundings define; every other case: `want`


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    c = BY_NAME[name]
    o = operands(name)
    sel = select(c)
    inp, wb = o.inp[sel].double(), o.w.bfloat16().double()
    res = o.res[sel].double() if o.res is not None else None
    if not c.dgrad:
        want, A = lr.conv_epilogue(inp, wb, np.ones(c.cout), np.zeros(c.cout), c.stride, None, relu=False)
        return Reference(sel, want, A, lr.rounding_count(c.cin, c.ks, "bf16", False), None, None, want)
    want, A = lr.conv_dgrad(inp, wb, c.stride, c.H, c.H, res)
    K = lr.rounding_count(c.cout, c.ks, "bf16", res is not None)
    if not c.accumulate:
        return Reference(sel, want, A, K, None, None, want)
    prod, A_prod = lr.conv_dgrad(inp, wb, c.stride, c.H, c.H, None, exact=True)
    return Reference(sel, want, A, K, prod, A_prod, lr.stored_product_sum(prod, res))


def gate(c: Case, ref: Reference, got: np.ndarray) -> np.ndarray:
    if c.accumulate:
        return lr.stored_product_gate_mask(got, ref.want, ref.A, ref.K, ref.prod, ref.A_prod)
    return lr.gate_mask(got, ref.want, ref.A, ref.K, "bf16")


def float32_evaluation(name: str) -> np.ndarray:
    """The selected images by torch's float32 CPU convolution on the same operands, stored as the engine stores them: one rounding to
    bf16 (accumulate path: the product rounded to bf16, then the float32 sum with res rounded again).  float64 NCHW."""
    c = BY_NAME[name]
    o = operands(name)
    sel = select(c)
    inp, wb = o.inp[sel], o.w.bfloat16().float()
    res = o.res[sel] if o.res is not None else None
    pad = c.ks // 2
    if not c.dgrad:
        y = F.conv2d(inp, wb, None, c.stride, pad)
    else:
        op = c.H - ((c.Ho - 1) * c.stride - 2 * pad + c.ks)
        y = F.conv_transpose2d(inp, wb, None, c.stride, pad, output_padding=op)
        if c.accumulate:
            y = y.bfloat16().float()
        if res is not None:
            y = y + res
    return y.bfloat16().double().numpy()
