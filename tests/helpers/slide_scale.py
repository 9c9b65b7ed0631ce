"""Two slides of more than 2^32 bytes that need no host copy, and the tile origins that probe them (tests/test_slide_scale_host.py,
tests/test_gpu_slide_scale.py).

H x W = 30 301 x 47 791: 4 344 345 273 bytes = 2^32 + 49 377 977; a row is 143 373 bytes (neither 4- nor 16-byte aligned);
H * W % 16 == 3 (the stain passes take their tail path); 344 rows lie wholly past byte 2^32.

`ClosedForm` is the synthetic slide of oracle/synth.py as a virtual image: any pixel from its coordinates, so a reference of a tile
anywhere costs the tile.  `Periodic` is a 1021 x 1031 block (prime sides) repeated over the slide: an additive statistic of the whole
slide is an integer combination of the statistic of four sub-blocks.  In both an address that wrapped by 2^31 or 2^32 bytes lands on
other content (checked on the host for every origin of `spots`)."""
import numpy as np

from oracle import synth

H, W = 30301, 47791
ROW_BYTES = 3 * W
EDGES = (2 ** 31, 2 ** 32)
BLOCK = (1021, 1031)

assert H * ROW_BYTES == 2 ** 32 + 49_377_977 and ROW_BYTES % 4 and (H * W) % 16 == 3
assert H - (2 ** 32 // ROW_BYTES + 1) == 344
assert H == 29 * 1021 + 692 and W == 46 * 1031 + 365


def _hash(y, x, c, seed):
    """oracle.synth's pixel formula on broadcast uint32 arrays."""
    with np.errstate(over="ignore"):
        v = (y.astype(np.uint32) * synth.K_Y) ^ (x.astype(np.uint32) * synth.K_X) ^ (c.astype(np.uint32) * synth.K_C) \
            ^ (np.uint32(seed & 0xFFFFFFFF) * synth.K_S)
    return ((v >> np.uint32(7)) & np.uint32(0xFF)).astype(np.uint8)


class ClosedForm:
    """A virtual uint8[h, w, 3] image over oracle.synth: `.shape` and `img[yy, xx]` for broadcast integer index arrays (what
    stain_aug_ref.py and geom_aug_ref.py ask of an image).  The device twin is tiles.synth_slide(h, w, seed, dev)."""

    def __init__(self, h, w, seed):
        self.shape, self.seed, self.dtype = (int(h), int(w), 3), int(seed), np.dtype(np.uint8)

    def __getitem__(self, key):
        yy, xx = (np.asarray(k) for k in key)
        h, w, _ = self.shape
        assert yy.dtype.kind in "iu" and xx.dtype.kind in "iu"
        assert yy.min() >= 0 and yy.max() < h and xx.min() >= 0 and xx.max() < w, "index outside the slide"
        yy, xx = np.broadcast_arrays(yy, xx)
        return _hash(yy[..., None], xx[..., None], np.arange(3), self.seed)

    def window(self, y0, x0, hh, ww):
        return synth.synth_region(int(y0), int(x0), int(hh), int(ww), self.seed)

    def flat(self, addr):
        """The bytes at flat byte offsets `addr` (int64, inside the allocation)."""
        a = np.asarray(addr, np.int64)
        h, w, _ = self.shape
        assert a.min() >= 0 and a.max() < h * w * 3
        y, rem = np.divmod(a, 3 * w)
        return _hash(y, rem // 3, rem % 3, self.seed)

    def device(self, dev):
        from deephisto_amd import tiles
        return tiles.synth_slide(self.shape[0], self.shape[1], self.seed, dev)


class Periodic:
    """The slide block[y % bh, x % bw] of h x w pixels, never materialised on the host."""

    def __init__(self, block, h, w):
        self.block = np.ascontiguousarray(block, dtype=np.uint8)
        self.bh, self.bw = self.block.shape[:2]
        self.shape, self.dtype = (int(h), int(w), 3), np.dtype(np.uint8)
        self.ny, self.ry = divmod(int(h), self.bh)
        self.nx, self.rx = divmod(int(w), self.bw)

    def parts(self):
        """[(multiplicity, sub-block)]: the slide is that many copies of each, as a multiset of pixels."""
        b = self.block
        every = ((self.ny * self.nx, b), (self.ny, b[:, :self.rx]), (self.nx, b[:self.ry]), (1, b[:self.ry, :self.rx]))
        return [(m, np.ascontiguousarray(s)) for m, s in every if m and s.size]

    def additive(self, f):
        """f over the whole slide for an additive uint64-valued f (stain_ref.moments, angle_hist, conc_hist with their operands
        bound): 29*46*f(block) + 29*f(block[:, :365]) + 46*f(block[:692]) + f(block[:692, :365]) at the slide-scale geometry."""
        return sum(np.uint64(m) * np.asarray(f(s), np.uint64) for m, s in self.parts())

    def additive_rows(self, f, y0, y1):
        """f over the rows y0 <= y < y1 (fewer than a block's), from one strip of the block."""
        assert 0 <= y0 < y1 <= self.shape[0] and y1 - y0 <= self.bh
        strip = self.block[(np.arange(y0, y1) % self.bh)]
        out = np.uint64(self.nx) * np.asarray(f(np.ascontiguousarray(strip)), np.uint64)
        return out + np.asarray(f(np.ascontiguousarray(strip[:, :self.rx])), np.uint64) if self.rx else out

    def __getitem__(self, key):
        yy, xx = (np.asarray(k) for k in key)
        h, w, _ = self.shape
        assert yy.min() >= 0 and yy.max() < h and xx.min() >= 0 and xx.max() < w, "index outside the slide"
        return self.block[yy % self.bh, xx % self.bw]

    def window(self, y0, x0, hh, ww):
        assert 0 <= y0 and y0 + hh <= self.shape[0] and 0 <= x0 and x0 + ww <= self.shape[1]
        return self.block[np.ix_(np.arange(y0, y0 + hh) % self.bh, np.arange(x0, x0 + ww) % self.bw)]

    def flat(self, addr):
        a = np.asarray(addr, np.int64)
        h, w, _ = self.shape
        assert a.min() >= 0 and a.max() < h * w * 3
        y, rem = np.divmod(a, 3 * w)
        return self.block[y % self.bh, (rem // 3) % self.bw, rem % 3]

    def device(self, dev):
        import torch
        h, w, _ = self.shape
        return repeat_on_device(torch.from_numpy(self.block).to(dev), h, w)


def repeat_on_device(block_dev, h, w):
    """block_dev[y % bh, x % bw] as a contiguous uint8[h, w, 3] on the block's device."""
    bh, bw = block_dev.shape[:2]
    return block_dev.repeat(-(-h // bh), -(-w // bw), 1)[:h, :w].contiguous()


def spots(h, w, P, over=False, seed=0):
    """int32[n, 2] tile origins.  For each edge E in (2^31, 2^32) that the slide reaches: the tile centred on the pixel that holds byte
    E, a tile whose first row starts in the row after E, a tile whose last row ends in the row before E.  Then the four corners
    ((h - P, w - P) holds the allocation's last byte) and four seeded random origins, all clamped into the slide.  `over` (the kernels
    that let a tile hang over the border): also (-3, -2) and (h - P + 2, w - P + 5)."""
    rb = 3 * w
    o = []
    for e in EDGES:
        if e >= h * rb:
            continue
        y, x = e // rb, e % rb // 3
        o += [(y - P // 2, x - P // 2), (y + 1, x - P // 2), (y - P, x - P // 2)]
    o += [(0, 0), (0, w - P), (h - P, 0), (h - P, w - P)]
    rng = np.random.default_rng(seed + P)
    o += [(int(rng.integers(0, h - P + 1)), int(rng.integers(0, w - P + 1))) for _ in range(4)]
    o = np.clip(np.asarray(o, np.int64), 0, [h - P, w - P])
    if over:
        o = np.concatenate([o, [[-3, -2], [h - P + 2, w - P + 5]]])
    return o.astype(np.int32)


def byte_span(origins, h, w, P):
    """(int64[n] offset of each tile's first byte inside the slide, int64[n] offset of its last byte inside the slide)."""
    o = np.asarray(origins, np.int64).reshape(-1, 2)
    y0, x0 = np.clip(o[:, 0], 0, h - 1), np.clip(o[:, 1], 0, w - 1)
    y1, x1 = np.clip(o[:, 0] + P - 1, 0, h - 1), np.clip(o[:, 1] + P - 1, 0, w - 1)
    return y0 * 3 * w + 3 * x0, y1 * 3 * w + 3 * x1 + 2


def assert_reaches_both_edges(origins, h, w, P):
    """The origins of a slide-scale case: a tile wholly on each side of 2^31 and of 2^32, a tile that holds each edge, and the tile that
    holds the allocation's last byte; min(offset) < 2^31 < 2^32 < max(offset)."""
    lo, hi = byte_span(origins, h, w, P)
    assert lo.min() < EDGES[0] < EDGES[1] < hi.max()
    for e in EDGES:
        assert (hi < e).any() and (lo > e).any() and ((lo <= e) & (e <= hi)).any(), e
    assert hi.max() == h * w * 3 - 1


# ---- what a wrapped address would read ------------------------------------------------------------------------------------------
def tile_addresses(origin, P, w):
    """int64[P, 3P]: the flat byte offset of every byte of the P x P tile at `origin` (inside the slide)."""
    y0, x0 = (int(v) for v in origin)
    return (np.arange(y0, y0 + P, dtype=np.int64) * (3 * w))[:, None] + (3 * x0 + np.arange(3 * P, dtype=np.int64))[None, :]


def wrapped(addr, w, modulus, rows_only=False):
    """`addr` as 32-bit (modulus 2^32) or 31-bit (2^31) arithmetic would form it: the whole offset truncated, or (`rows_only`) only the
    product y * row_bytes, the (int32)(y * row_bytes) of a kernel that adds the column part in 64 bits."""
    a = np.asarray(addr, np.int64)
    if not rows_only:
        return a % modulus
    row = a // (3 * w) * (3 * w)
    return row % modulus + (a - row)


def he_block(seed=11):
    """The 1021 x 1031 H&E block of the periodic slide.  The slide's last three pixels (the stain passes' tail: H * W % 16 == 3) are
    block[691, 362:365]; they are set to stained colours so that a dropped tail changes every statistic."""
    import stain_ref as R
    block = R.synth_he(BLOCK[0], BLOCK[1], seed, glass=0.3)
    block[(H - 1) % BLOCK[0], (W - 3) % BLOCK[1]:(W - 3) % BLOCK[1] + 3] = [[120, 60, 140], [90, 40, 120], [150, 80, 160]]
    return block


def same_bits(got, ref_f32):
    """A gather's output (torch tensor, f32 or bf16) against the float32 reference: the float32 bits, or the raw bits of torch's
    round-to-nearest-even conversion of the reference."""
    import torch
    ref = torch.from_numpy(np.ascontiguousarray(ref_f32))
    got = got.cpu()
    if got.dtype == torch.float32:
        return got.shape == ref.shape and torch.equal(got.view(torch.int32), ref.view(torch.int32))
    return got.shape == ref.shape and torch.equal(got.view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
