"""Test-time augmentation of whole-slide prediction over the eight dihedral views of the slide.

Histology has no up, down, left or right; a trained network only approximates that.  `TestTimeAugmenter` names a set of
orientations of the square (the dihedral group D4), `predict_full_patched(..., tta=...)` and `predict_random_patched(..., tta=...)`
classify every tile in each of them and average the logits.  A mirrored or turned tile of the slide is the plain tile, at a mapped
origin, of the mirrored or turned slide, so a view of the whole slide is another resident slide: `dihedral_view` builds it
(`dh_slide_dihedral`, csrc/dihedral.hip), `map_origins` maps the tile origins, and the fused gather + network entry runs unchanged.

    view = k + 4 f, k in 0..3, f in 0..1:    dst = np.rot90(np.fliplr(src) if f else src, k)      names: VIEWS[view]

One quarter turn of an H x W slide sends the origin (y, x) of a P x P tile to (W - P - x, y) and the slide to W x H; the mirror
sends it to (y, W - P - x).  The host tables and the origin mapping below need no GPU.
"""
from __future__ import annotations

import numbers

import numpy as np

from .resample import MAX_SIDE, _check_source, _overlap

VIEWS = ("r0", "r90", "r180", "r270", "r0f", "r90f", "r180f", "r270f")
NAMED_SETS = {
    "d4": VIEWS,
    "flips": ("r0", "r0f", "r180f", "r180"),          # identity, fliplr, flipud, both
    "rot": ("r0", "r90", "r180", "r270"),
}

# the kernel's tiling constants (csrc/dihedral.hip: kTile, kThreads, kChunk, kPitch)
TILE = 64                       # a workgroup moves TILE x TILE pixels through LDS
THREADS = 256
STORE_GROUP = 16                # bytes per load; destination rows leave in aligned groups of as many bytes
LDS_PITCH = 3 * TILE + 4        # 196 bytes = 49 dwords a tile row: odd, so a column walk changes bank with every row


def view_id(view) -> int:
    """The id 0..7 of a view given by name (VIEWS) or id; anything else is refused by name."""
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError(f"unknown view {view!r} (one of {', '.join(VIEWS)})")
        return VIEWS.index(view)
    if isinstance(view, bool) or not isinstance(view, numbers.Integral) or not 0 <= view < 8:
        raise ValueError(f"unknown view {view!r} (a name out of {', '.join(VIEWS)} or an id in 0..7)")
    return int(view)


def view_shape(h: int, w: int, view) -> tuple[int, int]:
    """(h, w) of the view of an h x w slide: swapped by the quarter turns."""
    return (int(w), int(h)) if view_id(view) & 1 else (int(h), int(w))


def compose(a, b) -> int:
    """The id of "view `a`, then view `b` of the result".  With r the quarter turn and s the mirror, view = r^k s^f and
    s r = r^-1 s, so r^kb s^fb r^ka s^fa = r^(kb -+ ka) s^(fa + fb), minus when fb is set."""
    a, b = view_id(a), view_id(b)
    ka, fa, kb, fb = a & 3, a >> 2, b & 3, b >> 2
    return ((kb - ka if fb else kb + ka) & 3) | (fa ^ fb) << 2


def inverse(a) -> int:
    """The id of the view that undoes `a`: a turn by the opposite angle; every mirrored view undoes itself."""
    a = view_id(a)
    return a if a >> 2 else -a & 3


COMPOSE = tuple(tuple(compose(a, b) for b in range(8)) for a in range(8))     # COMPOSE[a][b] == compose(a, b)
INVERSE = tuple(inverse(a) for a in range(8))


def _map(y, x, h, w, patch, v):
    """The mirror, then k quarter turns, on origin columns y, x of any integer array type that has + and -."""
    if v >> 2:
        x = w - patch - x
    for _ in range(v & 3):
        y, x, h, w = w - patch - x, y, w, h
    return y, x


def _check_geometry(h, w, patch):
    if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"slide of {h} x {w}: sides must be in [1, {MAX_SIDE}]")
    if patch < 1:
        raise ValueError(f"patch size {patch} must be positive")


def map_origins(origins_yx, h: int, w: int, patch: int, view) -> np.ndarray:
    """int32[n, 2]: where the `patch` x `patch` tiles at `origins_yx` (y, x) of an h x w slide lie in its view `view`:
    view_np(slide)[y':y'+P, x':x'+P] == view_np(slide[y:y+P, x:x+P])."""
    v = view_id(view)
    _check_geometry(h, w, patch)
    o = np.asarray(origins_yx)
    if o.ndim != 2 or o.shape[1] != 2 or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f"origins must be an integer array [n, 2], not {o.dtype}{list(o.shape)}")
    o = o.astype(np.int64)
    y, x = _map(o[:, 0], o[:, 1], int(h), int(w), int(patch), v)
    return np.stack([y, x], axis=1).astype(np.int32)


def map_origins_device(origins_dev, h: int, w: int, patch: int, view):
    """The device twin of map_origins: a contiguous int32[n, 2] tensor on the device of `origins_dev` (int32[n, 2])."""
    import torch
    v = view_id(view)
    _check_geometry(h, w, patch)
    if not isinstance(origins_dev, torch.Tensor) or origins_dev.dtype != torch.int32 or origins_dev.dim() != 2 or origins_dev.shape[1] != 2:
        raise ValueError("origins must be an int32[n, 2] tensor")
    if v == 0:
        return origins_dev.contiguous()
    y, x = _map(origins_dev[:, 0], origins_dev[:, 1], int(h), int(w), int(patch), v)
    return torch.stack([y, x], dim=1).to(torch.int32).contiguous()


# ---- device entry -----------------------------------------------------------------------------------------------------------
def dihedral_view(slide, view, out=None):
    """uint8[h', w', 3] on the slide's device: view `view` (a name out of VIEWS or an id) of `slide` (uint8[h, w, 3], contiguous,
    in GPU memory), (h', w') = view_shape(h, w, view); every byte is a source byte.  `out`: where to write, a contiguous uint8
    buffer of h * w * 3 elements (of any shape) on the same device that does not overlap the slide; the result is a view of it."""
    import torch
    from ._lib import check, lib
    from .tiles import _stream
    v = view_id(view)
    h, w = _check_source(slide)
    if h < 1 or w < 1:
        raise ValueError(f"slide of {h} x {w} has no pixel")
    if out is None:
        out = torch.empty(h * w * 3, dtype=torch.uint8, device=slide.device)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != slide.device
                or out.numel() != h * w * 3 or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 buffer of {h} * {w} * 3 = {h * w * 3} elements on {slide.device}")
        if _overlap(slide, out):
            raise ValueError("out must not overlap the slide")
    check(lib().dh_slide_dihedral(slide.data_ptr(), h, w, v, out.data_ptr(), _stream(slide.device)), "dh_slide_dihedral")
    return out.view(*view_shape(h, w, v), 3)


class TestTimeAugmenter:
    """The views a prediction is averaged over, and how.

    `views`: "d4" (all eight), "flips" (r0, r0f, r180f, r180), "rot" (r0 .. r270) or a sequence of names out of VIEWS; an empty
    sequence, an unknown name and a duplicate are refused by name.  The combination is the mean of the per-view logits in the
    order of `views`, in float32, exactly: acc = L[0]; acc += L[k] for k = 1 ..; acc *= float32(1 / V).  The order is part of
    the contract.  Probabilities are not averaged per view: `return_proba=True` takes the softmax of the averaged logits."""

    __test__ = False            # a class of the package, not a test case

    def __init__(self, views="d4"):
        if isinstance(views, str):
            if views not in NAMED_SETS:
                raise ValueError(f"unknown view set {views!r} (one of {', '.join(NAMED_SETS)}, or a sequence of names out of "
                                 f"{', '.join(VIEWS)})")
            views = NAMED_SETS[views]
        views = tuple(views)
        if not views:
            raise ValueError("test-time augmentation needs at least one view: the sequence is empty")
        for k, name in enumerate(views):
            if not isinstance(name, str) or name not in VIEWS:
                raise ValueError(f"unknown view {name!r} (one of {', '.join(VIEWS)})")
            if name in views[:k]:
                raise ValueError(f"duplicate view {name!r}")
        self.views = views
        self.ids = tuple(VIEWS.index(name) for name in views)

    def __len__(self):
        return len(self.views)

    def __repr__(self):
        return f"TestTimeAugmenter({list(self.views)!r})"

    @property
    def scale(self) -> float:
        """1 / V; applied as a float32."""
        return 1.0 / len(self.views)

    def fold(self, acc, logits, k: int):
        """Step k of the combination, in place on `acc`: view k's float32 logits are copied (k = 0) or added."""
        return acc.copy_(logits) if k == 0 else acc.add_(logits)

    def finish(self, acc):
        """The last step, in place: acc *= float32(1 / V)."""
        return acc.mul_(self.scale)

    def combine(self, per_view):
        """The mean of the float32 logits tensors `per_view` (one per view, in the order of `views`), by the stated fold."""
        per_view = list(per_view)
        if len(per_view) != len(self.views):
            raise ValueError(f"{len(per_view)} logits tensors for {len(self.views)} views")
        acc = per_view[0].clone()
        for k in range(1, len(per_view)):
            self.fold(acc, per_view[k], k)
        return self.finish(acc)


def as_augmenter(tta) -> TestTimeAugmenter | None:
    """`tta` as the predict functions take it: None, a TestTimeAugmenter, or what its constructor takes."""
    return tta if tta is None or isinstance(tta, TestTimeAugmenter) else TestTimeAugmenter(tta)
