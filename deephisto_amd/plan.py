"""The tile plan behind whole-slide prediction (`predict.predict_full_patched`) and tile embeddings (`embeddings.extract_embeddings`).

Over a dense sampler's grid (`TileGrid`): `filter_tiles` composes the kept list of the tissue and quality stages; `plan_tiles` takes the
rank's `shard_range` of it and sizes the launches with `launch_size` (`TilePlan`); `Lanes` spreads the launches (`launch_tiles`) over
`streams` HIP streams with one inference handle each; `exchange_rows` is the one all-gather and `finish` the tail.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import tiles
from ._lib import check
from .patch_samplers.full_samplers import FullImageDenseSampler
from .quality import check_fill_classes, score_quality
from .stain import StainNormalizer
from .tissue import fill_uncovered, score_tiles


def shard_range(n_items: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous [lo, hi) share of `n_items` for `rank` (sizes differ by at most 1)."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


_SIDE_STREAMS: dict = {}


def _side_stream(dev, i):
    key = (dev.index, i)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


def exchange_logits(local: torch.Tensor, n_unique: int, group=None) -> torch.Tensor:
    """The one exchange step of the sharded path: all-gather of per-tile logits.

    `local` is this rank's float32[ceil(n_unique/world), n_cls] block (its first
    hi-lo rows are real, the rest padding); returns float32[n_unique, n_cls] in the
    reference's tile order on every rank.  RCCL (backend "nccl") on GPUs; the same
    code runs on gloo/CPU tensors in the tests."""
    import torch.distributed as dist

    world = dist.get_world_size(group)
    per_rank = local.shape[0]
    gathered = torch.empty((world * per_rank, local.shape[1]), dtype=local.dtype, device=local.device)
    try:
        dist.all_gather_into_tensor(gathered, local.contiguous(), group=group)
    except NotImplementedError:  # a backend without the flat form; a real RCCL failure (RuntimeError) must surface, not be retried
        parts = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(parts, local.contiguous(), group=group)
        gathered = torch.cat(parts)
    rows = []
    for r in range(world):
        lo, hi = shard_range(n_unique, world, r)
        rows.append(gathered[r * per_rank:r * per_rank + (hi - lo)])
    return torch.cat(rows)


def launch_size(n_tiles: int, micro_batch: int) -> int:
    """Tiles per kernel launch for a rank's `n_tiles` under the cap `micro_batch` (never more than `micro_batch`).

    Near-equal launches instead of full ones plus a short tail, each a MULTIPLE OF 128 TILES (all but the last): the persistent
    kernels run one tile per workgroup per iteration on 256 CUs (stem: 768 workgroups), and a layer has 8 / 4 / 2 / 2 conv tiles
    per 256 x 256 image, so only multiples of 128 images fill the last iteration of every layer.  38 416 tiles as 10 x 3 842 paid
    an almost empty extra iteration in every layer of every launch (121 instead of 120.06 in layer 1, 31 instead of 30.02 in
    layers 3-4, 26 instead of 25.01 in the stem: ~2 % of the slide); 9 x 3 968 + 2 704 does not."""
    if n_tiles <= micro_batch:
        return micro_batch
    per = -(-n_tiles // -(-n_tiles // micro_batch))
    if micro_batch < 128 or os.environ.get("DH_MB_ALIGN") == "0":   # A/B: the round-3 rule (equal launches, any size)
        return per
    return min(micro_batch, max(128, -(-per // 128) * 128))


def accumulation_list(origins: np.ndarray, n_unique: int, kept: np.ndarray | None = None,
                      dedupe_padding: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """The ordered list predict_full_patched accumulates: (int64 row indices into the exchanged logits, int32 origins).

    `origins` is the sampler's padded list, whose first `n_unique` entries are the grid and whose rest repeat the corner tile
    (index n_unique - 1); `kept` holds the ascending indices of the unique tiles that ran (None: all of them), one logits row
    each.  The list is those tiles in grid order; the padding duplicates follow only when the corner is among them and
    `dedupe_padding` is false, each repeating the last row with its origin from the padded list."""
    tile = np.arange(n_unique, dtype=np.int64) if kept is None else np.asarray(kept, dtype=np.int64)
    rows, yx = np.arange(len(tile), dtype=np.int64), origins[:n_unique][tile]
    if len(origins) > n_unique and not dedupe_padding and len(tile) and tile[-1] == n_unique - 1:
        rows = np.concatenate([rows, np.full(len(origins) - n_unique, len(tile) - 1, dtype=np.int64)])
        yx = np.concatenate([yx, origins[n_unique:]])
    return rows, yx


def pack(cmap, *optional):
    """What a predict function returns: the bare map, or (cmap[, logits | canvas][, proba]) when more was asked for."""
    return (cmap, *optional) if optional else cmap


def normalised_first(predict):
    """Gives a predict function the keyword-only arguments `stain=None, stain_info=None`.

    With a StainNormalizer the sampler's resident slide is fitted and normalised on the device, and the UNCHANGED function runs
    over a sampler whose resident slide is `stain.normalize(slide)`: class map, logits, probabilities, the tissue filter's kept
    list and Otsu threshold are those of that slide.  The normalised copy takes the place of the sampler's device slide for the
    duration of the call and the sampler's own tensor is put back, never written (so one sampler must not be used from two
    threads at once).  Under torch.distributed every rank normalises its own copy: fit and pixels are integer-exact, hence
    identical without an exchange.  A streamed (ONDISK_MULTIPROC) sampler is refused.  `stain_info`: a dict that receives the
    StainFit under "fit".  Positional parameters and their order stay those of the wrapped function."""
    @functools.wraps(predict)
    def with_stain(sampler, *args, stain: StainNormalizer | None = None, stain_info: dict | None = None, **kwargs):
        if stain is None:
            return predict(sampler, *args, **kwargs)
        if not sampler.resident:
            raise ValueError("stain normalisation needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
        raw = sampler.data_device
        sampler._dev = stain.normalize(raw, stain_info)
        try:
            return predict(sampler, *args, **kwargs)
        finally:
            sampler._dev = raw
    # what inspect shows stays the positional parameters, which are the reference's: the keyword-only additions (these two, and
    # `tta=` / `tta_info=` of the wrapped function, which pass through **kwargs) are described in the docstrings
    sig = inspect.signature(predict)
    with_stain.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.kind is not p.KEYWORD_ONLY])
    return with_stain


# ---- the grid and the plan over it ------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class TileGrid:
    """What the plan and its tail read of a dense sampler: the padded origin list (int32[n_padded, 2]: the `n_unique` tiles of the
    grid in the reference's order, then copies of the corner tile) and its geometry."""
    origins: np.ndarray
    n_unique: int
    patch_size: int
    h: int
    w: int

    @classmethod
    def of_sampler(cls, sampler) -> "TileGrid":
        return cls(sampler.origins, sampler.n_tiles, sampler.patch_size, sampler.h, sampler.w)

    @classmethod
    def from_geometry(cls, h: int, w: int, patch_size: int, stride: int, n_unique: int, n_padded: int) -> "TileGrid":
        """The grid of a sampler that is no longer at hand, rebuilt from what a SlideEmbeddings stores of it."""
        o, n_u = tiles.tile_grid(h, w, patch_size, stride, 1)
        if n_u != n_unique:
            raise ValueError("the stored geometry does not reproduce the tile grid")
        pad = np.repeat(o[n_u - 1:n_u], n_padded - n_u, axis=0)
        return cls(np.concatenate([o[:n_u], pad]) if len(pad) else o[:n_u], n_u, patch_size, h, w)


def require_dense_resident(sampler, who: str) -> None:
    """The two refusals of everything that scores or reads the unique tiles of a resident slide; `who` opens the message."""
    if not isinstance(sampler, FullImageDenseSampler):
        raise ValueError(f"{who} works on the dense sampler's grid only (not on the random sampler's branch)")
    if not sampler.resident:
        raise ValueError(f"{who} needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")


def filter_tiles(sampler, tissue=None, tissue_info: dict | None = None, quality=None, quality_info: dict | None = None):
    """The tissue stage, then the quality stage over the tiles it kept (all unique tiles without one), on the sampler's resident
    slide.  Returns (kept, kept_yx_dev, fill_class): the ascending int64 indices of the tiles both stages kept (integer-exact: the
    same on every rank), their int32[k, 2] origins on the device and the class of the cells none of them covers; None, None, None
    without a filter.  `tissue_info` receives the tissue stage's info and list, `quality_info` the quality stage's and the composition."""
    for filt, who in ((tissue, "the tissue filter"), (quality, "the quality filter")):
        if filt is not None:
            require_dense_resident(sampler, who)
    check_fill_classes(tissue, quality)
    if tissue is None and quality is None:
        return None, None, None
    slide, P, unique = sampler.data_device, sampler.patch_size, sampler.origins[:sampler.n_tiles]
    kept, kept_yx_dev, threshold = None, torch.from_numpy(unique).to(slide.device), -1
    if tissue is not None:
        idx_dev, kept_yx_dev, info = score_tiles(slide, kept_yx_dev, P, tissue, unique)
        kept, threshold = idx_dev.cpu().numpy().astype(np.int64), info["threshold"]
        if tissue_info is not None:
            tissue_info.update(info, kept=kept)
    if quality is not None:
        # sharpness is measured over the pixels the tissue stage calls tissue (its resolved threshold; -1: every pixel)
        idx_dev, kept_yx_dev, info = score_quality(slide, kept_yx_dev, P, threshold, quality, unique if kept is None else unique[kept])
        q = idx_dev.cpu().numpy().astype(np.int64)
        kept = q if kept is None else kept[q]
        if quality_info is not None:
            quality_info.update(info, kept=kept)
    return kept, kept_yx_dev, (tissue if quality is None else quality).fill_class


@dataclass(frozen=True, eq=False)
class TilePlan:
    """Of the `n_work` tiles that run (`kept`, or every unique tile of `grid` for None), `rank` of `world` takes [lo, hi), whose
    origins are `o_dev`, in launches of `mb` tiles; its rows land in a block of `per_rank` rows, the size every rank exchanges."""
    grid: TileGrid
    kept: np.ndarray | None
    kept_yx_dev: torch.Tensor | None
    fill_class: int | None
    world: int
    rank: int
    lo: int
    hi: int
    n_work: int
    per_rank: int
    mb: int
    o_dev: torch.Tensor


def plan_shard(grid: TileGrid, world: int, rank: int, micro_batch: int, device, kept=None, kept_yx_dev=None, fill_class=None) -> TilePlan:
    """The TilePlan of `rank` among `world`; without a kept list: host arithmetic and one copy of origins to `device` (CPU or GPU)."""
    n_work = grid.n_unique if kept is None else len(kept)
    lo, hi = shard_range(n_work, world, rank)
    o_dev = torch.from_numpy(grid.origins[lo:hi]).to(device) if kept is None else kept_yx_dev[lo:hi]
    return TilePlan(grid, kept, kept_yx_dev, fill_class, world, rank, lo, hi, n_work, -(-n_work // world),
                    launch_size(hi - lo, micro_batch), o_dev)


def plan_tiles(sampler, model, micro_batch: int | None = None, group=None, tissue=None, tissue_info: dict | None = None,
               quality=None, quality_info: dict | None = None) -> TilePlan:
    """The plan of this process: the sampler's grid, filtered, sharded over the ranks of `group` when torch.distributed runs more
    than one, in launches of at most `micro_batch` tiles (None: `model.default_micro_batch()`, the most one launch takes)."""
    import torch.distributed as dist

    kept, kept_yx_dev, fill_class = filter_tiles(sampler, tissue, tissue_info, quality, quality_info)
    grid = TileGrid.of_sampler(sampler)
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    world, rank = (dist.get_world_size(group), dist.get_rank(group)) if distributed else (1, 0)
    dev = sampler.data_device.device if sampler.resident else sampler.device
    return plan_shard(grid, world, rank, micro_batch or model.default_micro_batch(), dev, kept, kept_yx_dev, fill_class)


# ---- launches ---------------------------------------------------------------------------------------------------------------
class Lanes:
    """`streams` inference handles of `model` (parameters are synced once, here), each with its own workspace and HIP stream, so
    that the short kernels and the tails of one micro-batch overlap with the convolutions of the next."""

    def __init__(self, model, streams: int, dev):
        self.handles = model.eval().lane_handles(max(1, streams))
        self.main = torch.cuda.current_stream(dev)
        self.streams = [self.main] + [_side_stream(dev, i) for i in range(1, len(self.handles))]

    def run(self, n: int, mb: int, launch) -> None:
        """`launch(handle, stream, s, e)` per range of `mb` rows of [0, n), round-robin over lanes forked from and joined into main."""
        for st in self.streams[1:]:
            st.wait_stream(self.main)
        for k, s in enumerate(range(0, n, mb)):
            lane = k % len(self.handles)
            launch(self.handles[lane], self.streams[lane], s, min(s + mb, n))
        for st in self.streams[1:]:
            self.main.wait_stream(st)


def launch_tiles(entry, handle, slide, h, w, o_dev, s, e, P, logits, stream, feat=None):
    """One launch of `entry` (`model.tiles_entry()`, or `model.features_entry()` with `feat`) over rows [s, e) of the int32[n, 2] `o_dev`
    in the uint8[h, w, 3] `slide`, into rows [s, e) of float32[n, n_classes] `logits` (None with `feat`: no fc) and float32[n, D] `feat`."""
    fwd, fwd_name = entry
    lg = None if logits is None else logits.data_ptr() + 4 * logits.shape[1] * s
    out = (lg,) if feat is None else (feat.data_ptr() + 4 * feat.shape[1] * s, lg)
    check(fwd(handle, slide.data_ptr(), h, w, o_dev.data_ptr() + 8 * s, e - s, P, *out, C.c_void_p(stream.cuda_stream)), fwd_name)


def exchange_rows(plan: TilePlan, local: torch.Tensor, group=None, timing: list | None = None) -> torch.Tensor:
    """This rank's float32[per_rank, C] block -> the `n_work` rows of all ranks in tile order: ONE all-gather (`exchange_logits`)
    when the plan is sharded and a tile ran anywhere.  `timing` receives one (start, end) pair of HIP events around it."""
    if plan.world == 1 or plan.n_work == 0:   # alone, or every rank rejected every tile: nothing to exchange
        return local[:plan.n_work]
    if timing is None or not local.is_cuda:
        return exchange_logits(local, plan.n_work, group)
    main = torch.cuda.current_stream(local.device)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(main)
    rows = exchange_logits(local, plan.n_work, group)
    ev[1].record(main)
    timing.append(ev)
    return rows


# ---- the tail ---------------------------------------------------------------------------------------------------------------
def finish(grid: TileGrid, logits_work, kept, kept_yx_dev, downscale, dedupe_padding, fill_class: int | None, return_logits,
           return_proba):
    """The tail of predict_full_patched: `logits_work` holds one row per tile that ran (`kept`, or every unique tile for None: the
    unfiltered run is the filtered one with every tile kept).  Ordered accumulation over accumulation_list and argmax; with a
    tile filter (`fill_class` not None) the fill of the cells no kept tile covers; the probabilities over the same list (uncovered
    cells: count 0 and the fill class); the logits scattered back to the padded list (NaN rows for rejected tiles)."""
    origins, n_unique, P, h, w = grid.origins, grid.n_unique, grid.patch_size, grid.h, grid.w
    rows, yx = accumulation_list(origins, n_unique, kept, dedupe_padding)
    n_dup = len(rows) - len(logits_work)   # the corner's padding duplicates: rows repeats the last row that often
    acc = (torch.cat([logits_work, logits_work[-1:].expand(n_dup, -1)]) if n_dup else logits_work).contiguous()
    if len(rows):
        _, cmap = tiles.accumulate_logits(acc, yx, P, downscale, h, w)
    else:   # all glass: no forward ran, every cell is uncovered
        cmap = torch.zeros((h // downscale, w // downscale), dtype=torch.int64, device=logits_work.device)
    if fill_class is not None:
        fill_uncovered(cmap, kept_yx_dev, P, downscale, h, w, fill_class)
    extra = []
    if return_proba:   # the same list right after the class map: the bin plan is reused
        extra.append(tiles.accumulate_probabilities(acc, yx, P, downscale, h, w, fill_class=-1 if fill_class is None else fill_class))
    if return_logits:
        whole = kept is None and len(acc) == len(origins)   # the accumulated tensor is the padded list already
        extra.insert(0, acc if whole else _padded_logits(logits_work, kept, n_unique, len(origins)))
    return pack(cmap, *extra)


def _padded_logits(logits_work, kept, n_unique, n_padded):
    """float32[n_padded, n_cls]: the rows of `logits_work` at their tiles' places in the padded list, NaN for rejected tiles,
    the padding duplicates copied from the corner tile."""
    pad = n_padded - n_unique
    if kept is None:
        return torch.cat([logits_work, logits_work[-1:].expand(pad, -1)]) if pad else logits_work
    logits = torch.full((n_padded, logits_work.shape[1]), float("nan"), dtype=torch.float32, device=logits_work.device)
    if len(kept):
        logits[torch.from_numpy(kept).to(logits.device)] = logits_work
    if pad:
        logits[n_unique:] = logits[n_unique - 1]
    return logits
