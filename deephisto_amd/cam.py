"""Fine whole-slide maps from the class activation maps of the last conv.

Both inference engines end in global average pool + fc, so a tile's logits are the mean over the positions of its last activation of
fc applied at each position.  `predict_fine_patched` keeps those per-position scores (`ResNetHIP.cam_tiles`: S x S rows per tile,
S = patch / 32, from the same forward pass) and accumulates each onto the 32 x 32-pixel block it belongs to
(`tiles.accumulate_cam`), so the map's values change every 32 pixels instead of once per tile footprint.  The plan -- tile list,
filters, shard range, launch size, the one all-gather, padding duplicates -- is `predict.predict_full_patched`'s, and the canvas
shape [h // d, w // d] does not move: everything behind the map takes it unchanged.
"""
from __future__ import annotations

import torch

from . import tiles
from .plan import (Lanes, _padded_logits, accumulation_list, exchange_rows, launch_tiles, normalised_first, pack, plan_tiles,
                   require_dense_resident)
from .quality import QualityFilter
from .tissue import TissueFilter, fill_uncovered

MAX_CLASSES = 64   # the probability kernels' limit, which the CAM head shares


@normalised_first
def predict_fine_patched(sampler, model, n_classes: int, downscale: int = 16, micro_batch: int | None = None, group=None,
                         streams: int = 2, dedupe_padding: bool = False, tissue: TissueFilter | None = None,
                         tissue_info: dict | None = None, quality: QualityFilter | None = None, quality_info: dict | None = None,
                         return_proba: bool = False, return_cam: bool = False):
    """Whole-slide prediction at the resolution of the last feature map: `predict_full_patched`'s plan with S x S rows per tile.

    Every tile that runs yields float32[S, S, n_classes] scores, S = patch / 32 (`model.cam_tiles`); the rows of all ranks are
    exchanged with the one all-gather (rows are S * S * n_classes wide) and accumulated over `plan.accumulation_list` -- padding
    duplicates and `dedupe_padding` mean what they mean in predict_full_patched -- by `tiles.accumulate_cam`: the ordered
    accumulation of the expanded list (`tiles.expand_positions`), bit for bit.  `tissue` / `quality` filter the tiles as there;
    cells no kept tile covers get the fill class.  Keyword-only `stain=` / `stain_info=`: see `plan.normalised_first`.
    `return_proba=True` appends a finished tiles.SlideProbabilities from the softmax of every position's scores
    (`tiles.accumulate_cam_probabilities`); `return_cam=True` the float32[n_padded, S, S, n_classes] rows in the padded list's
    order (NaN rows for rejected tiles, the padding duplicates copied from the corner tile).
    Refused with a ValueError: the random sampler, a streamed (ONDISK_MULTIPROC) slide, a patch size that is not a multiple of
    32, more than 64 classes.  There is no `tta`: a rotated view permutes the positions.
    Returns int64[h//d, w//d] on the device (then the rows, then the probabilities, when asked for)."""
    require_dense_resident(sampler, "predict_fine_patched")
    P = int(sampler.patch_size)
    if P % 32:
        raise ValueError(f"predict_fine_patched: patch {P} is not a multiple of 32 (a position is a 32 x 32-pixel block of the tile)")
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"predict_fine_patched: n_classes = {n_classes}, class activation maps take 1 to {MAX_CLASSES} classes")
    S = P // 32
    plan = plan_tiles(sampler, model, micro_batch, group, tissue, tissue_info, quality, quality_info)
    slide, o_dev, n = sampler.data_device, plan.o_dev, plan.hi - plan.lo
    local = torch.zeros((plan.per_rank, S * S * n_classes), dtype=torch.float32, device=o_dev.device)
    lanes = Lanes(model, streams, o_dev.device)
    entry = model.cam_entry()
    lanes.run(n, plan.mb, lambda handle, stream, s, e: launch_tiles(entry, handle, slide, sampler.h, sampler.w, o_dev, s, e, P, None,
                                                                    stream, feat=local))
    cam_work = exchange_rows(plan, local, group)
    return _finish(plan, cam_work, S, n_classes, downscale, dedupe_padding, return_proba, return_cam)


def _finish(plan, cam_work, S, n_classes, downscale, dedupe_padding, return_proba, return_cam):
    """`plan.finish` for rows of S * S positions: the fine accumulation over accumulation_list and argmax, the fill of uncovered
    cells, the fine mean probabilities over the same list, the rows scattered back to the padded list."""
    grid, kept, fill_class = plan.grid, plan.kept, plan.fill_class
    P, h, w = grid.patch_size, grid.h, grid.w
    rows, yx = accumulation_list(grid.origins, grid.n_unique, kept, dedupe_padding)
    n_dup = len(rows) - len(cam_work)   # the corner's padding duplicates: rows repeats the last row that often
    acc = (torch.cat([cam_work, cam_work[-1:].expand(n_dup, -1)]) if n_dup else cam_work).contiguous().view(-1, S, S, n_classes)
    if len(rows):
        _, cmap = tiles.accumulate_cam(acc, yx, P, downscale, h, w)
    else:   # all glass: no forward ran, every cell is uncovered
        cmap = torch.zeros((h // downscale, w // downscale), dtype=torch.int64, device=cam_work.device)
    if fill_class is not None:
        fill_uncovered(cmap, plan.kept_yx_dev, P, downscale, h, w, fill_class)
    extra = []
    if return_cam:
        extra.append(_padded_logits(cam_work, kept, grid.n_unique, len(grid.origins)).view(-1, S, S, n_classes))
    if return_proba:   # the same list right after the class map: the bin plan is reused
        extra.append(tiles.accumulate_cam_probabilities(acc, yx, P, downscale, h, w, fill_class=-1 if fill_class is None else fill_class))
    return pack(cmap, *extra)
