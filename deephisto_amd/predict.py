"""The device engine of whole-slide prediction (re-exported by examples/predict_full_patched.py, where the CLI lives).

`predict_full_patched(...)` is the device-resident fast path used by bench.py: tile ranges are sharded over the ranks of a
torch.distributed job (RCCL over xGMI), every rank runs fused gather+ResNet on its range (`_launch_tiles`, in launches of
`launch_size`), per-tile logits are all-gathered (`exchange_logits`), and the ordered accumulation + argmax run once over
`accumulation_list` (`_finish`).  `predict_random_patched(...)` is the same for the random sampler's branch (device coverage map,
large forward launches, one ordered accumulation).  With `return_proba=True` both also return the per-cell mean softmax
probabilities, hit counts, their class map and confidence (`tiles.SlideProbabilities`).
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import os

import numpy as np
import torch

from . import tiles
from ._lib import check
from .models.patch_cls_simple.engine import ResNetHIP
from .patch_samplers.full_samplers import FullImageDenseSampler
from .stain import StainNormalizer
from .quality import QualityFilter, check_fill_classes, score_quality
from .tissue import TissueFilter, fill_uncovered, score_tiles
from .tta import TestTimeAugmenter, as_augmenter, dihedral_view, map_origins_device, view_shape


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


def _pack(cmap, *optional):
    """What a predict function returns: the bare map, or (cmap[, logits | canvas][, proba]) when more was asked for."""
    return (cmap, *optional) if optional else cmap


def _normalised_first(predict):
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


def _launch_tiles(fwd, fwd_name, handle, slide, h, w, o_dev, s, e, P, out, n_classes, stream):
    """One launch of the model's fused tiles entry over rows [s, e) of the int32[n, 2] origins `o_dev` in the uint8[h, w, 3]
    `slide`; the logits land in rows [s, e) of the float32[n, n_classes] `out`."""
    check(fwd(handle, slide.data_ptr(), h, w, o_dev.data_ptr() + 8 * s, e - s, P, out.data_ptr() + 4 * n_classes * s,
              C.c_void_p(stream.cuda_stream)), fwd_name)


@_normalised_first
def predict_full_patched(sampler: FullImageDenseSampler, model, n_classes: int,
                         downscale: int = 16, micro_batch: int | None = None, group=None,
                         return_logits: bool = False, streams: int = 2, dedupe_padding: bool = False, timing: list | None = None,
                         tissue: TissueFilter | None = None, tissue_info: dict | None = None, return_proba: bool = False, *,
                         tta: TestTimeAugmenter | None = None, tta_info: dict | None = None,
                         quality: QualityFilter | None = None, quality_info: dict | None = None):
    """Device-resident whole-slide prediction (rows a1-a8 end to end).

    `model`: ResNet18HIP or ResNet50HIP; it names its own fused entry (`tiles_entry`) and launch size
    (`default_micro_batch`: ResNet-18 4 096 bf16 / 1 024 float32, ResNet-50 1 024).
    Single process: every tile (padding duplicates included) goes through the fused
    gather+network kernels in micro-batches, logits stay in HBM, one ordered
    accumulate + argmax.  Under torch.distributed (one process per GPU, backend
    "nccl" = RCCL): rank r takes the contiguous range shard_range(n_unique, world, r)
    of the reference-ordered origin list, logits are exchanged with ONE all-gather
    (n_unique x n_cls floats in total), and every rank finishes the map; the corner
    tile's padding duplicates are reconstructed from the gathered logits so the
    canvas equals the single-GPU / reference result.
    `dedupe_padding=True` leaves the padding duplicates of the corner tile out of the accumulation (the reference adds them,
    predict_full_patched.py:49-54, which is the default here).
    `timing`: a list that receives one (start, end) pair of HIP events around the all-gather (bench.py's `allgather_ms`).
    `tissue`: a TissueFilter: the unique tiles are scored on the device and only the kept ones run through
    the network (sharded over the ranks like the full list: every rank computes the same kept list); the ordered accumulation
    runs over the kept tiles (the corner's padding duplicates follow the corner), then the map cells no kept tile covers get
    `tissue.fill_class`.  The result is the unmasked computation with the rejected tiles' logits left out.  Needs a resident
    dense sampler.  `tissue_info`: a dict that receives threshold, min_pixels, n_tiles, n_kept, kept (int64 indices into the
    unique tiles) and, after Otsu, histogram.
    `return_proba=True` appends a tiles.SlideProbabilities to what is returned: per-cell mean softmax probability, hit
    count, argmax of the mean and confidence, from the same logits and the same tile list as the
    class map (so sharded, streamed and `dedupe_padding` runs give it too).  By default the corner tile's padding duplicates
    are added and counted like every other list entry, which weights the corner tile 1 + pad times in its footprint;
    `dedupe_padding=True` removes that.  With `tissue` it runs over the kept tiles only (a rejected tile's NaN row never
    enters a softmax) and uncovered cells get `tissue.fill_class`.
    Keyword-only `stain=` / `stain_info=`: see `_normalised_first`, which wraps this function.
    Keyword-only `tta`: a tta.TestTimeAugmenter (or what its constructor takes): every tile is classified
    in each of the augmenter's dihedral views and the logits are averaged per tile, in the order of the views, before the
    exchange; tile list, tissue filter, shard range, launch size, the one all-gather and everything behind it are those of
    the plain run, which sees one logits row per tile as before.  A view of the slide is built once per view into one reused
    buffer of the slide's size (peak memory: the slide plus one copy) and the unchanged fused entry runs over the mapped
    origins; every rank transforms its own copy (the bytes are exact, nothing is exchanged).  Needs a resident slide.  `stain=`
    composes: the views are those of the normalised slide.  `tta_info`: a dict that receives views (names) and
    n_forward_tiles (tiles x views on this rank).  None leaves every code path and every bit as it is.
    Keyword-only `quality`: a quality.QualityFilter: the tiles that survived the tissue stage (all unique
    tiles without one) are measured on the device and the out-of-focus and ink-marked ones are left out; the composition of the
    two stages is the kept list, which drives everything the tissue list drives above.  Sharpness is measured over the pixels
    the tissue filter calls tissue (its resolved threshold; without a tissue filter over every pixel).  Uncovered cells get
    `quality.fill_class`, which must equal `tissue.fill_class` when both are given.  Needs a resident dense sampler.  The sums
    are computed once, on the slide the prediction reads (`stain=`: the normalised one; `tta=`: the untransformed one).
    `quality_info`: a dict that receives threshold, min_sharpness, max_ink_pixels, n_tiles, n_kept, rejected_blur,
    rejected_ink, stats (int64[n, 4]) and reason (uint8[n]) of the scored tiles, and kept: the final list, as int64 indices into
    the unique tiles.  `tissue_info` keeps the tissue stage's list.  None leaves every code path and every bit as it is.
    Returns int64[h//d, w//d] on the device (and the float32[n_padded, n_cls] logits; rows of rejected tiles are NaN).
    """
    import torch.distributed as dist

    streamed = not sampler.resident          # ONDISK_MULTIPROC: row strips are uploaded as they are needed
    tta = as_augmenter(tta)
    if tta is not None and streamed:
        raise ValueError("test-time augmentation needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
    if tissue is not None:
        if not isinstance(sampler, FullImageDenseSampler):
            raise ValueError("the tissue filter works on the dense sampler's grid only (not on the random sampler's branch)")
        if streamed:
            raise ValueError("the tissue filter needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
    if quality is not None:
        if not isinstance(sampler, FullImageDenseSampler):
            raise ValueError("the quality filter works on the dense sampler's grid only (not on the random sampler's branch)")
        if streamed:
            raise ValueError("the quality filter needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
        check_fill_classes(tissue, quality)
    slide = None if streamed else sampler.data_device
    dev = sampler.device if streamed else slide.device
    P = sampler.patch_size
    origins = sampler.origins                      # padded, reference order
    n_unique = sampler.n_tiles
    kept = kept_yx_dev = None
    if tissue is not None:
        # the launch list becomes the kept tiles, in grid order (integer-exact: the same on every rank)
        kept_idx_dev, kept_yx_dev, info = score_tiles(slide, torch.from_numpy(origins[:n_unique]).to(dev), P, tissue,
                                                      origins[:n_unique])
        kept = kept_idx_dev.cpu().numpy().astype(np.int64)
        if tissue_info is not None:
            tissue_info.update(info, kept=kept)
    if quality is not None:
        # the second stage runs over the tiles the first one kept; the final list is the composition of the two
        t = -1 if tissue is None else info["threshold"]
        scored = torch.from_numpy(origins[:n_unique]).to(dev) if kept is None else kept_yx_dev
        q_idx_dev, kept_yx_dev, qinfo = score_quality(slide, scored, P, t, quality,
                                                      origins[:n_unique] if kept is None else origins[:n_unique][kept])
        q = q_idx_dev.cpu().numpy().astype(np.int64)
        kept = q if kept is None else kept[q]
        if quality_info is not None:
            quality_info.update(qinfo, kept=kept)
    n_work = n_unique if kept is None else len(kept)
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    lo, hi = shard_range(n_work, world, rank)
    # tiles per kernel launch (independent of the sampler's batch size).  bf16: 4 096, the library's maximum (a 64 x 64 x 64-channel
    # map of 4 096 tiles is 2 GiB).  float32: 1 024 -- the same map would be 4 GiB per tensor at 4 096 tiles, past the 32-bit byte
    # offsets of the conv schedule tables (the library refuses it)
    mb = launch_size(hi - lo, micro_batch or model.default_micro_batch())
    o_dev = torch.from_numpy(origins[lo:hi]).to(dev) if kept is None else kept_yx_dev[lo:hi]
    per_rank = -(-n_work // world)
    local = torch.zeros((per_rank, n_classes), dtype=torch.float32, device=dev)
    # parameters are synced to the native handles once; the loop below is launches only.
    # Micro-batches alternate over `streams` HIP streams (one workspace each) so that the short
    # kernels and the tails of one micro-batch overlap with the convolutions of the next.
    handles = model.eval().lane_handles(max(1, streams))
    main = torch.cuda.current_stream(dev)
    lanes = [main] + [_side_stream(dev, i) for i in range(1, len(handles))]
    for st in lanes[1:]:
        st.wait_stream(main)
    fwd, fwd_name = model.tiles_entry()
    if streamed:
        _forward_streamed(sampler, handles[0], origins[lo:hi], local, n_classes, mb, model)
    if tta is not None:
        _forward_views(tta, fwd, fwd_name, handles, lanes, slide, o_dev, P, mb, local, n_classes)
        if tta_info is not None:
            tta_info.update(views=list(tta.views), n_forward_tiles=(hi - lo) * len(tta))
    for k, s in enumerate(range(0, 0 if streamed or tta is not None else hi - lo, mb)):
        lane = k % len(handles)
        _launch_tiles(fwd, fwd_name, handles[lane], slide, sampler.h, sampler.w, o_dev, s, min(s + mb, hi - lo), P, local,
                      n_classes, lanes[lane])
    for st in lanes[1:]:
        main.wait_stream(st)
    if n_work == 0:   # every rank rejected every tile: nothing to exchange
        logits_work = local[:0]
    elif distributed and timing is not None and local.is_cuda:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(main)
        logits_work = exchange_logits(local, n_work, group)
        ev[1].record(main)
        timing.append(ev)
    else:
        logits_work = exchange_logits(local, n_work, group) if distributed else local[:n_work]
    return _finish(sampler, logits_work, kept, kept_yx_dev, downscale, dedupe_padding, tissue if quality is None else quality,
                   return_logits, return_proba)


def _forward_views(tta, fwd, fwd_name, handles, lanes, slide, o_dev, P, mb, local, n_classes):
    """The launches of predict_full_patched under test-time augmentation: for each view of `tta` in turn the view of `slide` is
    built (into one buffer, reused; "r0" is the slide itself), the fused entry runs over the mapped origins of `o_dev` in the
    plain run's micro-batches on `lanes`, and the view's logits are folded into the first len(o_dev) rows of `local`.
    The micro-batches of a view run on the lane streams and the transform of the next view overwrites the slide they read, so
    the lanes are joined into the main stream (lanes[0]) before each transform and wait for it afterwards; the fold of a view
    runs on the main stream behind the same join.  On return every lane has been joined and `local` holds the mean."""
    main, n = lanes[0], int(o_dev.shape[0])
    h, w = int(slide.shape[0]), int(slide.shape[1])
    buf = per_view = None
    if n == 0:
        return
    for k, v in enumerate(tta.ids):
        for st in lanes[1:]:
            main.wait_stream(st)
        if k > 1:
            tta.fold(local[:n], per_view, k - 1)      # view k - 1 has finished; view 0 went straight into `local`
        if v == 0:
            view = slide
        else:
            buf = torch.empty(slide.numel(), dtype=torch.uint8, device=slide.device) if buf is None else buf
            view = dihedral_view(slide, v, out=buf)
        o_view = map_origins_device(o_dev, h, w, P, v)
        if k and per_view is None:
            per_view = torch.empty((n, n_classes), dtype=torch.float32, device=slide.device)
        for st in lanes[1:]:
            st.wait_stream(main)
        vh, vw = view_shape(h, w, v)
        for j, s in enumerate(range(0, n, mb)):
            lane = j % len(handles)
            _launch_tiles(fwd, fwd_name, handles[lane], view, vh, vw, o_view, s, min(s + mb, n), P, local if k == 0 else per_view,
                          n_classes, lanes[lane])
    for st in lanes[1:]:
        main.wait_stream(st)
    if len(tta) > 1:
        tta.fold(local[:n], per_view, len(tta) - 1)
    tta.finish(local[:n])


def _finish(sampler, logits_work, kept, kept_yx_dev, downscale, dedupe_padding, tissue, return_logits, return_proba):
    """The tail of predict_full_patched: `logits_work` holds one row per tile that ran (`kept`, or every unique tile for None: the
    unfiltered run is the filtered one with every tile kept).  Ordered accumulation over accumulation_list and argmax; with a
    tile filter (`tissue`: the TissueFilter or QualityFilter that names the fill class) the fill of the cells no kept tile covers; the probabilities over the same list (uncovered cells: count 0 and
    the fill class); the logits scattered back to the padded list (NaN rows for rejected tiles)."""
    origins, n_unique, P = sampler.origins, sampler.n_tiles, sampler.patch_size
    h, w, dev = sampler.h, sampler.w, logits_work.device
    rows, yx = accumulation_list(origins, n_unique, kept, dedupe_padding)
    n_dup = len(rows) - len(logits_work)   # the corner's padding duplicates: rows repeats the last row that often
    acc = (torch.cat([logits_work, logits_work[-1:].expand(n_dup, -1)]) if n_dup else logits_work).contiguous()
    if len(rows):
        _, cmap = tiles.accumulate_logits(acc, yx, P, downscale, h, w)
    else:   # all glass: no forward ran, every cell is uncovered
        cmap = torch.zeros((h // downscale, w // downscale), dtype=torch.int64, device=dev)
    if tissue is not None:
        fill_uncovered(cmap, kept_yx_dev, P, downscale, h, w, tissue.fill_class)
    extra = []
    if return_proba:   # the same list right after the class map: the bin plan is reused
        extra.append(tiles.accumulate_probabilities(acc, yx, P, downscale, h, w,
                                                    fill_class=-1 if tissue is None else tissue.fill_class))
    if return_logits:
        whole = kept is None and len(acc) == len(origins)   # the accumulated tensor is the padded list already
        extra.insert(0, acc if whole else _padded_logits(logits_work, kept, n_unique, len(origins)))
    return _pack(cmap, *extra)


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


@_normalised_first
def predict_random_patched(sampler, model, n_classes: int, downscale: int = 16, micro_batch: int | None = None,
                           return_canvas: bool = False, timing: dict | None = None, return_proba: bool = False, *,
                           tta: TestTimeAugmenter | None = None):
    """The reference's default branch (FullImageRndSampler through ImagePredictorPatched.process(),
    predict_full_patched.py:40-63, 150-162) with the random sampler's device index logic and large forward launches.

    The sampler's origin sequence does not depend on the model, so the batches are planned and stepped on a coverage
    stream while `model.forward_tiles` runs over LARGE launches of the accumulated origins on the compute stream (4 096
    tiles in bf16, 1 024 in float32: the dense path's micro-batches) behind an event: planning batch k+1 overlaps the
    forward of earlier tiles, and the per-batch counter read-back never waits behind a forward.  All logits are
    accumulated in sampler order with ONE ordered accumulate at the end.  Large and small launches give identical
    logits, so the class map and canvas are bit-identical to the callback path under the same NumPy seed.
    `timing` (a dict) receives n_batches, n_tiles, host_s (planning + stepping wall time) and wall_s.
    `return_proba=True` appends a tiles.SlideProbabilities built from the same logits and origin
    sequence: under this sampler a cell is covered anything from `dense_level` to dozens of times, and `count` is what makes
    its probabilities comparable from cell to cell.
    Keyword-only `stain=` / `stain_info=`: see `_normalised_first`, which wraps this function.
    Keyword-only `tta`: a tta.TestTimeAugmenter (or what its constructor takes): every launch group runs
    once per view over the device-mapped origins and the logits are averaged per tile in the order of the views; sampler,
    origin sequence and accumulation are those of the plain run.  The groups are launched while the sampler is still
    planning, so all requested views of the slide are built once up front: V - 1 extra resident slides for V views ("r0" is
    the slide itself).  None changes nothing.
    Returns int64[h//d, w//d] on the device (and the float32 canvas when `return_canvas`)."""
    import time

    if not isinstance(model, ResNetHIP):
        raise TypeError("predict_random_patched needs a ResNet18HIP or ResNet50HIP model (use ImagePredictorPatched for other modules)")
    if not sampler.resident:
        raise ValueError("predict_random_patched needs an HBM-resident slide (ONDISK_MULTIPROC: use ImagePredictorPatched)")
    if getattr(sampler, "index_logic", None) != "device":
        raise ValueError("predict_random_patched needs FullImageRndSampler(..., index_logic='device')")
    t0 = time.perf_counter()
    slide = sampler.data_device
    dev, P, B = slide.device, sampler.patch_size, sampler.batch_size
    mb = micro_batch or model.default_micro_batch()
    cap = max(B, mb // B * B)                      # origins per launch group: whole batches
    main = torch.cuda.current_stream(dev)
    cov_stream = _side_stream(dev, "coverage")
    cov_stream.wait_stream(main)                   # the slide / model state queued so far
    model.eval()
    model.lane_handles(1)
    tta = as_augmenter(tta)
    # (view id, that view of the slide): built on the compute stream before the first launch
    views = [] if tta is None else [(v, slide if v == 0 else dihedral_view(slide, v)) for v in tta.ids]
    chunks: list[torch.Tensor] = []                # int32[cap, 2] origin buffers (kept alive to the end)
    logits: list[torch.Tensor] = []
    hosts: list[np.ndarray] = []
    fill = [cap]

    def out(n):
        if fill[0] + n > cap:
            with torch.cuda.stream(cov_stream):    # allocated from the coverage stream's pool, read by the compute stream
                chunks.append(torch.empty((cap, 2), dtype=torch.int32, device=dev))
            chunks[-1].record_stream(main)
            fill[0] = 0
        t = chunks[-1][fill[0]:fill[0] + n]
        fill[0] += n
        return t, t.data_ptr()

    def launch(o):
        ev = torch.cuda.Event()
        ev.record(cov_stream)
        main.wait_event(ev)
        with torch.cuda.stream(main):
            if tta is None:
                for s0 in range(0, o.shape[0], mb):
                    logits.append(model.forward_tiles(slide, o[s0:s0 + mb], P))
                return
            mapped = [map_origins_device(o, sampler.h, sampler.w, P, v) for v, _ in views]
            for s0 in range(0, o.shape[0], mb):
                logits.append(tta.combine(model.forward_tiles(view, m[s0:s0 + mb], P) for (_, view), m in zip(views, mapped)))

    n_batches, host_s = 0, 0.0
    th = time.perf_counter()
    for _, o_host, _filled in sampler._device_origin_batches(host_origins=True, out=out, stream=cov_stream):
        hosts.append(o_host)
        n_batches += 1
        if fill[0] + B > cap:                      # the group is full: hand it to the compute stream
            launch(chunks[-1][:fill[0]])
    if fill[0] and fill[0] + B <= cap and chunks:  # the last, partial group
        launch(chunks[-1][:fill[0]])
    host_s = time.perf_counter() - th
    origins = np.concatenate(hosts) if hosts else np.zeros((0, 2), np.int32)
    with torch.cuda.stream(main):
        lg = torch.cat(logits) if len(logits) > 1 else logits[0]
        canvas, cmap = tiles.accumulate_logits(lg.contiguous(), origins, P, downscale, sampler.h, sampler.w)
        proba = tiles.accumulate_probabilities(lg.contiguous(), origins, P, downscale, sampler.h, sampler.w) if return_proba else None
    if timing is not None:
        torch.cuda.synchronize(dev)
        timing.update(n_batches=n_batches, n_tiles=int(origins.shape[0]), host_s=host_s, wall_s=time.perf_counter() - t0)
    return _pack(cmap, *([canvas] if return_canvas else []) + ([proba] if return_proba else []))


def _forward_streamed(sampler, handle, origins: np.ndarray, local: torch.Tensor, n_classes: int, micro_batch: int, model):
    """Logits of `origins` (this rank's range, reference order) when the slide is not resident: the tiles are
    grouped by tile row; the P-row strip of each group is read from the reader into a pinned buffer, uploaded
    on a side stream (two strip buffers: the disk read and the upload of strip k+1 run under the forward of strip k) and
    serves as the 'slide' of the model's tiles entry; logits land at their
    reference-order positions."""
    dev, P, w = sampler.device, sampler.patch_size, sampler.w
    main = torch.cuda.current_stream(dev)
    copy_stream = torch.cuda.Stream(dev)
    ys = np.unique(origins[:, 0])
    groups = [np.nonzero(origins[:, 0] == y)[0] for y in ys]
    pinned = [torch.empty((P, w, 3), dtype=torch.uint8).pin_memory() for _ in range(2)]
    strip = [torch.empty((P, w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    uploaded = [torch.cuda.Event() for _ in range(2)]
    consumed = [None, None]
    fwd, fwd_name = model.tiles_entry()

    def stage(k):
        b = k & 1
        if consumed[b] is not None:
            consumed[b].synchronize()
        y = int(ys[k])
        np.copyto(pinned[b].numpy(), sampler.read_region(y, 0, y + P, w))
        with torch.cuda.stream(copy_stream):
            strip[b].copy_(pinned[b], non_blocking=True)
            uploaded[b].record(copy_stream)

    if len(ys):
        stage(0)
    for k, idx in enumerate(groups):
        b = k & 1
        main.wait_event(uploaded[b])
        o = np.zeros((len(idx), 2), np.int32)
        o[:, 1] = origins[idx, 1]
        o_dev = torch.from_numpy(o).to(dev)
        out = torch.empty((len(idx), n_classes), dtype=torch.float32, device=dev)
        for s0 in range(0, len(idx), micro_batch):
            _launch_tiles(fwd, fwd_name, handle, strip[b], P, w, o_dev, s0, min(s0 + micro_batch, len(idx)), P, out, n_classes, main)
        local[torch.from_numpy(idx).to(dev)] = out
        consumed[b] = torch.cuda.Event()
        consumed[b].record(main)
        # strip k is queued: NOW read strip k+1 from the reader (the host blocks on the disk while the GPU runs strip k;
        # staging before the launches left the GPU idle during every read)
        if k + 1 < len(ys):
            stage(k + 1)
