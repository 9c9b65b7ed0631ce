"""The device engine of whole-slide prediction (re-exported by examples/predict_full_patched.py, where the CLI lives).

`predict_full_patched(...)` is the device-resident fast path used by bench.py, over the tile plan of `plan.py`: tile ranges are
sharded over the ranks of a torch.distributed job (RCCL over xGMI), every rank runs fused gather+ResNet on its range
(`launch_tiles`, in launches of `launch_size`), per-tile logits are all-gathered (`exchange_logits`), and the ordered accumulation
+ argmax run once over `accumulation_list` (`finish`).  `predict_random_patched(...)` is the same for the random sampler's branch
(device coverage map, large forward launches, one ordered accumulation).  With `return_proba=True` both also return the per-cell
mean softmax probabilities, hit counts, their class map and confidence (`tiles.SlideProbabilities`).
"""
from __future__ import annotations

import numpy as np
import torch

from . import tiles
from .models.patch_cls_simple.engine import ResNetHIP
from .patch_samplers.full_samplers import FullImageDenseSampler
from .plan import (_SIDE_STREAMS, Lanes, _side_stream, accumulation_list, exchange_logits, exchange_rows, finish,  # noqa: F401  (exported here)
                   launch_size, launch_tiles, normalised_first, pack, plan_tiles, shard_range)
from .quality import QualityFilter
from .tissue import TissueFilter
from .tta import TestTimeAugmenter, as_augmenter, dihedral_view, map_origins_device, view_shape


@normalised_first
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
    Keyword-only `stain=` / `stain_info=`: see `plan.normalised_first`, which wraps this function.
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
    streamed = not sampler.resident          # ONDISK_MULTIPROC: row strips are uploaded as they are needed
    tta = as_augmenter(tta)
    if tta is not None and streamed:
        raise ValueError("test-time augmentation needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
    plan = plan_tiles(sampler, model, micro_batch, group, tissue, tissue_info, quality, quality_info)
    slide = None if streamed else sampler.data_device
    n, P, o_dev = plan.hi - plan.lo, sampler.patch_size, plan.o_dev
    local = torch.zeros((plan.per_rank, n_classes), dtype=torch.float32, device=o_dev.device)
    lanes = Lanes(model, streams, o_dev.device)
    entry = model.tiles_entry()
    if streamed:
        _forward_streamed(sampler, lanes.handles[0], sampler.origins[plan.lo:plan.hi], local, n_classes, plan.mb, model)
    elif tta is not None:
        _forward_views(tta, entry, lanes, slide, o_dev, P, plan.mb, local, n_classes)
        if tta_info is not None:
            tta_info.update(views=list(tta.views), n_forward_tiles=n * len(tta))
    else:
        lanes.run(n, plan.mb, lambda handle, stream, s, e: launch_tiles(entry, handle, slide, sampler.h, sampler.w, o_dev, s, e, P,
                                                                        local, stream))
    logits_work = exchange_rows(plan, local, group, timing)
    return finish(plan.grid, logits_work, plan.kept, plan.kept_yx_dev, downscale, dedupe_padding, plan.fill_class, return_logits,
                  return_proba)


def _forward_views(tta, entry, lanes, slide, o_dev, P, mb, local, n_classes):
    """The launches of predict_full_patched under test-time augmentation: for each view of `tta` in turn the view of `slide` is
    built (into one buffer, reused; "r0" is the slide itself), the fused entry runs over the mapped origins of `o_dev` in the
    plain run's micro-batches on `lanes`, and the view's logits are folded into the first len(o_dev) rows of `local`.
    The micro-batches of a view run on the lane streams and the transform of the next view overwrites the slide they read, so
    `lanes.run` joins them into the main stream behind each view and lets them wait for it before the next; the fold of a view
    runs on the main stream behind the same join.  On return every lane has been joined and `local` holds the mean."""
    n = int(o_dev.shape[0])
    h, w = int(slide.shape[0]), int(slide.shape[1])
    buf = per_view = None
    if n == 0:
        return
    for k, v in enumerate(tta.ids):
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
        vh, vw = view_shape(h, w, v)
        out = local if k == 0 else per_view
        lanes.run(n, mb, lambda handle, stream, s, e: launch_tiles(entry, handle, view, vh, vw, o_view, s, e, P, out, stream))
    if len(tta) > 1:
        tta.fold(local[:n], per_view, len(tta) - 1)
    tta.finish(local[:n])


@normalised_first
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
    Keyword-only `stain=` / `stain_info=`: see `plan.normalised_first`, which wraps this function.
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
    return pack(cmap, *([canvas] if return_canvas else []) + ([proba] if return_proba else []))


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
    entry = model.tiles_entry()

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
            launch_tiles(entry, handle, strip[b], P, w, o_dev, s0, min(s0 + micro_batch, len(idx)), P, out, main)
        local[torch.from_numpy(idx).to(dev)] = out
        consumed[b] = torch.cuda.Event()
        consumed[b].record(main)
        # strip k is queued: NOW read strip k+1 from the reader (the host blocks on the disk while the GPU runs strip k;
        # staging before the launches left the GPU idle during every read)
        if k + 1 < len(ys):
            stage(k + 1)
