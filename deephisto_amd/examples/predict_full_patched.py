"""Whole-slide patched prediction -- drop-in for examples/predict_full_patched.py.

Keeps `ImagePredictorPatched(psim_path, patch_sampler, batch_predictor, anno, layer,
downscale).process()`, `batch_predictor(patches, model, device)` and
`load_model(weights_path, device)` (predict_full_patched.py:22-78, 116-126), and adds
`predict_full_patched(...)`, the device-resident fast path used by bench.py:
tile ranges are sharded over the ranks of a torch.distributed job (RCCL over
xGMI), every rank runs fused gather+ResNet-18 on its range, per-tile logits are
all-gathered, and the ordered accumulation + argmax run once; and
`predict_random_patched(...)`, the same for the random sampler's branch (device
coverage map, large forward launches, one ordered accumulation).  With `return_proba=True` both also return
the per-cell mean softmax probabilities, hit counts, their class map and confidence (`tiles.SlideProbabilities`,
DESIGN.md section 4.8); `ImagePredictorPatched.process_proba()` is the same for the callback route.
`score_prediction(pred, anno, ...)` (deephisto_amd.scoring) scores any of these maps against the
slide's polygon annotation; the CLI does so with `--anno PATH [--score_json PATH]`.
`extract_regions(pred, ...)` (deephisto_amd.regions) lists a map's connected regions, removes the small
ones and traces them into polygons; the CLI does so with `--regions_json`, `--min_region [--clean_rounds]`, `--export_anno`.
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable

import numpy as np
import torch

import ctypes as C
import os

from .. import tiles
from .._lib import DH_LAYOUT_NCHW, check
from ..models.patch_cls_simple.engine import ResNetHIP
from ..models.patch_cls_simple.model import ResNet18HIP, get_model
from ..patch_samplers.full_samplers import DevicePatch, FullImageDenseSampler
from ..psimage_compat import Patch, open_slide
from ..regions import (SlideRegions, clean_map, export_annotation, extract_regions, label_components,  # noqa: F401  (exported here)
                       region_table, save_regions, trace_polygons)
from ..scoring import SlideScore, confusion, rasterize_annotation, save_score, score_prediction  # noqa: F401  (exported here)
from ..tissue import TissueFilter, fill_uncovered, score_tiles


def _n_classes(anno) -> int:
    if hasattr(anno, "anno_classes"):  # AnnoDescription (predict_full_patched.py:43)
        return len(anno.anno_classes)
    return int(anno)


class ImagePredictorPatched:
    def __init__(
        self,
        psim_path,
        patch_sampler,
        batch_predictor: Callable[[list[Patch]], "np.ndarray"],
        anno,
        layer: int,
        downscale: int = 4,
        device="cuda",
    ):
        self.patch_sampler = patch_sampler
        self.batch_predictor = batch_predictor
        self.anno = anno
        self.layer = layer
        self.downscale = downscale
        self.device = torch.device(device)
        self._cached_runs = None
        if isinstance(psim_path, (tuple, list)):  # (h, w) given directly
            self.h, self.w = int(psim_path[0]), int(psim_path[1])
        elif isinstance(psim_path, torch.Tensor):
            self.h, self.w = int(psim_path.shape[0]), int(psim_path.shape[1])
        else:
            with open_slide(psim_path) as psim:
                self.h, self.w = psim.layer_size(self.layer)

    def process(self) -> np.ndarray:
        """int64[h//d, w//d] class map.  Iterates the sampler and the caller's
        batch_predictor like the reference (predict_full_patched.py:47-48); the per-patch
        `prediction[...] += logits` loop and the argmax (:49-62) run on the GPU, in the
        same order (padding duplicates included), once all batches are in."""
        canvas, cmap = None, None
        for ps, origins, logits in self._runs():
            canvas, cmap = tiles.accumulate_logits(logits, origins, ps, self.downscale, self.h, self.w, canvas=canvas)
        if cmap is None:
            return np.zeros((self.h // self.downscale, self.w // self.downscale), dtype=np.int64)
        return cmap.cpu().numpy()

    def process_proba(self, fill_class: int = -1) -> tiles.SlideProbabilities:
        """The callback route of process() with the probability finish: the softmax of every patch's
        logits is summed and counted per cell in the sampler's order, then divided.  Returns a tiles.SlideProbabilities on
        `device` (proba, count, class_map = argmax of the mean probability, confidence); cells no patch covered hold
        `fill_class`.  process() and its argmax of logit sums are unchanged."""
        runs = self._runs() or [(1, np.zeros((0, 2), np.int32),
                                 torch.zeros((0, _n_classes(self.anno)), dtype=torch.float32, device=self.device))]
        state = None
        for k, (ps, origins, logits) in enumerate(runs):
            state = tiles.accumulate_probabilities(logits, origins, ps, self.downscale, self.h, self.w, state=state,
                                                   fill_class=fill_class, finish=k == len(runs) - 1)
        return state

    def _runs(self) -> list[tuple[int, np.ndarray, torch.Tensor]]:
        """Iterates the sampler and the batch_predictor once: (patch_size, int32 origins, float32 device logits) per run of
        patches of one size, in the sampler's order.  Kept, so that process() and process_proba() of one predictor share the
        one pass a sampler's generator allows."""
        if self._cached_runs is not None:
            return self._cached_runs
        n = _n_classes(self.anno)
        runs: list[tuple[int, list, list]] = []  # (patch_size, origins, logits) per run of equal size
        for patches, _progress in self.patch_sampler:
            preds = self.batch_predictor(patches)
            if isinstance(preds, torch.Tensor):
                preds = preds.detach().to(torch.float32)
            else:
                preds = torch.from_numpy(np.asarray(preds, dtype=np.float32))
            if preds.shape[0] != len(patches) or preds.shape[1] != n:
                raise ValueError(f"batch_predictor returned {tuple(preds.shape)} for {len(patches)} patches, {n} classes")
            for i, p in enumerate(patches):
                if not runs or runs[-1][0] != p.patch_size:
                    runs.append((p.patch_size, [], []))
                runs[-1][1].append((p.pos_y, p.pos_x))
                runs[-1][2].append(preds[i:i + 1])
        self._cached_runs = [(ps, np.asarray(origins, dtype=np.int32), torch.cat(logit_rows).to(self.device).contiguous())
                             for ps, origins, logit_rows in runs]
        return self._cached_runs


def batch_predictor(patches: list[Patch], model, device) -> np.ndarray:
    """float32[B, n_cls] raw logits for a list of patches (predict_full_patched.py:66-78).

    Patches cut by this package's samplers are gathered from the HBM-resident slide
    inside the stem kernel (no float copy of the pixels exists anywhere); foreign
    patches carrying host arrays are uploaded as uint8 and gathered the same way."""
    device = torch.device(device)
    ps = patches[0].patch_size
    origins = np.array([(p.pos_y, p.pos_x) for p in patches], dtype=np.int32)
    if all(isinstance(p, DevicePatch) and p._sampler is patches[0]._sampler for p in patches):
        slide = patches[0]._sampler.data_device
    else:  # stack foreign host patches into a strip "slide" of B tiles
        slide = torch.from_numpy(np.concatenate([np.asarray(p.data, dtype=np.uint8) for p in patches], axis=0)).to(device)
        origins = np.array([(i * ps, 0) for i in range(len(patches))], dtype=np.int32)
    o_dev = torch.from_numpy(origins).to(slide.device)
    if isinstance(model, ResNet18HIP):
        out = model.forward_tiles(slide, o_dev, ps)
    else:  # any other nn.Module: build the NCHW float input with the gather kernel
        with torch.no_grad():
            out = model(tiles.gather_tiles(slide, o_dev, ps, DH_LAYOUT_NCHW, torch.float32))
    return out.detach().cpu().numpy()


ARCHS = ("resnet18", "resnet50")


def detect_arch(state_dict) -> str:
    """Backbone of a checkpoint from its keys: a bottleneck's third convolution (`layer1.0.conv3.weight`) means ResNet-50."""
    return "resnet50" if "layer1.0.conv3.weight" in state_dict else "resnet18"


def resolve_arch(arch, state_dict=None) -> str:
    """`arch` None / "auto": read it from `state_dict` (ResNet-18 without one, as the reference); an explicit arch must match the
    checkpoint's keys."""
    if arch not in (None, "auto") and arch not in ARCHS:
        raise ValueError(f"unknown architecture {arch!r} (auto, {', '.join(ARCHS)})")
    found = detect_arch(state_dict) if state_dict is not None else None
    if arch in (None, "auto"):
        return found or "resnet18"
    if found is not None and found != arch:
        raise ValueError(f"--arch {arch} does not match the checkpoint, whose keys are those of a {found} "
                         f"({'has' if found == 'resnet50' else 'lacks'} layer1.0.conv3.weight)")
    return arch


def load_model(weights_path, device, compute_dtype: str = "f32", arch=None) -> torch.nn.Module:
    """predict_full_patched.py:116-126: 5-class model, state_dict loaded weights_only.  `arch` None / "auto" picks the backbone from
    the checkpoint's keys (resolve_arch); ResNet-50 runs in bf16 whatever `compute_dtype` says (as get_model)."""
    sd = torch.load(weights_path, weights_only=True, map_location=device)
    model = get_model(n_classes=5, compute_dtype=compute_dtype, arch=resolve_arch(arch, sd)).to(device)
    model.load_state_dict(sd)
    model.to(device).eval()
    return model


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


def predict_full_patched(sampler: FullImageDenseSampler, model, n_classes: int,
                         downscale: int = 16, micro_batch: int | None = None, group=None,
                         return_logits: bool = False, streams: int = 2, dedupe_padding: bool = False, timing: list | None = None,
                         tissue: TissueFilter | None = None, tissue_info: dict | None = None, return_proba: bool = False):
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
    Returns int64[h//d, w//d] on the device (and the float32[n_padded, n_cls] logits; rows of rejected tiles are NaN).
    """
    import torch.distributed as dist

    streamed = not sampler.resident          # ONDISK_MULTIPROC: row strips are uploaded as they are needed
    if tissue is not None:
        if not isinstance(sampler, FullImageDenseSampler):
            raise ValueError("the tissue filter works on the dense sampler's grid only (not on the random sampler's branch)")
        if streamed:
            raise ValueError("the tissue filter needs an HBM-resident slide (ONDISK_MULTIPROC streams it)")
    slide = None if streamed else sampler.data_device
    dev = sampler.device if streamed else slide.device
    P = sampler.patch_size
    origins = sampler.origins                      # padded, reference order
    n_unique, n_padded = sampler.n_tiles, len(origins)
    kept = None
    if tissue is not None:
        # the launch list becomes the kept tiles, in grid order (integer-exact: the same on every rank)
        kept_idx_dev, kept_yx_dev, info = score_tiles(slide, torch.from_numpy(origins[:n_unique]).to(dev), P, tissue,
                                                      origins[:n_unique])
        kept = kept_idx_dev.cpu().numpy().astype(np.int64)
        if tissue_info is not None:
            tissue_info.update(info, kept=kept)
    n_work = n_unique if kept is None else len(kept)
    # tiles per kernel launch (independent of the sampler's batch size).  bf16: 4 096, the library's maximum (a 64 x 64 x 64-channel
    # map of 4 096 tiles is 2 GiB).  float32: 1 024 -- the same map would be 4 GiB per tensor at 4 096 tiles, past the 32-bit byte
    # offsets of the conv schedule tables (the library refuses it)
    mb = micro_batch or model.default_micro_batch()
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    lo, hi = shard_range(n_work, world, rank)
    if hi - lo > mb:
        # near-equal launches instead of full ones plus a short tail, each a MULTIPLE OF 128 TILES (all but the last): the persistent
        # kernels run one tile per workgroup per iteration on 256 CUs (stem: 768 workgroups), and a layer has 8 / 4 / 2 / 2 conv tiles
        # per 256 x 256 image, so only multiples of 128 images fill the last iteration of every layer.  38 416 tiles as 10 x 3 842 paid
        # an almost empty extra iteration in every layer of every launch (121 instead of 120.06 in layer 1, 31 instead of 30.02 in
        # layers 3-4, 26 instead of 25.01 in the stem: ~2 % of the slide); 9 x 3 968 + 2 704 does not.
        k = -(-(hi - lo) // mb)
        per = -(-(hi - lo) // k)
        mb = min(mb, max(128, -(-per // 128) * 128)) if mb >= 128 else per
        if os.environ.get("DH_MB_ALIGN") == "0":   # A/B: the round-3 rule (equal launches, any size)
            mb = per
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
    for k, s in enumerate(range(0, 0 if streamed else hi - lo, mb)):
        e = min(s + mb, hi - lo)
        lane = k % len(handles)
        check(fwd(handles[lane], slide.data_ptr(), sampler.h, sampler.w, o_dev.data_ptr() + 8 * s, e - s, P,
                  local.data_ptr() + 4 * n_classes * s, C.c_void_p(lanes[lane].cuda_stream)),
              fwd_name)
    for st in lanes[1:]:
        main.wait_stream(st)
    if n_work == 0:   # every rank rejected every tile: nothing to exchange
        logits_unique = local[:0]
    elif distributed and timing is not None and local.is_cuda:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(main)
        logits_unique = exchange_logits(local, n_work, group)
        ev[1].record(main)
        timing.append(ev)
    else:
        logits_unique = exchange_logits(local, n_work, group) if distributed else local[:n_work]
    pad = n_padded - n_unique
    if kept is not None:
        return _finish_masked(sampler, logits_unique, kept, kept_yx_dev, n_classes, downscale, dedupe_padding, tissue,
                              return_logits, return_proba)
    logits = torch.cat([logits_unique, logits_unique[-1:].expand(pad, -1)]) if pad else logits_unique
    acc, yx = (logits_unique.contiguous(), origins[:n_unique]) if dedupe_padding else (logits.contiguous(), origins)
    _, cmap = tiles.accumulate_logits(acc, yx, P, downscale, sampler.h, sampler.w)
    out = (cmap, logits) if return_logits else (cmap,)
    if return_proba:   # the same list right after the class map: the bin plan is reused
        out += (tiles.accumulate_probabilities(acc, yx, P, downscale, sampler.h, sampler.w),)
    return out if len(out) > 1 else cmap


def _finish_masked(sampler, logits_kept, kept, kept_yx_dev, n_classes, downscale, dedupe_padding, tissue, return_logits,
                   return_proba=False):
    """The tissue-filtered tail of predict_full_patched: ordered accumulation over the kept tiles (plus the corner's padding
    duplicates when the corner is kept), argmax, fill of the uncovered cells; logits scattered back to the padded list.
    The probabilities run over the same kept list; cells it does not cover have count 0 and the fill class."""
    origins, n_unique, P = sampler.origins, sampler.n_tiles, sampler.patch_size
    h, w, dev = sampler.h, sampler.w, logits_kept.device
    pad = len(origins) - n_unique
    k = len(kept)
    acc, yx = logits_kept[:0].reshape(0, n_classes), origins[:0]
    if k == 0:   # all glass: no forward ran, every cell is uncovered
        cmap = torch.zeros((h // downscale, w // downscale), dtype=torch.int64, device=dev)
    else:
        acc, yx = logits_kept, origins[:n_unique][kept]
        if pad and not dedupe_padding and kept[-1] == n_unique - 1:   # the corner is the last unique tile
            acc = torch.cat([acc, acc[-1:].expand(pad, -1)])
            yx = np.concatenate([yx, origins[n_unique:]])
        _, cmap = tiles.accumulate_logits(acc.contiguous(), yx, P, downscale, h, w)
    fill_uncovered(cmap, kept_yx_dev, P, downscale, h, w, tissue.fill_class)
    proba = ((tiles.accumulate_probabilities(acc.contiguous(), yx, P, downscale, h, w, fill_class=tissue.fill_class),)
             if return_proba else ())
    if not return_logits:
        return (cmap, *proba) if proba else cmap
    logits = torch.full((len(origins), n_classes), float("nan"), dtype=torch.float32, device=dev)
    if k:
        logits[torch.from_numpy(kept).to(dev)] = logits_kept
    if pad:
        logits[n_unique:] = logits[n_unique - 1]
    return (cmap, logits, *proba)


def predict_random_patched(sampler, model, n_classes: int, downscale: int = 16, micro_batch: int | None = None,
                           return_canvas: bool = False, timing: dict | None = None, return_proba: bool = False):
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
            for s0 in range(0, o.shape[0], mb):
                logits.append(model.forward_tiles(slide, o[s0:s0 + mb], P))

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
    out = (cmap, canvas) if return_canvas else (cmap,)
    if return_proba:
        out += (proba,)
    return out if len(out) > 1 else cmap


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
            e0 = min(s0 + micro_batch, len(idx))
            check(fwd(handle, strip[b].data_ptr(), P, w, o_dev.data_ptr() + 8 * s0, e0 - s0, P,
                      out.data_ptr() + 4 * n_classes * s0, C.c_void_p(main.cuda_stream)), fwd_name)
        local[torch.from_numpy(idx).to(dev)] = out
        consumed[b] = torch.cuda.Event()
        consumed[b].record(main)
        # strip k is queued: NOW read strip k+1 from the reader (the host blocks on the disk while the GPU runs strip k;
        # staging before the launches left the GPU idle during every read)
        if k + 1 < len(ys):
            stage(k + 1)


def perform_and_save_visualizations(img, anno_dsc, pred, out_dir: Path = Path("."), stem: str | None = None,
                                    alpha: float = 0.6, save: bool = True, device="cuda", proba=None, heat_classes=(),
                                    truth=None, outcome=None):
    """Colourised class mask, the slide at the map's resolution and their overlay -- predict_full_patched.py:81-113.

    `img`: path (psimage, when installed: `get_region(..., target_hw)` as the reference) or a uint8[H,W,3]
    array / GPU tensor, which is sampled at the map's resolution by nearest source pixel (psimage's own
    resampler is third-party and unknown here).  The colour lookup and the float64 blend run on the GPU
    (`dh_colorize_map`, `dh_overlay_blend`) and are bit-identical to the reference's NumPy lines.
    `proba`: the run's tiles.SlideProbabilities; with `save`, `{stem}_confidence.jpg` (the confidence in white over the slide)
    and one `{stem}_heat_{label}.jpg` per label of `heat_classes` (that class's mean probability in the class colour) are
    written as well (`dh_heatmap_blend`, float64 like the overlay).
    `truth` / `outcome`: the label map and the outcome map of a scored run (`scoring.score_prediction(..., return_maps=True)`);
    with `save`, `{stem}_truth.jpg` (the labels in the class colours, unlabelled cells black) and `{stem}_errors.jpg` (correct
    cells green, wrong cells red, blended over the slide with `alpha` like the overlay; unlabelled cells black) are written.
    Returns (mask, image, overlay) as uint8[h, w, 3] NumPy arrays; JPEGs are written when `save`."""
    dev = torch.device(device)
    by_label = {a.label: a for a in anno_dsc.anno_classes}
    unknown = [lb for lb in heat_classes if lb not in by_label]
    if unknown or (heat_classes and proba is None):
        raise ValueError(f"heat_classes {list(heat_classes)}: needs proba and labels out of {', '.join(by_label)}")
    pred_t = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred))
    pred_t = pred_t.to(dev, torch.int64).contiguous()
    h, w = int(pred_t.shape[0]), int(pred_t.shape[1])
    n_ids = max((a.id for a in anno_dsc.anno_classes), default=-1) + 1
    lut = torch.zeros((n_ids, 3), dtype=torch.uint8)
    for a in anno_dsc.anno_classes:
        lut[a.id] = torch.tensor(a.color, dtype=torch.uint8)
    colored = tiles.colorize_map(pred_t, lut)
    if isinstance(img, (str, Path)):
        stem = stem or Path(img).stem
        with open_slide(img) as psim:
            small = torch.from_numpy(np.ascontiguousarray(psim.get_region((0, 0), (psim.height, psim.width), target_hw=(h, w)))).to(dev)
    else:
        full = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
        full = full.to(dev)
        ys = (torch.arange(h, device=dev) * full.shape[0]) // h
        xs = (torch.arange(w, device=dev) * full.shape[1]) // w
        small = full[ys][:, xs].contiguous()
    overlay = tiles.overlay_blend(small, colored, alpha)
    mask_np, img_np, ov_np = colored.cpu().numpy(), small.cpu().numpy(), overlay.cpu().numpy()
    if save:
        from PIL import Image
        out_dir = Path(out_dir)
        out_dir.mkdir(exist_ok=True, parents=True)
        stem = stem or "slide"
        Image.fromarray(mask_np).save(out_dir / f"{stem}_mask.jpg", quality=95)
        Image.fromarray(img_np).save(out_dir / f"{stem}.jpg", quality=95)
        Image.fromarray(ov_np).save(out_dir / f"{stem}_overlay.jpg", quality=95)
        if proba is not None:
            heat = tiles.heatmap_blend(small, proba.confidence.to(dev), (255, 255, 255), alpha)
            Image.fromarray(heat.cpu().numpy()).save(out_dir / f"{stem}_confidence.jpg", quality=95)
            for lb in heat_classes:
                heat = tiles.heatmap_blend(small, proba.proba.to(dev)[..., by_label[lb].id], by_label[lb].color, alpha)
                Image.fromarray(heat.cpu().numpy()).save(out_dir / f"{stem}_heat_{lb}.jpg", quality=95)
        if truth is not None:
            truth_rgb = tiles.colorize_map(truth.to(dev, torch.int64).contiguous(), lut)
            Image.fromarray(truth_rgb.cpu().numpy()).save(out_dir / f"{stem}_truth.jpg", quality=95)
        if outcome is not None:
            two = torch.tensor([ERROR_COLORS["correct"], ERROR_COLORS["wrong"]], dtype=torch.uint8)
            errors = tiles.overlay_blend(small, tiles.colorize_map(outcome.to(dev, torch.int64).contiguous(), two), alpha)
            Image.fromarray(errors.cpu().numpy()).save(out_dir / f"{stem}_errors.jpg", quality=95)
    return mask_np, img_np, ov_np


KNOWN_COLORS = {   # predict_full_patched.py:139-148
    "AT": (245, 119, 34),    # orange
    "BG": (153, 255, 255),   # cyan
    "LP": (64, 170, 72),     # green
    "MM": (255, 0, 0),       # red
    "TUM": (33, 67, 156),    # blue
}


ERROR_COLORS = {"correct": (0, 255, 0), "wrong": (255, 0, 0)}   # the 2-row LUT of the outcome map (0, 1)


def _anno_from_args(ap, args):
    """The records of --anno (None without it); a missing file, an annotation without a region of a known class and
    --score_json without --anno are argparse errors."""
    import json

    if args.score_json and not args.anno:
        ap.error("--score_json needs --anno")
    if not args.anno:
        return None
    if not Path(args.anno).is_file():
        ap.error(f"--anno {args.anno}: no such file")
    try:
        records = json.loads(Path(args.anno).read_text())
        known = [a for a in records if a["class"] in KNOWN_COLORS]
    except (ValueError, TypeError, KeyError) as e:
        ap.error(f"--anno {args.anno}: not a JSON list of {{class, vertices}} records ({e!r})")
    if not known:
        ap.error(f"--anno {args.anno}: none of its {len(records)} regions belongs to a known class ({', '.join(KNOWN_COLORS)})")
    return records


def _tissue_from_args(ap, args) -> TissueFilter | None:
    """The TissueFilter of the --tissue flags, or None for `--tissue off`; a bad combination is an argparse error."""
    from ..anno.utils import AnnoDescription

    if args.tissue == "off":
        return None
    if args.random_sampler:
        ap.error("--tissue works on the dense sampler's grid; it cannot be combined with --random_sampler")
    if args.ondisk:
        ap.error("--tissue needs the slide resident in HBM; it cannot be combined with --ondisk")
    labels = {a.label: a.id for a in AnnoDescription.with_known_colors(KNOWN_COLORS).anno_classes}
    if args.tissue_fill in labels:
        fill = labels[args.tissue_fill]
    elif args.tissue_fill == "-1":
        fill = -1
    else:
        ap.error(f"--tissue_fill must be one of {', '.join(labels)} or -1, not {args.tissue_fill!r}")
    try:
        threshold = "otsu" if args.tissue == "otsu" else int(args.tissue)
    except ValueError:
        ap.error(f"--tissue must be off, otsu or an integer threshold in [0, 255], not {args.tissue!r}")
    try:
        return TissueFilter(threshold, args.tissue_min_fraction, fill)
    except ValueError as e:
        ap.error(f"--tissue {args.tissue} / --tissue_min_fraction {args.tissue_min_fraction}: {e}")


def _proba_from_args(ap, args) -> None:
    """Checks the --proba flags; a bad combination or an unknown class label is an argparse error."""
    if args.heat and not args.proba:
        ap.error("--heat needs --proba")
    if args.save_proba and not args.proba:
        ap.error("--save_proba needs --proba")
    for lb in args.heat:
        if lb not in KNOWN_COLORS:
            ap.error(f"--heat labels must be out of {', '.join(KNOWN_COLORS)}, not {lb!r}")


def _regions_from_args(ap, args) -> None:
    """Checks the region flags; a bad combination is an argparse error."""
    if args.clean_rounds is not None and args.min_region is None:
        ap.error("--clean_rounds needs --min_region")
    if args.min_region is not None and args.min_region < 1:
        ap.error(f"--min_region must be >= 1, not {args.min_region}")
    if args.clean_rounds is not None and args.clean_rounds < 1:
        ap.error(f"--clean_rounds must be >= 1, not {args.clean_rounds}")


def save_proba(path, proba) -> tuple[Path, Path]:
    """Writes `proba.proba` as float16 to `path` (.npy) and `proba.count` to the same name with `_count` before the suffix."""
    path = Path(path)
    if path.suffix != ".npy":
        path = path.with_name(path.name + ".npy")
    path.parent.mkdir(exist_ok=True, parents=True)
    count_path = path.with_name(path.stem + "_count.npy")
    np.save(path, proba.proba.cpu().numpy().astype(np.float16))
    np.save(count_path, proba.count.cpu().numpy())
    return path, count_path


def main(argv=None, model=None):
    """The reference's `__main__` (predict_full_patched.py:128-177) as a per-rank program.

    The reference hard-codes the slide path, `./output/best_model.pth`, layer 2, downscale 16, patch 224, batch 64 and
    (dense branch, :165-167) stride 112; those are the defaults of the flags below.  The dense branch is the multi-GPU
    path: under `python -m torch.distributed.run --nproc-per-node N -m examples.predict_full_patched ...` every rank
    binds its GPU, joins the RCCL group, takes its contiguous tile range and the logits are exchanged with one
    all-gather (`predict_full_patched`); rank 0 writes the three JPEGs.  `--random_sampler` runs the reference's
    default branch (`FullImageRndSampler`, single process): `predict_random_patched` for a resident slide and a ResNet18HIP
    or ResNet50HIP model, `ImagePredictorPatched.process()` with the per-batch callback for an injected foreign model or `--ondisk`.
    `--synthetic H W` runs on a closed-form slide when no .psi file / psimage is at hand; `--weights ''` = random init.
    `--arch auto` reads the backbone from the checkpoint (ResNet-50 when it has `layer1.0.conv3.weight`).
    `--tissue otsu|<0..255>` classifies only the tiles that hold tissue (dense branch, resident slide; TissueFilter), with
    `--tissue_min_fraction` and `--tissue_fill` (a class label, or -1 for no class) for the cells no kept tile covers.
    `--proba` also computes the per-cell mean softmax probabilities and writes the confidence JPEG;
    `--heat LABEL ...` adds one heat map per class label; `--save_proba PATH` writes the probabilities as float16 PATH(.npy) and
    the hit counts as PATH_count.npy (rank 0).  The returned class map stays the argmax of the logit sums.
    `--anno PATH` scores the class map against the slide's polygon annotation (rank 0): prints the table
    and writes `{stem}_truth.jpg` and `{stem}_errors.jpg`; `--score_json PATH` writes the figures and the annotation's counts.
    `--regions_json PATH` writes the table of the map's connected regions (rank 0); `--min_region CELLS
    [--clean_rounds R]` first gives regions below CELLS cells the class of their large neighbours and writes
    `{stem}_clean_mask.jpg` and `{stem}_clean_overlay.jpg`; `--export_anno PATH` writes the regions as polygons in the
    annotation's JSON format.  The returned map and the three standard JPEGs are those of a run without these flags, and
    `--anno` keeps scoring the uncleaned map (the cleaned one gets a second score).
    `model`: an injected module (tests)."""
    import argparse

    from ..anno.utils import AnnoDescription
    from ..distributed import finalize, init_from_env
    from ..models.patch_cls_simple import utils
    from ..patch_samplers.full_samplers import FullImageRndSampler, SamplerExecutionMode

    ap = argparse.ArgumentParser(description=main.__doc__.splitlines()[0])
    ap.add_argument("--image", default="/home/xubiker/dev/PATH-DT-MSU.WSS2/images/test/test_01.psi")
    ap.add_argument("--synthetic", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--weights", default="./output/best_model.pth")
    ap.add_argument("--layer", type=int, default=2)
    ap.add_argument("--downscale_vis", type=int, default=16)
    ap.add_argument("--patch_size", type=int, default=224)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--stride", type=int, default=112)
    ap.add_argument("--random_sampler", action="store_true", default=False)
    ap.add_argument("--ondisk", action="store_true", help="SamplerExecutionMode.ONDISK_MULTIPROC: stream row strips")
    ap.add_argument("--compute_dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--arch", choices=["auto", *ARCHS], default="auto",
                    help="backbone; auto: from the checkpoint's keys (ResNet-18 with --weights ''); ResNet-50 is bf16")
    ap.add_argument("--out_dir", default="./output/")
    ap.add_argument("--no_visualizations", action="store_true")
    ap.add_argument("--tissue", default="off", metavar="{off,otsu,<int>}",
                    help="classify only tiles with tissue: chroma threshold 'otsu' or 0..255 (dense branch only)")
    ap.add_argument("--tissue_min_fraction", type=float, default=0.25,
                    help="share of a tile's pixels that must be tissue (0.25: a conventional default, not validated here)")
    ap.add_argument("--tissue_fill", default="-1", help="class label for cells no kept tile covers, or -1 (no class)")
    ap.add_argument("--proba", action="store_true", help="per-cell mean softmax probabilities; writes {stem}_confidence.jpg")
    ap.add_argument("--heat", nargs="+", default=[], metavar="LABEL",
                    help=f"with --proba: one {{stem}}_heat_LABEL.jpg per class label ({', '.join(KNOWN_COLORS)})")
    ap.add_argument("--save_proba", default=None, metavar="PATH",
                    help="with --proba: probabilities as float16 PATH(.npy), hit counts as PATH_count.npy (rank 0)")
    ap.add_argument("--anno", default=None, metavar="PATH",
                    help="the slide's annotation JSON: score the class map against it; writes {stem}_truth.jpg, {stem}_errors.jpg")
    ap.add_argument("--score_json", default=None, metavar="PATH", help="with --anno: the score and the annotation's counts as JSON")
    ap.add_argument("--regions_json", default=None, metavar="PATH", help="the table of the map's connected regions as JSON (rank 0)")
    ap.add_argument("--min_region", type=int, default=None, metavar="CELLS",
                    help="regions below CELLS cells take their large neighbours' class; writes {stem}_clean_mask.jpg, {stem}_clean_overlay.jpg")
    ap.add_argument("--clean_rounds", type=int, default=None, metavar="R", help="with --min_region: cleanup rounds (default 1)")
    ap.add_argument("--export_anno", default=None, metavar="PATH", help="the regions as polygons in the annotation's JSON format (rank 0)")
    args = ap.parse_args(argv)
    _regions_from_args(ap, args)
    tissue = _tissue_from_args(ap, args)
    anno_records = _anno_from_args(ap, args)
    _proba_from_args(ap, args)

    rank, world, _dev_index, owned = init_from_env()   # binds the rank's GPU before any other GPU call
    ok = False
    try:
        import torch.distributed as dist
        device = utils.get_device()
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if model is None:
            if device.type != "cuda":
                raise RuntimeError("predict_full_patched runs on the GPU only (HIP kernels); no CPU fallback")
            if args.weights:
                model = load_model(args.weights, device, args.compute_dtype, arch=args.arch)
            else:
                torch.manual_seed(0)   # the same random init on every rank
                model = get_model(n_classes=5, compute_dtype=args.compute_dtype, arch=resolve_arch(args.arch)).to(device).eval()
        anno_dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
        n_cls = len(anno_dsc.anno_classes)
        if args.synthetic is not None:
            img = tiles.synth_slide(args.synthetic[0], args.synthetic[1], 0, device)
            stem = f"synthetic_{args.synthetic[0]}x{args.synthetic[1]}"
        else:
            img, stem = Path(args.image), Path(args.image).stem
        mode = SamplerExecutionMode.ONDISK_MULTIPROC if args.ondisk else SamplerExecutionMode.INMEMORY_SINGLEPROC
        if args.random_sampler:
            if world > 1:
                raise RuntimeError("--random_sampler draws tiles from a running coverage map (one process); "
                                   "the dense sampler is the multi-GPU path")
            smp = FullImageRndSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                      mode=mode, device=device)
            proba = None
            if smp.resident and smp.index_logic == "device" and isinstance(model, ResNetHIP):
                pred = predict_random_patched(smp, model, n_cls, downscale=args.downscale_vis, return_proba=args.proba)
                if args.proba:
                    pred, proba = pred
                pred = pred.cpu().numpy()
            else:   # a foreign module or a slide streamed from disk: the reference's callback loop
                predictor = ImagePredictorPatched((smp.h, smp.w), patch_sampler=smp.generator(),
                                                  batch_predictor=lambda patches: batch_predictor(patches, model, device),
                                                  anno=anno_dsc, layer=args.layer, downscale=args.downscale_vis, device=device)
                pred = predictor.process()
                if args.proba:
                    proba = predictor.process_proba()
        else:
            smp = FullImageDenseSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                        mode=mode, stride=args.stride, device=device)
            info: dict = {}
            pred = predict_full_patched(smp, model, n_cls, downscale=args.downscale_vis,   # sharded when world > 1
                                        tissue=tissue, tissue_info=info, return_proba=args.proba)
            proba = None
            if args.proba:
                pred, proba = pred
            if tissue is not None and rank == 0:
                print(f"kept {info['n_kept']} of {info['n_tiles']} tiles, threshold {info['threshold']}", flush=True)
        truth = outcome = None
        if rank == 0 and anno_records is not None:   # the map is whole on rank 0
            score, truth, outcome, anno_info = score_prediction(pred, anno_records, anno_dsc, args.layer, smp.h, smp.w,
                                                                args.downscale_vis, return_maps=True, device=device)
            print(score, flush=True)
            print(f"annotation: {anno_info['n_rings']} rings of {anno_info['n_regions']} regions, "
                  f"{anno_info['skipped_class']} of unknown class, {anno_info['failed']} failed to parse", flush=True)
            if args.score_json:
                save_score(args.score_json, score, anno_info)
        if rank == 0 and not args.no_visualizations:
            src = img if isinstance(img, torch.Tensor) or not smp.resident else smp.data_device
            perform_and_save_visualizations(src, anno_dsc, pred, out_dir=Path(args.out_dir), stem=stem, device=device,
                                            proba=proba, heat_classes=args.heat, truth=truth, outcome=outcome)
        if rank == 0 and args.save_proba:
            save_proba(args.save_proba, proba)
        if rank == 0 and (args.regions_json or args.min_region is not None or args.export_anno):   # the map is whole on rank 0
            from PIL import Image
            res = extract_regions(pred, anno_dsc, args.layer, args.downscale_vis, min_cells=args.min_region or 0,
                                  rounds=args.clean_rounds or 1, polygons=bool(args.export_anno), device=device,
                                  confidence=proba.confidence if proba is not None else None)
            print(f"regions: {res.k}" + (f", cleanup below {args.min_region} cells changed {res.n_changed} cells" if args.min_region else "")
                  + (f", traced in {res.trace_s:.3f} s" if args.export_anno else ""), flush=True)
            if args.regions_json:
                save_regions(args.regions_json, res.regions, anno_dsc, args.downscale_vis, args.layer,
                             dict(min_region=args.min_region, clean_rounds=args.clean_rounds, n_changed=res.n_changed))
            if args.export_anno:
                export_annotation(args.export_anno, res.regions, res.polygons, anno_dsc)
            if args.min_region is not None and anno_records is not None:
                print("cleaned map:", flush=True)
                print(score_prediction(res.class_map, anno_records, anno_dsc, args.layer, smp.h, smp.w, args.downscale_vis,
                                       device=device), flush=True)
            if args.min_region is not None and not args.no_visualizations:
                src_img = img if isinstance(img, torch.Tensor) or not smp.resident else smp.data_device
                mask, _, overlay = perform_and_save_visualizations(src_img, anno_dsc, res.class_map, stem=stem, save=False, device=device)
                Path(args.out_dir).mkdir(exist_ok=True, parents=True)
                Image.fromarray(mask).save(Path(args.out_dir) / f"{stem}_clean_mask.jpg", quality=95)
                Image.fromarray(overlay).save(Path(args.out_dir) / f"{stem}_clean_overlay.jpg", quality=95)
        if world > 1:
            dist.barrier()
        ok = True
        return pred
    finally:
        finalize(owned, ok)   # a failing rank leaves without a barrier (distributed.finalize)


if __name__ == "__main__":
    main()
