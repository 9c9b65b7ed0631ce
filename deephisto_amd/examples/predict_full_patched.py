"""Whole-slide patched prediction -- drop-in for examples/predict_full_patched.py.

Keeps `ImagePredictorPatched(psim_path, patch_sampler, batch_predictor, anno, layer,
downscale).process()`, `batch_predictor(patches, model, device)`, `load_model(weights_path, device)` and the `__main__`
(predict_full_patched.py:22-78, 116-177), and re-exports the device engine (deephisto_amd.predict: `predict_full_patched(...)`,
the fast path used by bench.py, and `predict_random_patched(...)`; `ImagePredictorPatched.process_proba()` is their
`return_proba=True` for the callback route) and the visualiser (deephisto_amd.visualize: `perform_and_save_visualizations`,
`KNOWN_COLORS`, `save_proba`).
The scoring, region, embedding, clustering, PCA, neighbour and distance APIs (deephisto_amd.scoring, .regions, .embeddings,
.clustering, .pca, .neighbours, .distance; DESIGN.md sections 4.9 - 4.22) are re-exported too.  The command line lives in
deephisto_amd.cli, one module per flag group, each with its flags, its checks, what rank 0 reports and the group's description;
`_run` and `main` stay here.
`main` calls `predict_full_patched` and `predict_random_patched` through this module's globals (tests replace them here).
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable

import numpy as np
import torch

from .. import cli, tiles
from .._lib import DH_LAYOUT_NCHW, check  # noqa: F401  (exported here)
from ..anno.utils import AnnoDescription
from ..cli import check_args as _check_args, report_rank0 as _report_rank0  # noqa: F401  (exported here, as every name below)
from ..cli.common import Run, dense_resident_only as _dense_resident_only, embedding_flags, fill_class as _fill_class  # noqa: F401
from ..cli.distance import check as _distance_from_args  # noqa: F401
from ..cli.embed import check as _embeddings_from_args, knn_from_args as _knn_from_args  # noqa: F401
from ..cli.filters import quality_from_args as _quality_from_args, tissue_from_args as _tissue_from_args  # noqa: F401
from ..cli.regions import check as _regions_from_args  # noqa: F401
from ..cli.routes import fine_from_args as _fine_from_args, proba_from_args as _proba_from_args, tta_from_args as _tta_from_args  # noqa: F401
from ..cli.scoring import anno_from_args as _anno_from_args  # noqa: F401
from ..cli.slide import pyramid_from_args as _pyramid_from_args, stain_from_args as _stain_from_args  # noqa: F401
from ..clustering import INITS as CLUSTER_INITS, KMeans, cluster_description, cluster_map, cluster_palette  # noqa: F401  (exported here)
from ..distance import (SurfaceDistance, band_composition, check_edges, class_mask, close, dilate, distance_transform, erode,  # noqa: F401  (exported here)
                        margin_bands, open_, save_distance_report, signed_distance, surface_distances, tolerant_score)
from ..cam import predict_fine_patched  # noqa: F401  (exported here)
from ..embeddings import PrototypeClassifier, SlideEmbeddings, extract_embeddings, tile_labels  # noqa: F401  (exported here)
from ..neighbours import KNNClassifier, cap_per_class, nearest_rows, similar_tiles  # noqa: F401  (exported here)
from ..models.patch_cls_simple.engine import ResNetHIP
from ..models.patch_cls_simple.model import ARCHS, ResNet18HIP, detect_arch, get_model, resolve_arch  # noqa: F401  (exported here)
from ..patch_samplers.full_samplers import DevicePatch, FullImageDenseSampler
from ..pca import PCA  # noqa: F401  (exported here)
from ..predict import (_SIDE_STREAMS, _forward_streamed, _side_stream, exchange_logits, predict_full_patched,  # noqa: F401  (exported here)
                       predict_random_patched, shard_range)
from ..psimage_compat import Patch, open_slide
from ..quality import QualityFilter, score_quality, sharpness, sharpness_summary  # noqa: F401  (exported here)
from ..regions import (SlideRegions, clean_map, export_annotation, extract_regions, label_components,  # noqa: F401  (exported here)
                       region_table, save_regions, trace_polygons)
from ..scoring import SlideScore, confusion, rasterize_annotation, save_score, score_prediction  # noqa: F401  (exported here)
from ..stain import StainFit, StainNormalizer  # noqa: F401  (exported here)
from ..tissue import TissueFilter, fill_uncovered, score_tiles  # noqa: F401  (exported here)
from ..tta import TestTimeAugmenter, dihedral_view  # noqa: F401  (exported here)
from ..visualize import ERROR_COLORS, KNOWN_COLORS, _save_jpeg, perform_and_save_visualizations, save_proba  # noqa: F401  (exported here)


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


def load_model(weights_path, device, compute_dtype: str = "f32", arch=None) -> torch.nn.Module:
    """predict_full_patched.py:116-126: 5-class model, state_dict loaded weights_only.  `arch` None / "auto" picks the backbone from
    the checkpoint's keys (resolve_arch); ResNet-50 runs in bf16 whatever `compute_dtype` says (as get_model)."""
    sd = torch.load(weights_path, weights_only=True, map_location=device)
    model = get_model(n_classes=5, compute_dtype=compute_dtype, arch=resolve_arch(arch, sd)).to(device)
    model.load_state_dict(sd)
    model.to(device).eval()
    return model


def _build_parser():
    return cli.build_parser(main.__doc__.splitlines()[0])


def _run(args, model, device, rank, world) -> Run:
    """The prediction itself, by one of three routes: `predict_random_patched`, the reference's callback loop (both under
    --random_sampler) or the sharded `predict_full_patched`.  Returns the Run with `pred`, `proba` (None without --proba) and
    `embeddings` (None unless an embedding flag took the features entry)."""
    from ..patch_samplers.full_samplers import FullImageRndSampler, SamplerExecutionMode

    anno_dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
    n_cls = len(anno_dsc.anno_classes)
    if args.synthetic is not None:
        img = tiles.synth_slide(args.synthetic[0], args.synthetic[1], 0, device)
        stem = f"synthetic_{args.synthetic[0]}x{args.synthetic[1]}"
    else:
        img, stem = Path(args.image), Path(args.image).stem
    mode = SamplerExecutionMode.ONDISK_MULTIPROC if args.ondisk else SamplerExecutionMode.INMEMORY_SINGLEPROC
    img = cli.slide.prepare(args, img, mode, device, rank)   # --pyramid, --stain
    if not args.random_sampler:
        smp = FullImageDenseSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                    mode=mode, stride=args.stride, device=device)
        info: dict = {}
        qinfo: dict = {}
        emb = None
        if any(on for _, on in embedding_flags(args)):
            # the same plan through the features entry; the map is finished from that pass's logits by predict_full_patched's tail
            filt = args.quality_filter if args.quality_filter is not None else args.tissue_filter
            emb = extract_embeddings(smp, model, tissue=args.tissue_filter, tissue_info=info,
                                     quality=args.quality_filter, quality_info=qinfo, return_logits=True)
            out = emb.class_map(args.downscale_vis, fill_class=-1 if filt is None else filt.fill_class)
            if args.save_embeddings and rank == 0:
                Path(args.save_embeddings).parent.mkdir(parents=True, exist_ok=True)
                emb.save(args.save_embeddings)
                print(f"embeddings: {len(emb)} tiles x {emb.width} floats -> {args.save_embeddings}", flush=True)
        elif args.fine:   # the same plan through the CAM entry: S x S rows per tile, each onto its own 32-pixel block
            out = predict_fine_patched(smp, model, n_cls, downscale=args.downscale_vis, tissue=args.tissue_filter, tissue_info=info,
                                       quality=args.quality_filter, quality_info=qinfo, return_proba=args.proba)
        else:
            out = predict_full_patched(smp, model, n_cls, downscale=args.downscale_vis,   # sharded when world > 1
                                       tissue=args.tissue_filter, tissue_info=info, return_proba=args.proba, tta=args.tta_aug,
                                       quality=args.quality_filter, quality_info=qinfo)
        pred, proba = out if args.proba else (out, None)
        if rank == 0:
            cli.filters.report_kept(args, info, qinfo)
        return Run(args, smp, img, stem, device, pred, proba, emb)
    if world > 1:
        raise RuntimeError("--random_sampler draws tiles from a running coverage map (one process); "
                           "the dense sampler is the multi-GPU path")
    smp = FullImageRndSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                              mode=mode, device=device)
    if smp.resident and smp.index_logic == "device" and isinstance(model, ResNetHIP):
        out = predict_random_patched(smp, model, n_cls, downscale=args.downscale_vis, return_proba=args.proba, tta=args.tta_aug)
        pred, proba = out if args.proba else (out, None)
        pred = pred.cpu().numpy()
    else:   # a foreign module or a slide streamed from disk: the reference's callback loop
        if args.tta_aug is not None:   # _check_args refused what it could see; a sampler that fell back to host index logic lands here
            raise ValueError("--tta runs on the fused routes only; this slide and sampler go through the per-batch callback")
        predictor = ImagePredictorPatched((smp.h, smp.w), patch_sampler=smp.generator(),
                                          batch_predictor=lambda patches: batch_predictor(patches, model, device),
                                          anno=anno_dsc, layer=args.layer, downscale=args.downscale_vis, device=device)
        pred = predictor.process()
        proba = predictor.process_proba() if args.proba else None
    return Run(args, smp, img, stem, device, pred, proba)


def main(argv=None, model=None):
    """The reference's `__main__` (predict_full_patched.py:128-177) as a per-rank program.

    The flags, their checks and what rank 0 reports for them live in deephisto_amd.cli, one module per flag group, each with its
    group's description.  The dense branch is the multi-GPU path: under
    `python -m torch.distributed.run --nproc-per-node N -m examples.predict_full_patched ...` every rank
    binds its GPU, joins the RCCL group, takes its contiguous tile range and the logits are exchanged with one
    all-gather (`predict_full_patched`); rank 0 writes the three JPEGs.  `--random_sampler` runs the reference's
    default branch (`FullImageRndSampler`, single process): `predict_random_patched` for a resident slide and a ResNet18HIP
    or ResNet50HIP model, `ImagePredictorPatched.process()` with the per-batch callback for an injected foreign model or `--ondisk`.
    `model`: an injected module (tests)."""
    from ..distributed import finalize, init_from_env
    from ..models.patch_cls_simple import utils

    ap = _build_parser()
    args = ap.parse_args(argv)
    _check_args(ap, args, model)
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
        run = _run(args, model, device, rank, world)
        pred = run.pred   # the reporters rebind run.pred to the map the region flags describe; main returns the class map
        if rank == 0:
            _report_rank0(run)
        if world > 1:
            dist.barrier()
        ok = True
        return pred
    finally:
        finalize(owned, ok)   # a failing rank leaves without a barrier (distributed.finalize)


if __name__ == "__main__":
    main()

