"""Whole-slide patched prediction -- drop-in for examples/predict_full_patched.py.

Keeps `ImagePredictorPatched(psim_path, patch_sampler, batch_predictor, anno, layer,
downscale).process()`, `batch_predictor(patches, model, device)`, `load_model(weights_path, device)` and the `__main__`
(predict_full_patched.py:22-78, 116-177), and re-exports the device engine (deephisto_amd.predict: `predict_full_patched(...)`,
the fast path used by bench.py, and `predict_random_patched(...)`; `ImagePredictorPatched.process_proba()` is their
`return_proba=True` for the callback route) and the visualiser (deephisto_amd.visualize: `perform_and_save_visualizations`,
`KNOWN_COLORS`, `save_proba`).
`score_prediction(pred, anno, ...)` (deephisto_amd.scoring) scores any of these maps against the
slide's polygon annotation; the CLI does so with `--anno PATH [--score_json PATH]`.
`extract_regions(pred, ...)` (deephisto_amd.regions) lists a map's connected regions, removes the small
ones and traces them into polygons; the CLI does so with `--regions_json`, `--min_region [--clean_rounds]`, `--export_anno`.
`extract_embeddings(sampler, model, ...)` (deephisto_amd.embeddings) hands out the per-tile feature vectors of
the same plan, and `PrototypeClassifier` scores them against class prototypes; the CLI does so with `--save_embeddings PATH` and
`--prototypes PATH`.  Without an annotation, `--clusters K` groups them by k-means (deephisto_amd.clustering)
and paints the cluster map; `--pca N` fits a principal-component basis on them (deephisto_amd.pca) and
paints the first three components as RGB.  `--knn K --knn_bank PATH` classifies them by their nearest labelled tiles and
`--similar_to Y,X` retrieves the tiles most like one tile (deephisto_amd.neighbours).
`margin_bands`, `tolerant_score` and `surface_distances` (deephisto_amd.distance) rest on the exact distance
transform of a class mask; the CLI runs them with `--margin LABEL:PX[,PX...]`, `--score_tolerance PX`, `--surface` and writes one
report with `--distance_json PATH`.
`main` calls `predict_full_patched` and `predict_random_patched` through this module's globals (tests replace them here).
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable

import numpy as np
import torch

from .. import tiles
from .._lib import DH_LAYOUT_NCHW, check  # noqa: F401  (exported here)
from ..anno.utils import AnnoDescription
from ..clustering import INITS as CLUSTER_INITS, KMeans, cluster_description, cluster_map, cluster_palette  # noqa: F401  (exported here)
from ..distance import (SurfaceDistance, band_composition, check_edges, class_mask, close, dilate, distance_transform, erode,  # noqa: F401  (exported here)
                        margin_bands, open_, save_distance_report, signed_distance, surface_distances, tolerant_score)
from ..cam import predict_fine_patched  # noqa: F401  (exported here)
from ..embeddings import PrototypeClassifier, SlideEmbeddings, extract_embeddings, tile_labels  # noqa: F401  (exported here)
from ..neighbours import KNNClassifier, cap_per_class, nearest_rows, similar_tiles  # noqa: F401  (exported here)
from ..models.patch_cls_simple.engine import ResNetHIP
from ..models.patch_cls_simple.model import ResNet18HIP, get_model
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


def _dense_resident_only(ap, args, who: str) -> None:
    """`who` (a flag, or a feature by name) runs over the dense sampler's grid of a resident slide: --random_sampler and --ondisk
    are argparse errors."""
    if args.random_sampler:
        ap.error(f"{who} works on the dense sampler's grid; it cannot be combined with --random_sampler")
    if args.ondisk:
        ap.error(f"{who} needs the slide resident in HBM; it cannot be combined with --ondisk")


def _fill_class(ap, flag: str, spelled: str) -> int:
    """The class id of a --tissue_fill / --quality_fill value: a class label, or -1 for no class."""
    labels = {a.label: a.id for a in AnnoDescription.with_known_colors(KNOWN_COLORS).anno_classes}
    if spelled != "-1" and spelled not in labels:
        ap.error(f"{flag} must be one of {', '.join(labels)} or -1, not {spelled!r}")
    return labels.get(spelled, -1)


def _tissue_from_args(ap, args) -> TissueFilter | None:
    """The TissueFilter of the --tissue flags, or None for `--tissue off`; a bad combination is an argparse error."""
    if args.tissue == "off":
        return None
    _dense_resident_only(ap, args, "--tissue")
    fill = _fill_class(ap, "--tissue_fill", args.tissue_fill)
    try:
        threshold = "otsu" if args.tissue == "otsu" else int(args.tissue)
    except ValueError:
        ap.error(f"--tissue must be off, otsu or an integer threshold in [0, 255], not {args.tissue!r}")
    try:
        return TissueFilter(threshold, args.tissue_min_fraction, fill)
    except ValueError as e:
        ap.error(f"--tissue {args.tissue} / --tissue_min_fraction {args.tissue_min_fraction}: {e}")


def _quality_from_args(ap, args) -> QualityFilter | None:
    """The QualityFilter of --min_sharpness / --max_ink / --quality_fill (any of them switches it on), or None; a bad
    combination is an argparse error."""
    if args.min_sharpness is None and args.max_ink is None and args.quality_fill is None:
        if args.quality_json:
            ap.error("--quality_json needs --min_sharpness, --max_ink or --quality_fill")
        return None
    _dense_resident_only(ap, args, "the quality filter")
    spelled = args.quality_fill if args.quality_fill is not None else "-1"
    fill = _fill_class(ap, "--quality_fill", spelled)
    try:
        filt = QualityFilter(0 if args.min_sharpness is None else args.min_sharpness,
                             1.0 if args.max_ink is None else args.max_ink, fill_class=fill)
    except ValueError as e:
        ap.error(f"--min_sharpness {args.min_sharpness} / --max_ink {args.max_ink}: {e}")
    if not 0 < args.patch_size <= 1024:
        ap.error(f"the quality filter takes --patch_size in [1, 1024], not {args.patch_size}")
    if args.tissue_filter is not None and args.tissue_filter.fill_class != filt.fill_class:
        ap.error(f"--tissue_fill {args.tissue_fill} and --quality_fill {spelled} must name the same class")
    return filt


def _stain_from_args(ap, args) -> StainNormalizer | None:
    """The StainNormalizer of the --stain flags, or None for `--stain off`; a bad combination is an argparse error."""
    if args.stain == "off":
        if args.stain_target or args.save_stain_fit:
            ap.error("--stain_target and --save_stain_fit need --stain macenko")
        return None
    if args.ondisk:
        ap.error("--stain needs the slide resident in HBM; it cannot be combined with --ondisk")
    target = None
    if args.stain_target:
        if not Path(args.stain_target).is_file():
            ap.error(f"--stain_target {args.stain_target}: no such file")
        try:
            target = StainFit.from_json(Path(args.stain_target).read_text())
            return StainNormalizer(args.stain, target=target)
        except (ValueError, TypeError) as e:
            ap.error(f"--stain_target {args.stain_target}: not a usable StainFit ({e})")
    return StainNormalizer(args.stain)


def _tta_from_args(ap, args, model=None) -> TestTimeAugmenter | None:
    """The TestTimeAugmenter of --tta, or None for `--tta off`; a bad combination is an argparse error.  `model`: the module
    injected into main, if any: a foreign one under --random_sampler goes the callback route, which has no views."""
    if args.tta == "off":
        return None
    if args.ondisk:
        ap.error("--tta needs the slide resident in HBM; it cannot be combined with --ondisk")
    if args.random_sampler and model is not None and not isinstance(model, ResNetHIP):
        ap.error("--tta runs on the fused routes (a ResNet18HIP or ResNet50HIP model); under --random_sampler a foreign model "
                 "goes through the per-batch callback, which has no views")
    return TestTimeAugmenter(args.tta)


def _pyramid_from_args(ap, args) -> None:
    """Checks --pyramid; a bad combination is an argparse error."""
    if not args.pyramid:
        return
    if args.ondisk:
        ap.error("--pyramid holds the layer resident in HBM; it cannot be combined with --ondisk")
    if args.synthetic is None and Path(args.image).suffix != ".npy":
        ap.error(f"--pyramid serves the layers of a --synthetic slide or a .npy image; {args.image} goes to psimage, "
                 "which has layers of its own")


def _proba_from_args(ap, args) -> None:
    """Checks the --proba flags; a bad combination or an unknown class label is an argparse error."""
    if args.heat and not args.proba:
        ap.error("--heat needs --proba")
    if args.save_proba and not args.proba:
        ap.error("--save_proba needs --proba")
    for lb in args.heat:
        if lb not in KNOWN_COLORS:
            ap.error(f"--heat labels must be out of {', '.join(KNOWN_COLORS)}, not {lb!r}")


def _embeddings_from_args(ap, args) -> None:
    """Checks --save_embeddings / --prototypes / --clusters / --pca / --knn / --similar_to; a bad combination is an argparse error."""
    if args.knn is not None and not args.knn_bank:
        ap.error("--knn needs --knn_bank")
    if args.knn_bank and args.knn is None:
        ap.error("--knn_bank needs --knn")
    if args.knn_per_class is not None and args.knn is None:
        ap.error("--knn_per_class needs --knn")
    if args.similar_to is None and (args.similar_k is not None or args.similar_json):
        ap.error("--similar_k and --similar_json need --similar_to")
    for flag, value in (("--save_embeddings", args.save_embeddings), ("--prototypes", args.prototypes),
                        ("--clusters", args.clusters), ("--load_clusters", args.load_clusters),
                        ("--pca", args.pca is not None), ("--load_pca", args.load_pca),
                        ("--knn", args.knn is not None), ("--similar_to", args.similar_to is not None)):
        if not value:
            continue
        _dense_resident_only(ap, args, flag)
        if args.tta != "off":
            ap.error(f"{flag} stores one forward pass per tile; it cannot be combined with --tta")
        if args.proba:
            ap.error(f"{flag} finishes the class map from the stored logits; it cannot be combined with --proba")
    if args.prototypes and not args.anno and not Path(args.prototypes).is_file():
        ap.error(f"--prototypes {args.prototypes}: no such file (with --anno the prototypes are fitted and written there)")
    if args.clusters is not None and not 1 <= args.clusters <= 64:
        ap.error(f"--clusters must be in 1 .. 64, not {args.clusters}")
    if args.load_clusters:
        if args.save_clusters or args.cluster_seed is not None or args.cluster_init is not None:
            ap.error("--load_clusters applies a saved codebook: --save_clusters, --cluster_seed and --cluster_init belong to a fit")
        if not Path(args.load_clusters).is_file():
            ap.error(f"--load_clusters {args.load_clusters}: no such file")
    elif args.clusters is None and (args.save_clusters or args.cluster_seed is not None or args.cluster_init is not None):
        ap.error("--save_clusters, --cluster_seed and --cluster_init need --clusters")
    if (args.clusters is not None or args.load_clusters) and args.min_region is not None:
        ap.error("--min_region cleans the class map; with --clusters the region flags describe the cluster map as it is")
    if args.pca is not None and not 1 <= args.pca <= 64:
        ap.error(f"--pca must be in 1 .. 64, not {args.pca}")
    if args.load_pca:
        if args.save_pca or args.pca is not None:
            ap.error("--load_pca applies a saved basis: --pca and --save_pca belong to a fit")
        if not Path(args.load_pca).is_file():
            ap.error(f"--load_pca {args.load_pca}: no such file")
    elif args.save_pca and args.pca is None:
        ap.error("--save_pca needs --pca")
    _knn_from_args(ap, args)


def _knn_from_args(ap, args) -> None:
    """Checks --knn / --knn_bank / --knn_per_class and --similar_to / --similar_k; leaves the pixel of --similar_to as a
    (y, x) tuple in `args.similar_yx` (None without the flag)."""
    n_cls = len(KNOWN_COLORS)
    if args.knn is not None:
        if not 1 <= args.knn <= 63:
            ap.error(f"--knn must be in 1 .. 63 (leave-one-out asks for one neighbour more), not {args.knn}")
        if args.knn_per_class is not None and not args.anno:
            ap.error("--knn_per_class caps a fit: it needs --anno")
        if args.knn_per_class is not None and args.knn_per_class < 1:
            ap.error(f"--knn_per_class must be >= 1, not {args.knn_per_class}")
        if args.clusters is not None or args.load_clusters:
            ap.error("--knn and --clusters each hand their own map to the region flags; run them one at a time")
        if args.min_region is not None:
            ap.error("--min_region cleans the class map; with --knn the region flags describe the k-NN map as it is")
        if not args.anno:
            if not Path(args.knn_bank).is_file():
                ap.error(f"--knn_bank {args.knn_bank}: no such file (with --anno the bank is fitted and written there)")
            try:
                bank = KNNClassifier.load(args.knn_bank)
            except (ValueError, KeyError, OSError) as e:
                ap.error(f"--knn_bank {args.knn_bank}: not a KNNClassifier file ({e!r})")
            arch = resolve_arch(None) if args.arch == "auto" and not args.weights else args.arch
            width = {"resnet18": 512, "resnet50": 2048}.get(arch)   # auto with a checkpoint: known once it is read (_knn_rank0)
            if bank.n_classes != n_cls or (width is not None and bank.bank.shape[1] != width):
                ap.error(f"--knn_bank {args.knn_bank}: {bank.n_classes} classes x {bank.bank.shape[1]} floats do not fit this model "
                         f"and description ({n_cls} x {width or 'the model width'})")
    args.similar_yx = None
    if args.similar_to is not None:
        try:
            y, x = (int(v) for v in args.similar_to.split(","))
        except ValueError:
            ap.error(f"--similar_to takes Y,X (a pixel of the slide), not {args.similar_to!r}")
        if args.synthetic is not None and not args.pyramid and not (0 <= y < args.synthetic[0] and 0 <= x < args.synthetic[1]):
            ap.error(f"--similar_to {y},{x} lies outside the slide ({args.synthetic[0]} x {args.synthetic[1]})")
        if min(y, x) < 0:
            ap.error(f"--similar_to {y},{x} lies outside the slide")
        if args.similar_k is not None and not 1 <= args.similar_k <= 63:
            ap.error(f"--similar_k must be in 1 .. 63, not {args.similar_k}")
        args.similar_yx = (y, x)


def _fine_from_args(ap, args) -> None:
    """Checks --fine; a bad combination is an argparse error."""
    if not args.fine:
        return
    _dense_resident_only(ap, args, "--fine")
    if args.tta != "off":
        ap.error("--fine places every position of a tile's last feature map; a rotated view permutes them: it cannot be combined "
                 "with --tta")
    for flag, value in (("--save_embeddings", args.save_embeddings), ("--prototypes", args.prototypes),
                        ("--clusters", args.clusters is not None), ("--load_clusters", args.load_clusters),
                        ("--pca", args.pca is not None), ("--load_pca", args.load_pca),
                        ("--knn", args.knn is not None), ("--similar_to", args.similar_to is not None)):
        if value:
            ap.error(f"{flag} finishes the class map from one logits row per tile; it cannot be combined with --fine")
    if args.patch_size % 32:
        ap.error(f"--fine needs a --patch_size that is a multiple of 32, not {args.patch_size}")


def _regions_from_args(ap, args) -> None:
    """Checks the region flags; a bad combination is an argparse error."""
    if args.clean_rounds is not None and args.min_region is None:
        ap.error("--clean_rounds needs --min_region")
    if args.min_region is not None and args.min_region < 1:
        ap.error(f"--min_region must be >= 1, not {args.min_region}")
    if args.clean_rounds is not None and args.clean_rounds < 1:
        ap.error(f"--clean_rounds must be >= 1, not {args.clean_rounds}")


def _distance_from_args(ap, args) -> None:
    """Checks --margin / --score_tolerance / --surface / --distance_json; leaves (label, edges in px) of --margin in
    `args.margin_spec` (None without the flag).  A bad combination is an argparse error."""
    args.margin_spec = None
    if args.score_tolerance is not None and not args.anno:
        ap.error("--score_tolerance needs --anno")
    if args.surface and not args.anno:
        ap.error("--surface needs --anno")
    if args.score_tolerance is not None and args.score_tolerance < 0:
        ap.error(f"--score_tolerance must be >= 0, not {args.score_tolerance}")
    if args.distance_json and args.margin is None and args.score_tolerance is None and not args.surface:
        ap.error("--distance_json needs --margin, --score_tolerance or --surface")
    steps = [f for f, on in (("--margin", args.margin is not None), ("--score_tolerance", args.score_tolerance is not None),
                             ("--surface", args.surface)) if on]
    if steps and (args.clusters is not None or args.load_clusters):
        ap.error(f"{steps[0]} names the classes of the description; it cannot be combined with --clusters, whose map holds clusters")
    if args.margin is None:
        return
    label, sep, spelled = args.margin.partition(":")
    if not sep or not spelled:
        ap.error(f"--margin takes LABEL:PX[,PX...], not {args.margin!r}")
    if label not in KNOWN_COLORS:
        ap.error(f"--margin label must be out of {', '.join(KNOWN_COLORS)}, not {label!r}")
    try:
        edges = [int(v) for v in spelled.split(",")]
    except ValueError:
        ap.error(f"--margin takes LABEL:PX[,PX...] with integer PX, not {args.margin!r}")
    if len(edges) == 1:
        if edges[0] <= 0:
            ap.error(f"--margin {args.margin}: a single PX must be > 0 (it stands for -PX,0,PX)")
        edges = [-edges[0], 0, edges[0]]
    try:
        edges = check_edges(edges)
    except ValueError:
        ap.error(f"--margin {args.margin}: the edges must ascend strictly (and stay below 2^31 px, at most 64 bands)")
    args.margin_spec = (label, edges)


def _build_parser():
    import argparse

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
    ap.add_argument("--min_sharpness", type=int, default=None, metavar="N",
                    help="reject out-of-focus tiles: Laplacian variance of the luma over a tile's tissue pixels below N grey levels "
                         "squared (0..1040400; dense branch only; --quality_json reports the slide's quartiles)")
    ap.add_argument("--max_ink", type=float, default=None, metavar="F",
                    help="reject tiles with more than the share F of pen-mark or very dark pixels (0..1)")
    ap.add_argument("--quality_fill", default=None, help="class label for cells no kept tile covers, or -1 (as --tissue_fill)")
    ap.add_argument("--quality_json", default=None, metavar="PATH",
                    help="with the quality filter: thresholds, counts and the sharpness quartiles of the scored tiles as JSON (rank 0)")
    ap.add_argument("--pyramid", action="store_true",
                    help="--layer L of a --synthetic slide or a .npy image is the slide at 1/L of its resolution, area-averaged on the "
                         "device (PyramidSlide); without it such a slide has one layer, whatever --layer says")
    ap.add_argument("--stain", choices=["off", "macenko"], default="off",
                    help="normalise the slide's stain appearance on the device before anything reads it (resident slide); "
                         "with --pyramid the layer is normalised, not the base")
    ap.add_argument("--stain_target", default=None, metavar="PATH", help="with --stain: a StainFit JSON (another slide's fit) as the target")
    ap.add_argument("--save_stain_fit", default=None, metavar="PATH", help="with --stain: this slide's StainFit as JSON (rank 0)")
    ap.add_argument("--tta", choices=["off", "flips", "d4"], default="off",
                    help="test-time augmentation: classify every tile in 4 (flips) or all 8 (d4) orientations of the square and "
                         "average the logits (resident slide; 4 / 8 times the forward work)")
    ap.add_argument("--fine", action="store_true",
                    help="the map from the class activation maps of the last conv: values change every 32 px, same forward pass "
                         "(dense sampler, resident slide, --patch_size a multiple of 32)")
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
    ap.add_argument("--save_embeddings", default=None, metavar="PATH",
                    help="every classified tile's pooled feature vector (512 / 2048 floats), origins and logits as one .npz (rank 0); "
                         "the class map comes from the same forward pass (dense branch, resident slide)")
    ap.add_argument("--prototypes", default=None, metavar="PATH",
                    help="nearest-class-mean scoring of the tile embeddings: with --anno, fit the class prototypes on this slide's "
                         "annotated tiles and write them to PATH; without, load PATH and write {stem}_prototype_map.jpg")
    ap.add_argument("--clusters", type=int, default=None, metavar="K",
                    help="k-means over the tile embeddings of this pass (1 .. 64 clusters, no annotation needed): writes "
                         "{stem}_clusters.jpg and {stem}_clusters.json (rank 0); --regions_json / --export_anno then describe the "
                         "cluster map's regions, named cluster_0 ...")
    ap.add_argument("--cluster_seed", type=int, default=None, metavar="S", help="with --clusters: the seed of the k-means++ draws (default 0)")
    ap.add_argument("--cluster_init", choices=list(CLUSTER_INITS), default=None, help="with --clusters: the seeding (default kmeans++)")
    ap.add_argument("--save_clusters", default=None, metavar="PATH", help="with --clusters: the fitted codebook as one .npz (rank 0)")
    ap.add_argument("--load_clusters", default=None, metavar="PATH",
                    help="apply the codebook of an earlier --save_clusters to this slide instead of fitting (K comes from the file)")
    ap.add_argument("--pca", type=int, default=None, metavar="N",
                    help="principal components of the tile embeddings of this pass (1 .. 64, no annotation needed): writes "
                         "{stem}_pca.jpg, the first three components as red, green and blue, and {stem}_pca.json (rank 0)")
    ap.add_argument("--save_pca", default=None, metavar="PATH", help="with --pca: the fitted basis as one .npz (rank 0)")
    ap.add_argument("--load_pca", default=None, metavar="PATH",
                    help="apply the basis of an earlier --save_pca to this slide instead of fitting (N comes from the file)")
    ap.add_argument("--knn", type=int, default=None, metavar="K",
                    help="k-nearest-neighbour classification of the tile embeddings against a bank of labelled tiles (1 .. 63, "
                         "needs --knn_bank): writes {stem}_knn.jpg and {stem}_knn_overlay.jpg (rank 0); --regions_json / "
                         "--export_anno then describe that map's regions")
    ap.add_argument("--knn_bank", default=None, metavar="PATH",
                    help="with --knn: with --anno, fit the bank on this slide's annotated tiles, write it to PATH and print the "
                         "leave-one-out accuracy; without, load PATH")
    ap.add_argument("--knn_per_class", type=int, default=None, metavar="N",
                    help="with --knn and --anno: at most N tiles of a class enter the bank (every ceil(count / N)-th, in tile order)")
    ap.add_argument("--similar_to", default=None, metavar="Y,X",
                    help="retrieval: the tiles of this slide most like the tile under pixel Y,X, as JSON (rank 0)")
    ap.add_argument("--similar_k", type=int, default=None, metavar="K", help="with --similar_to: how many tiles (1 .. 63, default 16)")
    ap.add_argument("--similar_json", default=None, metavar="PATH",
                    help="with --similar_to: where the JSON goes (default {out_dir}/{stem}_similar.json)")
    ap.add_argument("--margin", default=None, metavar="LABEL:PX[,PX...]",
                    help="bands of distance around class LABEL, edges in layer pixels, negative inside the class (a single PX means "
                         "-PX,0,PX): prints the classes per band and writes {stem}_margin.jpg (rank 0)")
    ap.add_argument("--score_tolerance", type=int, default=None, metavar="PX",
                    help="with --anno: a second score that leaves out the cells within PX layer pixels of a label change of the annotation")
    ap.add_argument("--surface", action="store_true",
                    help="with --anno: Hausdorff, HD95 and average symmetric surface distance of every class the annotation holds")
    ap.add_argument("--distance_json", default=None, metavar="PATH",
                    help="with --margin, --score_tolerance or --surface: their results as one JSON (rank 0)")
    return ap


def _check_args(ap, args, model=None) -> None:
    """The flag checkers, before the process group or any GPU is touched; leaves the TissueFilter (or None) in
    `args.tissue_filter`, the QualityFilter (or None) in `args.quality_filter`, the StainNormalizer (or None) in `args.stain_norm`, the TestTimeAugmenter (or None) in `args.tta_aug`
    and the records of --anno (or None) in `args.anno_records`.  `model`: the module injected into main, if any."""
    _regions_from_args(ap, args)
    _pyramid_from_args(ap, args)
    args.stain_norm = _stain_from_args(ap, args)
    args.tissue_filter = _tissue_from_args(ap, args)
    args.quality_filter = _quality_from_args(ap, args)
    args.tta_aug = _tta_from_args(ap, args, model)
    args.anno_records = _anno_from_args(ap, args)
    _proba_from_args(ap, args)
    _embeddings_from_args(ap, args)
    _fine_from_args(ap, args)
    _distance_from_args(ap, args)


def _run(args, model, device, rank, world):
    """The prediction itself, by one of three routes: `predict_random_patched`, the reference's callback loop (both under
    --random_sampler) or the sharded `predict_full_patched`.  Returns (pred, proba, sampler, img, stem); `proba` is None
    without --proba."""
    from ..patch_samplers.full_samplers import FullImageRndSampler, SamplerExecutionMode

    anno_dsc = AnnoDescription.with_known_colors(KNOWN_COLORS)
    n_cls = len(anno_dsc.anno_classes)
    if args.synthetic is not None:
        img = tiles.synth_slide(args.synthetic[0], args.synthetic[1], 0, device)
        stem = f"synthetic_{args.synthetic[0]}x{args.synthetic[1]}"
    else:
        img, stem = Path(args.image), Path(args.image).stem
    mode = SamplerExecutionMode.ONDISK_MULTIPROC if args.ondisk else SamplerExecutionMode.INMEMORY_SINGLEPROC
    if args.pyramid:
        # the layer takes the slide's place for every route below and for the overlays; --stain then
        # normalises the layer.  A .npy image goes up in bands, so HBM holds the layer and one band, never the whole scan
        from ..resample import PyramidSlide
        img = PyramidSlide(img, device=device).layer_device(args.layer)
    if args.stain_norm is not None:
        # the normalised slide takes the raw one's place for every route below and for the overlays (the map and the picture
        # under it must agree); every rank normalises its own copy, integer-exact, so all hold the same pixels
        if not isinstance(img, torch.Tensor):
            img = FullImageDenseSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                        mode=mode, stride=args.stride, device=device).data_device
        sinfo: dict = {}
        img = args.stain_norm.normalize(img, sinfo)
        fit = sinfo["fit"]
        if rank == 0:
            print(f"stain: identity fit ({fit.reason})" if fit.identity else
                  f"stain: {fit.n_stained} stained pixels, HE {np.round(np.array(fit.HE).T, 4).tolist()}, "
                  f"maxC {np.round(fit.maxC, 4).tolist()}", flush=True)
            if args.save_stain_fit:
                Path(args.save_stain_fit).parent.mkdir(parents=True, exist_ok=True)
                Path(args.save_stain_fit).write_text(fit.to_json())
    if not args.random_sampler:
        smp = FullImageDenseSampler(img, layer=args.layer, patch_size=args.patch_size, batch_size=args.batch_size,
                                    mode=mode, stride=args.stride, device=device)
        info: dict = {}
        qinfo: dict = {}
        args.embeddings = None
        if args.save_embeddings or args.prototypes or args.clusters is not None or args.load_clusters or args.pca is not None \
                or args.load_pca or args.knn is not None or args.similar_to is not None:
            # the same plan through the features entry; the map is finished from that pass's logits by predict_full_patched's tail
            filt = args.quality_filter if args.quality_filter is not None else args.tissue_filter
            emb = args.embeddings = extract_embeddings(smp, model, tissue=args.tissue_filter, tissue_info=info,
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
        if args.tissue_filter is not None and rank == 0:
            print(f"kept {info['n_kept']} of {info['n_tiles']} tiles, threshold {info['threshold']}", flush=True)
        if args.quality_filter is not None and rank == 0:
            print(f"quality: {qinfo['n_kept']} of {qinfo['n_tiles']} tiles pass, {qinfo['rejected_blur']} blurred "
                  f"(min_sharpness {qinfo['min_sharpness']}), {qinfo['rejected_ink']} ink-marked "
                  f"(more than {qinfo['max_ink_pixels']} pixels)", flush=True)
            if args.quality_json:
                _save_quality(args.quality_json, args.quality_filter, qinfo)
        return pred, proba, smp, img, stem
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
    return pred, proba, smp, img, stem


def _save_quality(path, filt: QualityFilter, qinfo: dict) -> None:
    """--quality_json: the filter's thresholds, the counts and the five-number summary of the scored tiles' sharpness."""
    import json

    doc = dict(min_sharpness=qinfo["min_sharpness"], max_ink_fraction=filt.max_ink_fraction, max_ink_pixels=qinfo["max_ink_pixels"],
               ink_chroma=filt.ink_chroma, ink_margin=filt.ink_margin, dark_max=filt.dark_max, fill_class=filt.fill_class,
               threshold=qinfo["threshold"], n_tiles=qinfo["n_tiles"], n_kept=qinfo["n_kept"],
               rejected_blur=qinfo["rejected_blur"], rejected_ink=qinfo["rejected_ink"],
               sharpness=sharpness_summary(qinfo["stats"]))
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(doc, indent=1) + "\n")


def _prototypes_rank0(args, smp, src, stem, anno_dsc, out_dir, device) -> None:
    """--prototypes: with --anno, fit the class prototypes on this slide's annotated tiles (the label of a tile is the annotation's
    at the cell under its centre) and save them; without, load them and write the prototype class map over the slide."""
    emb, n_cls = args.embeddings, len(anno_dsc.anno_classes)
    if args.anno_records is not None:
        truth, _ = rasterize_annotation(args.anno_records, anno_dsc, args.layer, smp.h, smp.w, args.downscale_vis, device=device)
        pc = PrototypeClassifier(n_cls).fit(emb, tile_labels(emb, truth, args.downscale_vis))
        Path(args.prototypes).parent.mkdir(parents=True, exist_ok=True)
        pc.save(args.prototypes)
        print(f"prototypes: {int(pc.counts.sum())} labelled tiles, per class {pc.counts.tolist()}, empty {pc.empty_classes} "
              f"-> {args.prototypes}", flush=True)
        return
    pc = PrototypeClassifier.load(args.prototypes, device=device)
    if pc.n_classes != n_cls or pc.prototypes.shape[1] != emb.width:
        raise ValueError(f"--prototypes {args.prototypes}: {pc.n_classes} classes x {pc.prototypes.shape[1]} floats do not fit this "
                         f"model and description ({n_cls} x {emb.width})")
    pmap = pc.predict_map(emb, args.downscale_vis)
    if not args.no_visualizations:
        _, _, overlay = perform_and_save_visualizations(src, anno_dsc, pmap, stem=stem, save=False, device=device)
        out_dir.mkdir(exist_ok=True, parents=True)
        _save_jpeg(overlay, out_dir / f"{stem}_prototype_map.jpg")


def _knn_rank0(args, smp, src, stem, anno_dsc, out_dir, device):
    """--knn: with --anno, fit the bank on this slide's annotated tiles (the label of a tile is the annotation's at the cell under
    its centre, --knn_per_class caps a class), save it and print the leave-one-out accuracy; without, load it.  Either way write
    `{stem}_knn.jpg` and `{stem}_knn_overlay.jpg` from the k-NN class map, which is returned."""
    emb, n_cls = args.embeddings, len(anno_dsc.anno_classes)
    if args.anno_records is not None:
        truth, _ = rasterize_annotation(args.anno_records, anno_dsc, args.layer, smp.h, smp.w, args.downscale_vis, device=device)
        labels = tile_labels(emb, truth, args.downscale_vis)
        if args.knn_per_class is not None:
            labels = cap_per_class(labels, n_cls, args.knn_per_class)
        knn = KNNClassifier(n_cls, k=args.knn).fit(emb, labels)
        Path(args.knn_bank).parent.mkdir(parents=True, exist_ok=True)
        knn.save(args.knn_bank)
        loo = f"{knn.leave_one_out()[0]:.4f}" if len(knn.bank) else "none (an empty bank)"
        print(f"knn: k = {knn.k}, {len(knn.bank)} labelled tiles in the bank, per class {knn.counts.tolist()}, "
              f"leave-one-out accuracy {loo} -> {args.knn_bank}", flush=True)
    else:
        knn = KNNClassifier.load(args.knn_bank, device=device)
        knn.k = args.knn
        if knn.n_classes != n_cls or knn.bank.shape[1] != emb.width:
            raise ValueError(f"--knn_bank {args.knn_bank}: {knn.n_classes} classes x {knn.bank.shape[1]} floats do not fit this "
                             f"model and description ({n_cls} x {emb.width})")
    kmap = knn.predict_map(emb, args.downscale_vis)
    if not args.no_visualizations:
        mask, _, overlay = perform_and_save_visualizations(src, anno_dsc, kmap, stem=stem, save=False, device=device)
        out_dir.mkdir(exist_ok=True, parents=True)
        _save_jpeg(mask, out_dir / f"{stem}_knn.jpg")
        _save_jpeg(overlay, out_dir / f"{stem}_knn_overlay.jpg")
    return kmap


def _similar_rank0(args, stem, out_dir) -> None:
    """--similar_to Y,X: the tiles of this slide most like the tile under that pixel, nearest first, as JSON."""
    import json

    emb = args.embeddings
    y, x = args.similar_yx
    if not (y < emb.h and x < emb.w):
        raise ValueError(f"--similar_to {y},{x} lies outside the slide ({emb.h} x {emb.w})")
    res = similar_tiles(emb, (y, x), k=args.similar_k or 16)
    doc = dict(pixel=[y, x], query_row=res["query_row"], query_origin=res["query_origin"].tolist(), patch_size=emb.patch_size,
               k=len(res["rows"]), rows=res["rows"].tolist(), origins=res["origins"].tolist(),
               dist=[float(d) for d in res["dist"]])
    path = Path(args.similar_json) if args.similar_json else out_dir / f"{stem}_similar.json"
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"similar: {len(res['rows'])} tiles like the one at {doc['query_origin']} -> {path}", flush=True)


def _clusters_rank0(args, src, stem, out_dir, device):
    """--clusters / --load_clusters: fit k-means on this slide's embeddings (or apply a saved codebook), write
    `{stem}_clusters.json` and, with visualisations, `{stem}_clusters.jpg`.  Returns (cluster map, its AnnoDescription)."""
    import json

    emb = args.embeddings
    if args.load_clusters:
        km = KMeans.load(args.load_clusters, device=device)
        if km.centres_.shape[1] != emb.width or (args.clusters is not None and args.clusters != km.n_clusters):
            raise ValueError(f"--load_clusters {args.load_clusters}: {km.n_clusters} clusters x {km.centres_.shape[1]} floats do not fit "
                             f"this run ({'any' if args.clusters is None else args.clusters} x {emb.width})")
        labels, dist = km.predict(emb, return_dist=True)
        sizes = torch.bincount(labels[labels >= 0].to(torch.int64), minlength=km.n_clusters).cpu().numpy().tolist()
        inertia = float(dist.double().sum())
    else:
        km = KMeans(args.clusters, init=args.cluster_init or "kmeans++", seed=args.cluster_seed or 0).fit(emb)
        labels, sizes, inertia = km.labels_, km.counts_.tolist(), km.inertia_
        if args.save_clusters:
            Path(args.save_clusters).parent.mkdir(parents=True, exist_ok=True)
            km.save(args.save_clusters)
    K = km.n_clusters
    print(f"clusters: {K} over {len(emb)} tiles, sizes {sizes}, inertia {inertia:.6g}, "
          + (f"codebook {args.load_clusters}" if args.load_clusters else
             f"{km.n_iter_} iterations, {'converged' if km.converged_ else 'not converged'}"), flush=True)
    dsc = cluster_description(K)
    cmap = cluster_map(emb, labels, K, args.downscale_vis)
    out_dir.mkdir(exist_ok=True, parents=True)
    doc = dict(n_clusters=K, n_tiles=len(emb), sizes=sizes, inertia=inertia, iterations=km.n_iter_, converged=km.converged_,
               init=km.init, seed=km.seed, normalize=km.normalize, fitted_here=not args.load_clusters,
               colors={a.label: list(a.color) for a in dsc.anno_classes})
    (out_dir / f"{stem}_clusters.json").write_text(json.dumps(doc, indent=1) + "\n")
    if not args.no_visualizations:
        _, _, overlay = perform_and_save_visualizations(src, dsc, cmap, stem=stem, save=False, device=device)
        _save_jpeg(overlay, out_dir / f"{stem}_clusters.jpg")
    return cmap, dsc


def _pca_rank0(args, stem, out_dir, device) -> None:
    """--pca / --load_pca: fit a principal-component basis on this slide's embeddings (or apply a saved one), write
    `{stem}_pca.json` and, with visualisations, `{stem}_pca.jpg`: the first min(3, N) components as red, green and blue."""
    import json
    import time

    emb = args.embeddings
    if args.load_pca:
        pca = PCA.load(args.load_pca, device=device)
        if pca.components_.shape[1] != emb.width:
            raise ValueError(f"--load_pca {args.load_pca}: a basis of {pca.components_.shape[1]} columns does not fit this run "
                             f"({emb.width})")
    else:
        pca = PCA(args.pca).fit(emb)
        if args.save_pca:
            Path(args.save_pca).parent.mkdir(parents=True, exist_ok=True)
            pca.save(args.save_pca)
    N = pca.n_components
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    pca.transform(emb)
    torch.cuda.synchronize(device)
    project_ms = 1e3 * (time.perf_counter() - t0)
    ratio = pca.explained_variance_ratio_
    print(f"pca: {N} components over {len(emb)} tiles, explained variance {float(ratio.sum()):.4f} "
          f"(first {float(ratio[0]):.4f}), " + (f"basis {args.load_pca}" if args.load_pca else f"fitted on {pca.n_samples_} rows"),
          flush=True)
    out_dir.mkdir(exist_ok=True, parents=True)
    doc = dict(n_components=N, n_tiles=len(emb), n_samples=pca.n_samples_, explained_variance=pca.explained_variance_.tolist(),
               explained_variance_ratio=ratio.tolist(), scatter_ms=pca.timings_.get("scatter_ms"), eigen_ms=pca.timings_.get("eigen_ms"),
               project_ms=project_ms, fitted_here=not args.load_pca)
    (out_dir / f"{stem}_pca.json").write_text(json.dumps(doc, indent=1) + "\n")
    if not args.no_visualizations:
        _save_jpeg(pca.colour_map(emb, args.downscale_vis, components=tuple(range(min(3, N)))), out_dir / f"{stem}_pca.jpg")


def _report_rank0(args, pred, proba, smp, img, stem, device) -> None:
    """What rank 0, where the map is whole, prints and writes after the prediction: the score, the JPEGs, the probability
    files, then the regions with the cleaned map's score and JPEGs, then the distance steps on the map the regions describe."""
    anno_dsc, out_dir = AnnoDescription.with_known_colors(KNOWN_COLORS), Path(args.out_dir)
    src = None if args.no_visualizations else img if isinstance(img, torch.Tensor) or not smp.resident else smp.data_device
    truth = outcome = None
    if args.anno_records is not None:
        score, truth, outcome, anno_info = score_prediction(pred, args.anno_records, anno_dsc, args.layer, smp.h, smp.w,
                                                            args.downscale_vis, return_maps=True, device=device)
        print(score, flush=True)
        print(f"annotation: {anno_info['n_rings']} rings of {anno_info['n_regions']} regions, "
              f"{anno_info['skipped_class']} of unknown class, {anno_info['failed']} failed to parse", flush=True)
        if args.score_json:
            save_score(args.score_json, score, anno_info)
    if not args.no_visualizations:
        perform_and_save_visualizations(src, anno_dsc, pred, out_dir=out_dir, stem=stem, device=device,
                                        proba=proba, heat_classes=args.heat, truth=truth, outcome=outcome)
    if args.save_proba:
        save_proba(args.save_proba, proba)
    if args.prototypes:
        _prototypes_rank0(args, smp, src, stem, anno_dsc, out_dir, device)
    if args.pca is not None or args.load_pca:
        _pca_rank0(args, stem, out_dir, device)
    if args.similar_to is not None:
        _similar_rank0(args, stem, out_dir)
    if args.knn is not None:
        pred = _knn_rank0(args, smp, src, stem, anno_dsc, out_dir, device)   # the region flags below describe the k-NN map
    if args.clusters is not None or args.load_clusters:
        pred, anno_dsc = _clusters_rank0(args, src, stem, out_dir, device)   # the region flags below describe the cluster map
    if args.regions_json or args.min_region is not None or args.export_anno:
        pred = _regions_rank0(args, pred, proba, smp, src, stem, anno_dsc, out_dir, device)   # the cleaned map under --min_region
    if args.margin_spec is not None or args.score_tolerance is not None or args.surface:
        _distance_rank0(args, pred, truth, src, stem, anno_dsc, out_dir, device)


def _regions_rank0(args, pred, proba, smp, src, stem, anno_dsc, out_dir, device):
    """The region flags: table, cleanup, polygons, the cleaned map's score and JPEGs.  Returns the map they describe: the
    cleaned one under --min_region, else `pred`."""
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
    if args.min_region is not None and args.anno_records is not None:
        print("cleaned map:", flush=True)
        print(score_prediction(res.class_map, args.anno_records, anno_dsc, args.layer, smp.h, smp.w, args.downscale_vis,
                               device=device), flush=True)
    if args.min_region is not None and not args.no_visualizations:
        mask, _, overlay = perform_and_save_visualizations(src, anno_dsc, res.class_map, stem=stem, save=False, device=device)
        out_dir.mkdir(exist_ok=True, parents=True)
        _save_jpeg(mask, out_dir / f"{stem}_clean_mask.jpg")
        _save_jpeg(overlay, out_dir / f"{stem}_clean_overlay.jpg")
    return res.class_map if args.min_region is not None else pred


def _distance_rank0(args, pred, truth, src, stem, anno_dsc, out_dir, device) -> None:
    """--margin / --score_tolerance / --surface on `pred` (the map the region flags describe) and `truth` (the annotation's label
    map, None without --anno): prints the figures, writes `{stem}_margin.jpg` and the report of --distance_json."""
    labels = [""] * (max(a.id for a in anno_dsc.anno_classes) + 1)
    for a in anno_dsc.anno_classes:
        labels[a.id] = a.label
    d = args.downscale_vis
    margin = tolerant = surface = None
    if args.margin_spec is not None:
        label, edges = args.margin_spec
        bands = margin_bands(pred, [labels.index(label)], edges, d, device=device)
        counts = band_composition(pred, bands, len(labels), len(edges) - 1)
        margin = dict(label=label, edges_px=edges, class_labels=labels, counts=counts)
        print(f"margin of {label}, edges {edges} px; cells per band of {', '.join(labels)}, no class:", flush=True)
        for i, row in enumerate(counts.tolist()):
            print(f"  [{edges[i]}, {edges[i + 1]}) {row}", flush=True)
        if not args.no_visualizations:
            dsc = AnnoDescription.with_known_colors({f"band_{i}": c for i, c in enumerate(cluster_palette(len(edges) - 1))})
            _, _, overlay = perform_and_save_visualizations(src, dsc, bands, stem=stem, save=False, device=device)
            out_dir.mkdir(exist_ok=True, parents=True)
            _save_jpeg(overlay, out_dir / f"{stem}_margin.jpg")
    if args.score_tolerance is not None:
        score = tolerant_score(pred, truth, labels, args.score_tolerance, d, device=device)
        tolerant = dict(tolerance_px=args.score_tolerance, score=score)
        print(f"score without the cells within {args.score_tolerance} px of a label change:", flush=True)
        print(score, flush=True)
    if args.surface:
        held = torch.bincount(truth[truth >= 0].to(torch.int64), minlength=len(labels)).cpu().tolist()
        surface = {labels[k]: surface_distances(pred, truth, k, d, device=device) for k in range(len(labels)) if held[k] and labels[k]}
        for lb, s in surface.items():
            print(f"surface {lb}: hausdorff {s.hausdorff:.1f} px, hd95 {s.hd95:.1f} px, assd {s.assd:.2f} px "
                  f"({s.n_pred} predicted, {s.n_truth} annotated boundary cells)", flush=True)
    if args.distance_json:
        save_distance_report(args.distance_json, d, margin=margin, tolerant=tolerant, surface=surface)


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
    `--min_sharpness N` and `--max_ink F` leave out the out-of-focus and the ink-marked tiles among those (DESIGN.md section 4.16;
    QualityFilter; dense branch, resident slide; either switches the filter on, as does `--quality_fill`, which must name the
    class of `--tissue_fill` when both filters run); `--quality_json PATH` writes thresholds, counts and the quartiles of the
    scored tiles' sharpness (rank 0), from which to pick N.
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
    `--pyramid` makes `--layer L` of a `--synthetic` slide or a `.npy` image the slide at 1/L of its resolution (DESIGN.md section
    4.14): the exact area average, built on the device; everything below reads that layer, and `--stain` normalises it.
    `--tta flips|d4` classifies every tile in four or all eight orientations of the square and averages the logits per tile
    (both fused routes, resident slide; refused with `--ondisk` and for a foreign model on the callback
    route); overlays, scoring and regions read the untransformed slide and the map, as without it.
    `--stain macenko` normalises the slide's stain appearance first (resident slide): the prediction, the
    tissue filter and the overlays all read the normalised slide; `--stain_target PATH` takes another slide's saved fit as the
    target instead of the default constants, `--save_stain_fit PATH` writes this slide's fit (rank 0).
    `--save_embeddings PATH` writes every classified tile's pooled feature vector, origin, grid index and logits as one `.npz`
    (rank 0; `SlideEmbeddings.load`); the class map is finished from the logits of that same forward pass
    and is the map of a run without the flag, bit for bit.  `--prototypes PATH` with `--anno` fits one prototype per class on this
    slide's annotated tiles and writes them; without `--anno` it loads them and writes `{stem}_prototype_map.jpg`, the
    nearest-prototype class of every cell over the slide.  Both take the dense branch and a resident slide and are refused with
    `--random_sampler`, `--ondisk`, `--tta` and `--proba`.
    `--clusters K [--cluster_seed S] [--cluster_init kmeans++|maximin] [--save_clusters PATH]` runs k-means over the embeddings of
    the same pass (no annotation needed; the same refusals) and writes `{stem}_clusters.jpg`, the cluster of
    most covering tiles per cell in a K-colour palette over the slide, and `{stem}_clusters.json` (K, sizes, inertia, iterations,
    converged); `--load_clusters PATH` applies a saved codebook instead of fitting.  `--regions_json` / `--export_anno` then
    describe the cluster map's regions, named `cluster_0` ...; the class map and its JPEGs are those of a run without the flags.
    `--pca N [--save_pca PATH]` fits the first N principal components of the embeddings of the same pass (DESIGN.md section 4.19;
    the same refusals) and writes `{stem}_pca.jpg`, the first three components of every cell's tiles as red, green and blue, and
    `{stem}_pca.json` (N, tiles, explained variance and ratios, milliseconds of scatter, eigen-solve and projection);
    `--load_pca PATH` applies a saved basis instead of fitting.
    `--knn K --knn_bank PATH` classifies every tile by its K nearest tiles of a labelled bank (the same
    refusals): with `--anno` the bank is this slide's annotated tiles (`--knn_per_class N` keeps at most N of a class), written
    to PATH with the leave-one-out accuracy printed; without `--anno` PATH is loaded.  Either way `{stem}_knn.jpg` and
    `{stem}_knn_overlay.jpg` show the class of most neighbours per cell, and `--regions_json` / `--export_anno` describe that map.
    `--similar_to Y,X [--similar_k K] [--similar_json PATH]` writes the K tiles of this slide most like the tile under that pixel
    (origins and squared distances of the normalised embeddings, nearest first, the tile itself left out) as JSON.
    `--fine` builds the map from the class activation maps of the last conv (`predict_fine_patched`): every
    tile's S x S per-position scores, S = patch_size / 32, go onto their own 32 x 32-pixel blocks, so the map's values change
    every 32 px instead of once per tile footprint, from the same forward pass.  The canvas shape does not move: `--proba`,
    `--heat`, `--save_proba`, `--anno`, the region flags, `--tissue`, the quality flags and `--stain` compose with it.  Dense
    branch, resident slide, `--patch_size` a multiple of 32; refused with `--tta`, `--random_sampler`, `--ondisk` and the
    embedding flags.
    `--margin LABEL:PX[,PX...]` cuts the map into bands of distance around class LABEL (edges in layer
    pixels, negative inside the class, a single PX meaning `-PX,0,PX`), prints the classes per band and writes `{stem}_margin.jpg`,
    one colour per band over the slide.  With `--anno`, `--score_tolerance PX` adds a score that leaves out the cells within PX
    of a label change of the annotation and `--surface` the Hausdorff, HD95 and average symmetric surface distance of every class
    the annotation holds.  `--distance_json PATH` writes all three as one report (rank 0).  They run on the map the region flags
    describe (the cleaned one under `--min_region`) and are refused with `--clusters`; every other output is that of a run
    without them.
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
        pred, proba, smp, img, stem = _run(args, model, device, rank, world)
        if rank == 0:
            _report_rank0(args, pred, proba, smp, img, stem, device)
        if world > 1:
            dist.barrier()
        ok = True
        return pred
    finally:
        finalize(owned, ok)   # a failing rank leaves without a barrier (distributed.finalize)


if __name__ == "__main__":
    main()
