"""Tile embeddings of a whole slide and a prototype (nearest-class-mean) scorer on top of them.

`extract_embeddings(sampler, model, ...)` runs the tile plan of `predict.predict_full_patched` (`plan.py`) through the models' features entry
(`dh_resnet18_features_tiles` / `dh_resnet50_features_tiles`: the fused gather + forward with every tile's pooled feature vector,
the input of `fc`, stored as well) and returns a `SlideEmbeddings`: float32[n_kept, 512 | 2048] on the device, one exchange of
the rows under torch.distributed.  `PrototypeClassifier` turns embeddings plus a handful of labelled tiles (`tile_labels`) into a
class map or a similarity heat map without a training step, on three small deterministic kernels (`normalize_rows`,
`prototype_scores`, `class_sums`: no atomics, every row's result independent of the launch).
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .patch_samplers.full_samplers import FullImageDenseSampler
from .plan import Lanes, TileGrid, exchange_rows, finish, launch_tiles, normalised_first, plan_tiles, require_dense_resident
from .quality import QualityFilter
from .tiles import _stream
from .tissue import TissueFilter, fill_uncovered

CHUNK_ROWS = 1024   # DH_EMBED_CHUNK_ROWS: the chunking of class_sums' summation order


def _rows(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} must live in GPU memory (HIP kernels; no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{what} must be float32[n, D]")
    return t.contiguous()


def _vector(t: torch.Tensor, D: int, x: torch.Tensor, what: str) -> torch.Tensor:
    """`_rows` for one dimension: float32[D] on the device of the rows `x`."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != x.device:
        raise RuntimeError(f"{what} must live in GPU memory, on the features' device (HIP kernels; no CPU fallback)")
    if t.dtype != torch.float32 or tuple(t.shape) != (D,):
        raise ValueError(f"{what} must be float32[{D}], not {t.dtype}{list(t.shape)}")
    return t.contiguous()


def _count(value, most: int, what: str) -> int:
    """`value` as an int, a ValueError unless it lies in [1, most]."""
    if not 1 <= int(value) <= most:
        raise ValueError(f"{what} must be in [1, {most}], not {value}")
    return int(value)


def _out_buffer(t: torch.Tensor | None, dtype, shape: tuple, dev, what: str) -> torch.Tensor:
    """The output tensor a caller passed, checked (a ValueError of text `what` unless it is contiguous, of `dtype` and `shape`,
    on `dev`), or a new one when there is none."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
        raise ValueError(what)
    return t


# ---- the three kernels ---------------------------------------------------------------------------------------------
def normalize_rows(features: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """float32[n, D]: every row divided by its Euclidean norm (`dh_embed_normalize`); a row whose sum of squares is 0 stays zero.
    `out` may be `features` itself (in place)."""
    x = _rows(features, "features")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 GPU tensor of the features' shape")
    check(lib().dh_embed_normalize(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), out.data_ptr(), _stream(x.device)),
          "dh_embed_normalize")
    return out


def prototype_scores(features: torch.Tensor, prototypes: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """float32[n, K]: scale * features @ prototypes.T (`dh_embed_scores`), each element one chain of fused multiply-adds over the
    columns in ascending order: a row's scores do not depend on the other rows of the launch."""
    x, p = _rows(features, "features"), _rows(prototypes, "prototypes")
    if p.shape[1] != x.shape[1] or p.device != x.device:
        raise ValueError(f"prototypes are {tuple(p.shape)} but the features have {x.shape[1]} columns (one device)")
    out = torch.empty((int(x.shape[0]), int(p.shape[0])), dtype=torch.float32, device=x.device)
    check(lib().dh_embed_scores(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), p.data_ptr(), int(p.shape[0]), float(scale),
                                out.data_ptr(), _stream(x.device)), "dh_embed_scores")
    return out


def class_sums(features: torch.Tensor, labels: torch.Tensor, n_classes: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(float32[K, D] per-class sums, int64[K] counts) of the rows whose int32 label is in [0, K) (`dh_embed_class_sums`); other
    labels, -1 among them, are ignored.  Rows are added in chunks of CHUNK_ROWS in ascending order, then the chunk partials in
    ascending order, all in float32: the same bits on every run and every rank."""
    x = _rows(features, "features")
    lb = labels.to(device=x.device, dtype=torch.int32).contiguous() if isinstance(labels, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(x.device)
    if lb.dim() != 1 or lb.shape[0] != x.shape[0]:
        raise ValueError(f"{tuple(lb.shape)} labels for {x.shape[0]} rows")
    n, D, K = int(x.shape[0]), int(x.shape[1]), int(n_classes)
    size = lib().dh_embed_class_work_size(n, D, K)
    if size < 0:
        check(-22, "dh_embed_class_work_size")
    work = torch.empty(size, dtype=torch.float32, device=x.device)
    sums = torch.empty((K, D), dtype=torch.float32, device=x.device)
    counts = torch.empty(K, dtype=torch.int64, device=x.device)
    check(lib().dh_embed_class_sums(x.data_ptr(), lb.data_ptr(), n, D, K, sums.data_ptr(), counts.data_ptr(), work.data_ptr(),
                                    _stream(x.device)), "dh_embed_class_sums")
    return sums, counts


# ---- the embeddings of a slide ---------------------------------------------------------------------------------------
_META = ("patch_size", "stride", "h", "w", "layer", "arch", "compute_dtype", "n_unique", "n_padded")


class SlideEmbeddings:
    """The per-tile embeddings of one slide.

    `features` float32[n_kept, D] and `logits` (float32[n_kept, n_classes] or None) on the device, one row per tile that ran, in
    grid order; `origins` int32[n_kept, 2] (y, x) and `tile_index` int64[n_kept] (indices into the sampler's unique grid) on the
    host.  `patch_size`, `stride`, `h`, `w`, `layer`, `arch`, `compute_dtype` describe the run; `n_unique` / `n_padded` are the
    lengths of the sampler's unique and padded tile lists, from which the accumulation list is rebuilt.  Under `gather=False`
    the rows are this rank's share only (`row_range` = its [lo, hi) within the kept tiles)."""

    def __init__(self, features, origins, tile_index, logits=None, *, patch_size, stride, h, w, layer=1, arch="resnet18",
                 compute_dtype="f32", n_unique=None, n_padded=None, row_range=None):
        self.features, self.logits = features, logits
        self.origins = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 2)
        self.tile_index = np.ascontiguousarray(tile_index, dtype=np.int64).reshape(-1)
        if features.dim() != 2 or features.dtype != torch.float32 or len(self.origins) != features.shape[0] \
                or len(self.tile_index) != features.shape[0]:
            raise ValueError("features must be float32[n, D] with one origin and one tile index per row")
        if logits is not None and (logits.dim() != 2 or logits.shape[0] != features.shape[0]):
            raise ValueError("logits must hold one row per feature row")
        self.patch_size, self.stride, self.h, self.w, self.layer = int(patch_size), int(stride), int(h), int(w), int(layer)
        self.arch, self.compute_dtype = str(arch), str(compute_dtype)
        grid, n_u = tiles.tile_grid(self.h, self.w, self.patch_size, self.stride, 1) if n_unique is None else (None, int(n_unique))
        self.n_unique = n_u
        self.n_padded = int(n_padded) if n_padded is not None else n_u if grid is None else len(grid)
        self.row_range = None if row_range is None else (int(row_range[0]), int(row_range[1]))

    def __len__(self):
        return int(self.features.shape[0])

    @property
    def width(self) -> int:
        return int(self.features.shape[1])

    def _meta(self) -> dict:
        return {k: getattr(self, k) for k in _META} | {"row_range": self.row_range, "format": "deephisto_amd.SlideEmbeddings/1"}

    def save(self, path) -> None:
        """One `.npz`: features, origins, tile_index, logits (when held) and the metadata as a JSON string; nothing pickled."""
        arrays = dict(features=self.features.detach().cpu().numpy(), origins=self.origins, tile_index=self.tile_index,
                      meta=np.array(json.dumps(self._meta())))
        if self.logits is not None:
            arrays["logits"] = self.logits.detach().cpu().numpy()
        with open(path, "wb") as f:   # the name as given (np.savez would append .npz to a bare path)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device="cpu") -> "SlideEmbeddings":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            if meta.get("format") != "deephisto_amd.SlideEmbeddings/1":
                raise ValueError(f"{path} is not a SlideEmbeddings file")
            meta.pop("format")
            logits = torch.from_numpy(z["logits"]).to(device) if "logits" in z.files else None
            return cls(torch.from_numpy(z["features"]).to(device), z["origins"], z["tile_index"], logits, **meta)

    def require_all_rows(self) -> None:
        if self.row_range is not None:
            raise ValueError("these embeddings hold one rank's rows only (gather=False): a map needs all of them")

    def fill_uncovered(self, cmap: torch.Tensor, downscale: int, fill_class: int) -> torch.Tensor:
        """In place: the cells of int64[h // d, w // d] `cmap` no tile of these embeddings covers become `fill_class`."""
        self.require_all_rows()
        if len(self) != self.n_unique:
            fill_uncovered(cmap, torch.from_numpy(self.origins).to(cmap.device), self.patch_size, downscale, self.h, self.w, fill_class)
        return cmap

    def class_map(self, downscale: int = 16, dedupe_padding: bool = False, fill_class: int = -1) -> torch.Tensor:
        """int64[h // d, w // d]: the class map `predict_full_patched` gives for this run, bit for bit, finished from the
        stored logits by its own tail (`plan.finish`); cells no kept tile covers get `fill_class`."""
        if self.logits is None:
            raise ValueError("class_map needs the logits: extract_embeddings(..., return_logits=True)")
        self.require_all_rows()
        grid = TileGrid.from_geometry(self.h, self.w, self.patch_size, self.stride, self.n_unique, self.n_padded)
        if len(self) == self.n_unique:   # every unique tile ran: the unfiltered tail
            return finish(grid, self.logits, None, None, downscale, dedupe_padding, None, False, False)
        kept_yx_dev = torch.from_numpy(self.origins).to(self.features.device)
        return finish(grid, self.logits, self.tile_index, kept_yx_dev, downscale, dedupe_padding, fill_class, False, False)


@normalised_first
def extract_embeddings(sampler: FullImageDenseSampler, model, micro_batch: int | None = None, group=None, streams: int = 2,
                       tissue: TissueFilter | None = None, tissue_info: dict | None = None,
                       quality: QualityFilter | None = None, quality_info: dict | None = None,
                       return_logits: bool = False, gather: bool = True, *, tta=None) -> SlideEmbeddings:
    """The pooled feature vector of every tile `predict_full_patched` would classify, from the same plan (`plan.plan_tiles`;
    `tissue=`, `quality=` and their info dicts as there), each launch through the model's features entry.
    `gather=True`: one `exchange_logits` of the feature rows (and a second for the logits with `return_logits`), after which
    every rank holds all rows in tile order; `gather=False`: each rank keeps its own rows (`row_range`).
    Keyword-only `stain=` / `stain_info=`: see `plan.normalised_first`, which wraps this function.
    Refused with a ValueError: a streamed (ONDISK_MULTIPROC) sampler, any sampler but the dense one, and `tta=`."""
    if tta is not None:
        raise ValueError("extract_embeddings has no test-time augmentation (an average of embeddings over views is out of scope)")
    require_dense_resident(sampler, "extract_embeddings")
    if not hasattr(model, "features_entry"):
        raise ValueError("extract_embeddings needs a ResNet18HIP or ResNet50HIP model")
    plan = plan_tiles(sampler, model, micro_batch, group, tissue, tissue_info, quality, quality_info)
    slide, P, o_dev, grid = sampler.data_device, sampler.patch_size, plan.o_dev, plan.grid
    n, D = plan.hi - plan.lo, model.feature_width
    feat = torch.zeros((plan.per_rank, D), dtype=torch.float32, device=slide.device)
    logits = torch.zeros((plan.per_rank, model.n_classes), dtype=torch.float32, device=slide.device) if return_logits else None
    entry = model.features_entry()
    Lanes(model, streams, slide.device).run(n, plan.mb, lambda handle, stream, s, e: launch_tiles(
        entry, handle, slide, sampler.h, sampler.w, o_dev, s, e, P, logits, stream, feat=feat))
    tile_index = np.arange(grid.n_unique, dtype=np.int64) if plan.kept is None else plan.kept
    yx = grid.origins[:grid.n_unique][tile_index]
    row_range = None
    if gather:
        feat = exchange_rows(plan, feat, group)
        logits = exchange_rows(plan, logits, group) if return_logits else None
    else:
        feat, logits = feat[:n], logits[:n] if return_logits else None
        tile_index, yx = tile_index[plan.lo:plan.hi], yx[plan.lo:plan.hi]
        row_range = (plan.lo, plan.hi) if plan.world > 1 else None
    return SlideEmbeddings(feat, yx, tile_index, logits, patch_size=P, stride=sampler.stride, h=sampler.h, w=sampler.w,
                           layer=sampler.layer, arch="resnet50" if D == 2048 else "resnet18",
                           compute_dtype=model.compute_dtype, n_unique=grid.n_unique, n_padded=len(grid.origins), row_range=row_range)


def tile_labels(emb: SlideEmbeddings, truth_map, downscale: int) -> np.ndarray:
    """int32[n_kept]: the value of the int32[h // d, w // d] label map `truth_map` (what `scoring.rasterize_annotation` returns;
    -1: unlabelled) at the cell under each tile's centre pixel (y + P // 2, x + P // 2); -1 where that cell lies past the map."""
    t = truth_map.detach().cpu().numpy() if isinstance(truth_map, torch.Tensor) else np.asarray(truth_map)
    if t.ndim != 2 or t.shape != (emb.h // downscale, emb.w // downscale):
        raise ValueError(f"truth_map must be [h // d, w // d] = {(emb.h // downscale, emb.w // downscale)}, not {t.shape}")
    cy = (emb.origins[:, 0].astype(np.int64) + emb.patch_size // 2) // downscale
    cx = (emb.origins[:, 1].astype(np.int64) + emb.patch_size // 2) // downscale
    inside = (cy < t.shape[0]) & (cx < t.shape[1])
    out = np.full(len(emb.origins), -1, dtype=np.int32)
    out[inside] = t[cy[inside], cx[inside]].astype(np.int32)
    return out


class PrototypeClassifier:
    """Nearest-class-mean scoring of embeddings: one prototype per class, the (normalised) mean of the (normalised) features of
    that class's labelled tiles; a tile's score for a class is `scale` times their dot product (the cosine when `normalize`).

    `fit` leaves `prototypes` float32[K, D] on the features' device, `counts` int64[K] on the host and `empty_classes`, the ids
    without a labelled tile (their prototype is zero, their score 0)."""

    def __init__(self, n_classes: int, normalize: bool = True, scale: float = 1.0):
        self.n_classes, self.normalize, self.scale = _count(n_classes, 64, "n_classes"), bool(normalize), float(scale)
        self.prototypes = None
        self.counts = None
        self.empty_classes: list[int] = []

    def _prepared(self, features):
        features = features.features if isinstance(features, SlideEmbeddings) else features
        return normalize_rows(features) if self.normalize else _rows(features, "features")

    def fit(self, features, labels) -> "PrototypeClassifier":
        """`features` float32[n, D] (or a SlideEmbeddings), `labels` int32[n] with -1 (or anything outside [0, K)) for
        unlabelled tiles: normalise, per-class sums in the fixed order of `class_sums`, divide by the counts, normalise again."""
        x = self._prepared(features)
        sums, counts = class_sums(x, labels, self.n_classes)
        self.counts = counts.cpu().numpy()
        self.empty_classes = [int(k) for k in np.nonzero(self.counts == 0)[0]]
        mean = sums / counts.clamp(min=1).to(torch.float32)[:, None]
        self.prototypes = normalize_rows(mean) if self.normalize else mean.contiguous()
        return self

    def scores(self, features) -> torch.Tensor:
        """float32[n, K] scores of float32[n, D] features (or a SlideEmbeddings)."""
        if self.prototypes is None:
            raise ValueError("the classifier has no prototypes: fit() or load() first")
        x = self._prepared(features)
        return prototype_scores(x, self.prototypes.to(x.device), self.scale)

    def predict_map(self, emb: SlideEmbeddings, downscale: int = 16, fill_class: int = -1) -> torch.Tensor:
        """int64[h // d, w // d] class map: the score rows accumulated over the tiles' footprints in tile order, like logits
        (`tiles.accumulate_logits`), then the first maximum per cell; cells no tile of `emb` covers get `fill_class`."""
        sc = self.scores(emb.features)
        emb.require_all_rows()
        if len(emb) == 0:
            return torch.full((emb.h // downscale, emb.w // downscale), fill_class, dtype=torch.int64, device=sc.device)
        _, cmap = tiles.accumulate_logits(sc, emb.origins, emb.patch_size, downscale, emb.h, emb.w)
        return emb.fill_uncovered(cmap, downscale, fill_class)

    def similarity(self, emb: SlideEmbeddings, query_rows, downscale: int = 16) -> torch.Tensor:
        """float32[h // d, w // d] in [0, 1], ready for `tiles.heatmap_blend`: per cell, the mean over the tiles covering it of
        the cosine between a tile's embedding and the mean embedding of the tiles `query_rows` (row indices into `emb`),
        negative cosines clamped to 0; 0 where no tile covers the cell.  Needs no fit."""
        q = torch.as_tensor(np.asarray(query_rows, dtype=np.int64).reshape(-1), device=emb.features.device)
        if len(q) == 0 or int(q.min()) < 0 or int(q.max()) >= len(emb):
            raise ValueError("query_rows must name at least one row of the embeddings")
        x = normalize_rows(emb.features)
        lb = torch.full((len(emb),), -1, dtype=torch.int32, device=x.device)
        lb[q] = 0
        sums, _ = class_sums(x, lb, 1)
        cos = prototype_scores(x, normalize_rows(sums), 1.0).clamp_(0.0, 1.0)
        both = torch.cat([cos, torch.ones_like(cos)], dim=1).contiguous()
        canvas, _ = tiles.accumulate_logits(both, emb.origins, emb.patch_size, downscale, emb.h, emb.w, want_map=False)
        return torch.where(canvas[..., 1] > 0, canvas[..., 0] / canvas[..., 1].clamp(min=1.0), torch.zeros_like(canvas[..., 0])).contiguous()

    def save(self, path) -> None:
        """One `.npz`: prototypes, counts and the settings as a JSON string; nothing pickled."""
        if self.prototypes is None:
            raise ValueError("the classifier has no prototypes to save")
        meta = dict(format="deephisto_amd.PrototypeClassifier/1", n_classes=self.n_classes, normalize=self.normalize, scale=self.scale,
                    empty_classes=self.empty_classes)
        with open(path, "wb") as f:
            np.savez(f, prototypes=self.prototypes.detach().cpu().numpy(), counts=np.asarray(self.counts, dtype=np.int64),
                     meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path, device="cpu") -> "PrototypeClassifier":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            if meta.get("format") != "deephisto_amd.PrototypeClassifier/1":
                raise ValueError(f"{path} is not a PrototypeClassifier file")
            pc = cls(meta["n_classes"], meta["normalize"], meta["scale"])
            pc.prototypes = torch.from_numpy(z["prototypes"]).to(device)
            pc.counts = z["counts"].astype(np.int64)
            pc.empty_classes = [int(k) for k in meta["empty_classes"]]
            return pc
