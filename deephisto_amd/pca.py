"""Principal components of tile embeddings: spectrum, projection, colour maps.

`centred_scatter` is the one heavy step, the scatter matrix of the rows about their mean on the device (`dh_embed_scatter`: n D^2
multiply-adds in a fixed chunked order, one triangle computed and mirrored); `project` is the centred projection
(`dh_embed_project`: the subtract happens before the multiply, so the large common mean of pooled ReLU features does not
cancel against `mean . component` afterwards).  `PCA` puts them together with `embeddings.class_sums` for the mean and a float64
symmetric eigen-solve of the D x D covariance on the host; `reduce` hands the projected rows on as a `SlideEmbeddings` that
`clustering.KMeans`, `cluster_map` and `PrototypeClassifier` take unchanged, `colour_map` paints three components as RGB.

Every step is bit-deterministic: the kernels have one fixed order each and the host's part is float64 NumPy on values copied
back.  After `extract_embeddings(..., gather=True)` every rank holds all rows, so every rank that fits computes the same basis
and nothing is exchanged.
"""
from __future__ import annotations

import json
import time

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .embeddings import SlideEmbeddings, _count, _rows, _stream, _vector, class_sums, normalize_rows

MAX_COMPONENTS = 64   # of dh_embed_project
_FORMAT = "deephisto_amd.PCA/1"
_TINY = float(np.finfo(np.float32).tiny)   # the least variance a whitening divides by


# ---- the two kernels ----------------------------------------------------------------------------------------------------
def centred_scatter(features: torch.Tensor, mean: torch.Tensor) -> torch.Tensor:
    """float32[D, D]: S[a][b] = sum_i t_i[a] t_i[b] with t_i = features[i] - mean in float32 (`dh_embed_scatter`).  Rows are
    cut into chunks of CHUNK_ROWS; a chunk's partial is one chain of fused multiply-adds over its rows in ascending order, the
    partials are added in ascending chunk order: the same bits on every run and every rank, S == S.T bit for bit, and all zero
    for n = 0."""
    x = _rows(features, "features")
    n, D = int(x.shape[0]), int(x.shape[1])
    size = lib().dh_embed_scatter_work_size(n, D)
    if size < 0:
        check(-22, "dh_embed_scatter_work_size")
    m = _vector(mean, D, x, "mean")
    work = torch.empty(size, dtype=torch.float32, device=x.device) if size else None
    out = torch.empty((D, D), dtype=torch.float32, device=x.device)
    check(lib().dh_embed_scatter(x.data_ptr(), n, D, m.data_ptr(), out.data_ptr(), work.data_ptr() if size else None,
                                 _stream(x.device)), "dh_embed_scatter")
    return out


def project(features: torch.Tensor, mean: torch.Tensor, components: torch.Tensor, scale: torch.Tensor | None = None,
            width: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """float32[n, width or K]: scale[j] * (features[i] - mean) . components[j] (`dh_embed_project`), each element one chain of
    fused multiply-adds of the float32 differences over the columns in ascending order: a row's result does not depend on the
    other rows of the launch.  `scale`: float32[K] on the device, or None for 1.  `width` (>= K, a multiple of 4): the columns
    behind K are zero.  `out`: a contiguous float32[n, ld] GPU tensor to write into instead (K <= ld, ld % 4 == 0); its columns
    behind K are left as they are."""
    x, c = _rows(features, "features"), _rows(components, "components")
    n, D, K = int(x.shape[0]), int(x.shape[1]), int(c.shape[0])
    if c.shape[1] != D or c.device != x.device:
        raise ValueError(f"components are {tuple(c.shape)} but the features have {D} columns (one device)")
    m = _vector(mean, D, x, "mean")
    s = None if scale is None else _vector(scale, K, x, "scale")
    if out is not None:
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n or out.device != x.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32[n, ld] GPU tensor on the features' device")
        res = buf = out
    elif width is not None:
        res = buf = torch.zeros((n, int(width)), dtype=torch.float32, device=x.device)
    else:   # the kernel's rows are a multiple of four floats long
        buf = torch.empty((n, -(-K // 4) * 4), dtype=torch.float32, device=x.device)
        res = buf if buf.shape[1] == K else None
    check(lib().dh_embed_project(x.data_ptr(), n, D, m.data_ptr(), c.data_ptr(), K, None if s is None else s.data_ptr(),
                                 buf.data_ptr(), int(buf.shape[1]), _stream(x.device)), "dh_embed_project")
    return res if res is not None else buf[:, :K].contiguous()


# ---- the host's part: pure functions, testable without a GPU ------------------------------------------------------------
def fix_signs(components) -> np.ndarray:
    """The rows of float64[K, D] `components` with the sign rule applied: the entry of largest magnitude of each row (the first
    such index at ties) is positive."""
    v = np.array(components, dtype=np.float64, copy=True).reshape(len(components), -1)
    for j in range(v.shape[0]):
        if v[j, int(np.argmax(np.abs(v[j])))] < 0:
            v[j] = -v[j]
    return v


def top_components(cov, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(float64[k] eigenvalues in descending order, float64[k, D] unit eigenvectors under the sign rule) of the symmetric
    float64[D, D] `cov`, by `numpy.linalg.eigh`."""
    lam, vec = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.argsort(-lam, kind="stable")[:int(k)]
    return lam[order], fix_signs(vec[:, order].T)


def colour_levels(mean: torch.Tensor, covered: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """uint8, the shape of `mean`: floor(255 clamp((v - lo) / (hi - lo), 0, 1) + 0.5) where `covered`, 128 there when hi == lo, and
    0 where not covered.  Works on tensors of any device."""
    if hi == lo:
        lev = torch.full_like(mean, 128.0)
    else:
        lev = torch.floor(255.0 * ((mean - float(lo)) / (float(hi) - float(lo))).clamp(0.0, 1.0) + 0.5)
    return torch.where(covered, lev, torch.zeros_like(lev)).to(torch.uint8)


# ---- PCA --------------------------------------------------------------------------------------------------------------------
class PCA:
    """Principal-component analysis of embedding rows, the same bits on every run and every rank.

    `fit`: the column mean in the fixed order of `class_sums` (every label 0; the float32 sums divided by n in float64 and
    rounded once to float32), the scatter matrix about it on the device (`centred_scatter`), the covariance S / (n - 1) in
    float64 on the host, its eigen-decomposition there (`top_components`: descending eigenvalues; the entry of largest magnitude
    of each component is positive).  `whiten`: `transform` divides component j by sqrt(explained_variance_[j]) (at least the
    least normal float32).  `normalize`: rows are divided by their norm first (into a copy), for `fit` and `transform` alike.

    After `fit`: `mean_` float32[D] and `components_` float32[K, D] on the device, `explained_variance_` and
    `explained_variance_ratio_` (against the trace of the covariance) float64[K] on the host, `n_samples_`; `timings_` holds the
    milliseconds of the scatter and the eigen-solve.

    Ranks: after `extract_embeddings(..., gather=True)` every rank holds all rows and every step above is deterministic, so
    every rank computes the same basis and nothing is exchanged; one rank's share (`gather=False`) is refused."""

    def __init__(self, n_components: int, whiten: bool = False, normalize: bool = False):
        self.n_components, self.whiten, self.normalize = _count(n_components, MAX_COMPONENTS, "n_components"), bool(whiten), bool(normalize)
        self.mean_ = self.components_ = self.explained_variance_ = self.explained_variance_ratio_ = None
        self.n_samples_ = 0
        self.timings_: dict = {}

    # -- rows ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _features(item, need_all: bool) -> torch.Tensor:
        if isinstance(item, SlideEmbeddings):
            if need_all and item.row_range is not None:
                raise ValueError("these embeddings hold one rank's rows only (gather=False, row_range): a PCA needs every rank to "
                                 "hold all rows (extract_embeddings(..., gather=True))")
            return item.features
        return item

    def _prepared(self, features, need_all: bool) -> torch.Tensor:
        """The rows to work on; `need_all`: a fit needs every row, a projection is row by row and takes one rank's share too."""
        if isinstance(features, (list, tuple)):
            if not features:
                raise ValueError("an empty list of embeddings")
            x = torch.cat([_rows(self._features(f, need_all), "features") for f in features], dim=0)
        else:
            x = _rows(self._features(features, need_all), "features")
        return normalize_rows(x) if self.normalize else x   # normalize_rows writes a new tensor: the caller's rows stay

    # -- fit / transform ------------------------------------------------------------------------------------------------
    def fit(self, features) -> "PCA":
        """`features`: float32[n, D] on the device, a SlideEmbeddings, or a list of either (rows concatenated in list order, so
        several slides share one basis).  n >= 2 and n_components <= D."""
        x = self._prepared(features, True)
        n, D, K = int(x.shape[0]), int(x.shape[1]), self.n_components
        if n < 2:
            raise ValueError(f"n = {n} rows have no covariance: a PCA needs n >= 2")
        if K > D:
            raise ValueError(f"n_components = {K} exceeds the {D} columns of the features")
        t0 = time.perf_counter()
        sums, _ = class_sums(x, torch.zeros(n, dtype=torch.int32, device=x.device), 1)
        mean = (sums[0].double() / n).to(torch.float32).contiguous()
        cov = (centred_scatter(x, mean).double() / (n - 1)).cpu().numpy()   # the copy waits for the kernels
        t1 = time.perf_counter()
        lam, vec = top_components(cov, K)
        t2 = time.perf_counter()
        self.mean_ = mean
        self.components_ = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).to(x.device)
        self.explained_variance_ = lam
        self.explained_variance_ratio_ = lam / float(np.trace(cov))
        self.n_samples_ = n
        self.timings_ = dict(scatter_ms=1e3 * (t1 - t0), eigen_ms=1e3 * (t2 - t1))
        return self

    def _scale(self, device) -> torch.Tensor | None:
        if not self.whiten:
            return None
        s = 1.0 / np.sqrt(np.maximum(np.asarray(self.explained_variance_, dtype=np.float64), _TINY))
        return torch.from_numpy(s.astype(np.float32)).to(device)

    def transform(self, features, width: int | None = None) -> torch.Tensor:
        """float32[n, width or K]: the rows of `features` (a float32[n, D] GPU tensor or a SlideEmbeddings) about `mean_` along
        `components_` (`project`), divided by the components' standard deviations with `whiten`; with a `width` (>= K, a
        multiple of 4) the remaining columns are zero."""
        if self.components_ is None:
            raise ValueError("the model has no components: fit() or load() first")
        x = self._prepared(features, False)
        if width is not None and (int(width) < self.n_components or int(width) % 4):
            raise ValueError(f"width must be a multiple of 4 and at least n_components = {self.n_components}, not {width}")
        return project(x, self.mean_.to(x.device), self.components_.to(x.device), self._scale(x.device), width)

    def reduce(self, emb: SlideEmbeddings, width: int = 64) -> SlideEmbeddings:
        """A SlideEmbeddings with the origins, tile index, logits and geometry of `emb` whose `features` are
        `transform(emb, width)`: the projection, zero-padded to `width` columns (a multiple of 64 suits the other embed kernels).
        `KMeans(..., normalize=False)`, `cluster_map` and `PrototypeClassifier(normalize=False)` take it unchanged."""
        return SlideEmbeddings(self.transform(emb, width), emb.origins, emb.tile_index, emb.logits, patch_size=emb.patch_size,
                               stride=emb.stride, h=emb.h, w=emb.w, layer=emb.layer, arch=emb.arch, compute_dtype=emb.compute_dtype,
                               n_unique=emb.n_unique, n_padded=emb.n_padded, row_range=emb.row_range)

    def colour_map(self, emb: SlideEmbeddings, downscale: int = 16, components=(0, 1, 2), clip=(1.0, 99.0)) -> torch.Tensor:
        """uint8[h // d, w // d, 3] on the device: up to three components as red, green and blue (a channel without a component
        stays 0).  Per cell the mean of a component over the tiles covering it (the projected columns and a column of ones
        accumulated over the tiles' footprints in tile order, `tiles.accumulate_logits`), mapped through
        floor(255 clamp((v - lo) / (hi - lo), 0, 1) + 0.5) with lo and hi the `clip` percentiles of the per-tile values
        (`numpy.percentile`, linear, float64, on the host); a channel with hi == lo is 128 wherever a tile covers; cells no tile
        covers are 0."""
        emb.require_all_rows()
        comps = [int(c) for c in components]
        if not 1 <= len(comps) <= 3 or any(not 0 <= c < self.n_components for c in comps):
            raise ValueError(f"components must name one to three of the {self.n_components} components, not {components!r}")
        if not 0.0 <= float(clip[0]) <= float(clip[1]) <= 100.0:
            raise ValueError(f"clip must be two ascending percentiles in [0, 100], not {clip!r}")
        dev = emb.features.device
        out = torch.zeros((emb.h // downscale, emb.w // downscale, 3), dtype=torch.uint8, device=dev)
        if len(emb) == 0:
            return out
        z = self.transform(emb)[:, comps]
        both = torch.cat([z, torch.ones((len(emb), 1), dtype=torch.float32, device=dev)], dim=1).contiguous()
        canvas, _ = tiles.accumulate_logits(both, emb.origins, emb.patch_size, downscale, emb.h, emb.w, want_map=False)
        count = canvas[..., len(comps)]
        covered = count > 0
        per_tile = z.cpu().numpy().astype(np.float64)
        for ch in range(len(comps)):
            lo, hi = (float(v) for v in np.percentile(per_tile[:, ch], [float(clip[0]), float(clip[1])]))
            out[..., ch] = colour_levels(canvas[..., ch] / count.clamp(min=1.0), covered, lo, hi)
        return out

    # -- files ----------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One `.npz`: mean, components, the spectrum and the settings as a JSON string; nothing pickled."""
        if self.components_ is None:
            raise ValueError("the model has no components to save")
        meta = dict(format=_FORMAT, n_components=self.n_components, whiten=self.whiten, normalize=self.normalize,
                    n_samples=self.n_samples_)
        with open(path, "wb") as f:
            np.savez(f, mean=self.mean_.detach().cpu().numpy(), components=self.components_.detach().cpu().numpy(),
                     explained_variance=np.asarray(self.explained_variance_, dtype=np.float64),
                     explained_variance_ratio=np.asarray(self.explained_variance_ratio_, dtype=np.float64),
                     meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path, device="cpu") -> "PCA":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"])) if "meta" in z.files else {}
            if meta.get("format") != _FORMAT:
                raise ValueError(f"{path} is not a PCA file")
            pca = cls(meta["n_components"], meta["whiten"], meta["normalize"])
            pca.mean_ = torch.from_numpy(z["mean"]).to(device)
            pca.components_ = torch.from_numpy(z["components"]).to(device)
            pca.explained_variance_ = z["explained_variance"].astype(np.float64)
            pca.explained_variance_ratio_ = z["explained_variance_ratio"].astype(np.float64)
            pca.n_samples_ = int(meta["n_samples"])
            return pca
