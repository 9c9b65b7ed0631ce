"""Unsupervised tissue maps: deterministic k-means over tile embeddings.

`nearest_centres` is the assignment step of Lloyd's algorithm on the device (`dh_embed_assign`: per row the nearest of K centres by
direct differences, the lexicographic minimum of (distance, index)); `embeddings.class_sums` is its update step.  `KMeans` puts the
two together with a k-means++ or maximin seeding, `cluster_map` paints the labels onto the map canvas in the format of the class
maps, so `regions.extract_regions` and `visualize` take the result unchanged (`cluster_description` names and colours the clusters).

Every step is bit-deterministic: the kernels have one fixed order each, the stopping rule reads integer labels only, and what the
host draws comes from a seeded generator and from distances copied back.  After `extract_embeddings(..., gather=True)` every rank
holds all rows, so every rank that fits computes the same centres and labels and nothing is exchanged.
"""
from __future__ import annotations

import colorsys
import json

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .anno.utils import AnnoDescription
from .embeddings import SlideEmbeddings, _count, _out_buffer, _rows, _stream, class_sums, normalize_rows

MAX_CLUSTERS = 64   # of dh_embed_class_sums; dh_embed_assign itself goes past it in passes (k0, merge)
INITS = ("kmeans++", "maximin")
_FORMAT = "deephisto_amd.KMeans/1"


def nearest_centres(features: torch.Tensor, centres: torch.Tensor, out_label: torch.Tensor | None = None,
                    out_dist: torch.Tensor | None = None, k0: int = 0, merge: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(int32[n] labels, float32[n] squared distances): per row of float32[n, D] `features` the nearest row of float32[K, D]
    `centres` (`dh_embed_assign`, 1 <= K <= 64).  A distance is one chain over the columns in ascending order of
    t = x - m, acc = fma(t, t, acc); the label is `k0` + the index of the smallest distance, the lower index at equal distances; a
    row with no finite distance gets (-1, +inf).  `merge`: start from the pairs already in `out_dist` / `out_label` (both
    required then) instead of (+inf, -1): centres beyond 64 in passes with rising `k0`, or one new centre per call as the seeding
    does.  A row's result does not depend on the other rows of the launch."""
    x, c = _rows(features, "features"), _rows(centres, "centres")
    if c.shape[1] != x.shape[1] or c.device != x.device:
        raise ValueError(f"centres are {tuple(c.shape)} but the features have {x.shape[1]} columns (one device)")
    n = int(x.shape[0])
    if merge and (out_label is None or out_dist is None):
        raise ValueError("merge=True starts from out_label and out_dist: both must be given")
    out_label = _out_buffer(out_label, torch.int32, (n,), x.device,
                            "out_label must be a contiguous int32[n] GPU tensor on the features' device")
    out_dist = _out_buffer(out_dist, torch.float32, (n,), x.device,
                           "out_dist must be a contiguous float32[n] GPU tensor on the features' device")
    check(lib().dh_embed_assign(x.data_ptr(), n, int(x.shape[1]), c.data_ptr(), int(c.shape[0]), int(k0), int(bool(merge)),
                                out_label.data_ptr(), out_dist.data_ptr(), _stream(x.device)), "dh_embed_assign")
    return out_label, out_dist


# ---- the host's part: pure functions, testable without a GPU ------------------------------------------------------------
def _weights(dist) -> np.ndarray:
    """float64 weights of float32 distances: what is not finite (a row of NaN has distance +inf) weighs nothing."""
    w = np.asarray(dist, dtype=np.float64).reshape(-1)
    return np.where(np.isfinite(w) & (w > 0), w, 0.0)


def draw_index(dist, u: float) -> int:
    """The row a k-means++ draw `u` in [0, 1) picks among rows of weight `dist`: float64 cumulative sums, the first row whose
    cumulative weight exceeds u * total.  A row of weight 0 is never picked; when every weight is 0 the answer is row 0."""
    w = _weights(dist)
    if len(w) == 0:
        raise ValueError("draw_index needs at least one row")
    cum = np.cumsum(w)
    total = cum[-1]
    if not total > 0:
        return 0
    i = int(np.searchsorted(cum, float(u) * total, side="right"))
    return i if i < len(w) else int(np.flatnonzero(w)[-1])   # u * total rounded up to the total: the last row that weighs anything


def farthest_index(dist) -> int:
    """The first row of the largest (finite) distance: the maximin seeding's next centre and the new home of an empty cluster."""
    return int(np.argmax(_weights(dist)))


def canonical_order(counts) -> np.ndarray:
    """int64[K]: the old cluster numbers in canonical order, by descending size and, at equal sizes, ascending old number."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    return np.lexsort((np.arange(len(c)), -c)).astype(np.int64)


def cluster_palette(n_clusters: int) -> list[tuple[int, int, int]]:
    """`n_clusters` RGB colours, the same for a cluster number whatever K is: hues a golden-ratio step apart, three brightness bands."""
    out = []
    for k in range(int(n_clusters)):
        r, g, b = colorsys.hsv_to_rgb((0.07 + 0.6180339887498949 * k) % 1.0, (0.85, 0.6, 0.95)[k % 3], (0.95, 0.75, 0.55)[(k // 3) % 3])
        out.append((int(round(255 * r)), int(round(255 * g)), int(round(255 * b))))
    return out


def cluster_description(n_clusters: int) -> AnnoDescription:
    """The AnnoDescription of a cluster map: classes `cluster_0` ... with ids 0 ... and the colours of `cluster_palette`."""
    return AnnoDescription.with_known_colors({f"cluster_{k}": c for k, c in enumerate(cluster_palette(n_clusters))})


# ---- k-means ------------------------------------------------------------------------------------------------------------
class KMeans:
    """Lloyd's k-means on the device, the same bits on every run and every rank.

    `init`: "kmeans++" (the first row from `np.random.default_rng(seed)`, each next one drawn on the host with probability
    proportional to the squared distance to the nearest centre so far, `draw_index`), "maximin" (the row nearest the mean of all
    rows, then each time the row farthest from the centres so far; `seed` is not read) or a float32[K, D] array / tensor of
    centres.  `normalize`: rows are divided by their norm first (into a copy), for `fit` and `predict` alike.

    One iteration: per-cluster sums in the fixed order of `class_sums`, centres = sums / counts, `nearest_centres` into the other
    label buffer; it ends when no label changed or after `max_iter` iterations.  An empty cluster's centre becomes the row of
    largest distance (the first maximum, whose distance then counts as 0 so that two empty clusters take different rows), in
    ascending cluster order.  Afterwards clusters are renumbered by descending size (ties: the lower old number), so numbers and
    colours do not depend on the seeding order.  `inertia_` is reported and never read back into the algorithm.

    After `fit`: `centres_` float32[K, D] and `labels_` int32[n] on the device, `counts_` int64[K] on the host, `inertia_`,
    `n_iter_`, `converged_`.  A row without a finite distance (NaN features) has label -1 and belongs to no cluster.

    Ranks: after `extract_embeddings(..., gather=True)` every rank holds all rows, every step here is bit-deterministic, so every
    rank computes the same centres and labels and nothing is exchanged; one rank's share (`gather=False`) is refused."""

    def __init__(self, n_clusters: int, init="kmeans++", seed: int = 0, max_iter: int = 50, normalize: bool = True):
        self.n_clusters = _count(n_clusters, MAX_CLUSTERS, "n_clusters")
        self._init_centres = None
        if isinstance(init, str):
            if init not in INITS:
                raise ValueError(f"init must be one of {', '.join(INITS)} or a [K, D] array of centres, not {init!r}")
        else:
            c = init.detach().to(torch.float32) if isinstance(init, torch.Tensor) else torch.from_numpy(np.array(init, dtype=np.float32))
            if c.dim() != 2 or c.shape[0] != self.n_clusters:
                raise ValueError(f"explicit initial centres must be [{self.n_clusters}, D], not {list(c.shape)}")
            self._init_centres, init = c, "explicit"
        if int(max_iter) < 0:
            raise ValueError(f"max_iter must be >= 0, not {max_iter}")
        self.init, self.seed, self.max_iter, self.normalize = init, int(seed), int(max_iter), bool(normalize)
        self.centres_ = self.labels_ = self.counts_ = None
        self.inertia_, self.n_iter_, self.converged_ = None, 0, False
        self.seed_rows_: list[int] = []   # the rows a "kmeans++" / "maximin" seeding took, in seeding order

    # -- rows ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _features(item) -> torch.Tensor:
        if isinstance(item, SlideEmbeddings):
            if item.row_range is not None:
                raise ValueError("these embeddings hold one rank's rows only (gather=False): k-means needs every rank to hold all "
                                 "rows (extract_embeddings(..., gather=True))")
            return item.features
        return item

    def _prepared(self, features) -> torch.Tensor:
        if isinstance(features, (list, tuple)):
            if not features:
                raise ValueError("an empty list of embeddings")
            x = torch.cat([_rows(self._features(f), "features") for f in features], dim=0)
        else:
            x = _rows(self._features(features), "features")
        return normalize_rows(x) if self.normalize else x   # normalize_rows writes a new tensor: the caller's rows stay

    # -- seeding --------------------------------------------------------------------------------------------------------
    def _seed(self, x, label, dist) -> torch.Tensor:
        """The K initial centres; leaves the first assignment in `label` / `dist`."""
        n, D, K = int(x.shape[0]), int(x.shape[1]), self.n_clusters
        if self._init_centres is not None:
            c = self._init_centres.to(x.device).contiguous()
            if c.shape[1] != D:
                raise ValueError(f"the initial centres have {c.shape[1]} columns, the features {D}")
            nearest_centres(x, c, label, dist)
            return c
        centres = torch.empty((K, D), dtype=torch.float32, device=x.device)
        rng = np.random.default_rng(self.seed)
        self.seed_rows_ = []
        for j in range(K):
            if j == 0 and self.init == "kmeans++":
                row = int(rng.integers(n))
            elif j == 0:
                sums, _ = class_sums(x, torch.zeros(n, dtype=torch.int32, device=x.device), 1)
                nearest_centres(x, sums / float(n), label, dist)
                d = dist.cpu().numpy()
                row = int(np.argmin(np.where(np.isfinite(d), d, np.inf)))   # the first minimum
            elif self.init == "kmeans++":
                row = draw_index(dist.cpu().numpy(), float(rng.random()))
            else:
                row = farthest_index(dist.cpu().numpy())
            self.seed_rows_.append(row)
            centres[j] = x[row]
            nearest_centres(x, centres[j:j + 1], label, dist, k0=j, merge=j > 0)
        return centres

    # -- fit / predict --------------------------------------------------------------------------------------------------
    def fit(self, features) -> "KMeans":
        """`features`: float32[n, D] on the device, a SlideEmbeddings, or a list of either (rows concatenated in list order, so
        several slides share one codebook).  n >= n_clusters."""
        x = self._prepared(features)
        n, K = int(x.shape[0]), self.n_clusters
        if n < K:
            raise ValueError(f"{n} rows cannot seed {K} clusters")
        label = [torch.empty(n, dtype=torch.int32, device=x.device) for _ in range(2)]
        dist = torch.empty(n, dtype=torch.float32, device=x.device)
        centres = self._seed(x, label[0], dist)
        cur, self.n_iter_, self.converged_ = 0, 0, False
        for _ in range(self.max_iter):
            sums, counts = class_sums(x, label[cur], K)
            cnt = counts.cpu().numpy()
            centres = sums / counts.clamp(min=1).to(torch.float32)[:, None]
            empty = np.flatnonzero(cnt == 0)
            if len(empty):
                d = dist.cpu().numpy().copy()
                for k in empty:   # ascending
                    row = farthest_index(d)
                    centres[int(k)] = x[row]
                    d[row] = 0.0
            nearest_centres(x, centres, label[1 - cur], dist)
            changed = int((label[1 - cur] != label[cur]).sum())
            cur = 1 - cur
            self.n_iter_ += 1
            if changed == 0:
                self.converged_ = True
                break
        lab = label[cur]
        cnt = torch.bincount(lab[lab >= 0].to(torch.int64), minlength=K).cpu().numpy().astype(np.int64)
        order = canonical_order(cnt)
        new_of_old = np.empty(K, dtype=np.int32)
        new_of_old[order] = np.arange(K, dtype=np.int32)
        remap = torch.from_numpy(new_of_old).to(x.device)
        self.labels_ = torch.where(lab >= 0, remap[lab.clamp(min=0).to(torch.int64)], lab).contiguous()
        self.centres_ = centres[torch.from_numpy(order).to(x.device)].contiguous()
        self.counts_ = cnt[order]
        self.inertia_ = float(dist.double().sum())
        return self

    def predict(self, features, return_dist: bool = False):
        """int32[n] on the device: the nearest of `centres_` for every row of `features` (as `fit` takes them), after the same
        normalisation; with `return_dist` also the float32[n] squared distances."""
        if self.centres_ is None:
            raise ValueError("the model has no centres: fit() or load() first")
        x = self._prepared(features)
        lab, dist = nearest_centres(x, self.centres_.to(x.device))
        return (lab, dist) if return_dist else lab

    # -- files ----------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One `.npz`: centres, counts and the settings and outcome as a JSON string; nothing pickled."""
        if self.centres_ is None:
            raise ValueError("the model has no centres to save")
        meta = dict(format=_FORMAT, n_clusters=self.n_clusters, init=self.init, seed=self.seed, max_iter=self.max_iter,
                    normalize=self.normalize, inertia=self.inertia_, n_iter=self.n_iter_, converged=self.converged_)
        with open(path, "wb") as f:
            np.savez(f, centres=self.centres_.detach().cpu().numpy(), counts=np.asarray(self.counts_, dtype=np.int64),
                     meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path, device="cpu") -> "KMeans":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            if meta.get("format") != _FORMAT:
                raise ValueError(f"{path} is not a KMeans file")
            km = cls(meta["n_clusters"], "kmeans++", meta["seed"], meta["max_iter"], meta["normalize"])
            km.init = meta["init"]
            km.centres_ = torch.from_numpy(z["centres"]).to(device)
            km.counts_ = z["counts"].astype(np.int64)
            km.inertia_, km.n_iter_, km.converged_ = meta["inertia"], int(meta["n_iter"]), bool(meta["converged"])
            return km


# ---- the map --------------------------------------------------------------------------------------------------------------
def cluster_map(emb: SlideEmbeddings, labels, n_clusters: int, downscale: int = 16, fill_class: int = -1) -> torch.Tensor:
    """int64[h // d, w // d] in the format of the class maps: per cell the cluster most of the tiles covering it belong to, the
    lowest number at equal votes.  One-hot float32 rows go over the tiles' footprints like logits (`tiles.accumulate_logits`; the
    sums are small integers, hence exact), then the first maximum.  Cells no tile of `emb` covers, and cells whose tiles all have
    label -1, get `fill_class`."""
    K = _count(n_clusters, MAX_CLUSTERS, "n_clusters")
    dev = emb.features.device
    lb = labels.to(device=dev, dtype=torch.int64) if isinstance(labels, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(dev)
    if lb.dim() != 1 or lb.shape[0] != len(emb):
        raise ValueError(f"{tuple(lb.shape)} labels for {len(emb)} tiles")
    emb.require_all_rows()
    if len(emb) == 0:
        return torch.full((emb.h // downscale, emb.w // downscale), fill_class, dtype=torch.int64, device=dev)
    if int(lb.max()) >= K:
        raise ValueError(f"a label of {int(lb.max())} among {K} clusters")
    votes = torch.zeros((len(emb), K), dtype=torch.float32, device=dev)
    rows = torch.nonzero(lb >= 0).reshape(-1)
    votes[rows, lb[rows]] = 1.0
    canvas, cmap = tiles.accumulate_logits(votes, emb.origins, emb.patch_size, downscale, emb.h, emb.w)
    emb.fill_uncovered(cmap, downscale, fill_class)
    if len(rows) != len(emb):
        cmap[canvas.sum(dim=2) == 0] = fill_class
    return cmap
