"""Nearest neighbours of tile embeddings: exact device top-k, a k-NN classifier and tile retrieval.

`nearest_rows` is the primitive (`dh_embed_knn`): for every query row the k nearest rows of a bank, by the direct differences of
`dh_embed_assign`, the k smallest pairs under the lexicographic order (distance, index).  The order is total, so the answer is one
list whatever the launch looks like, and a bank may go through in passes (`m0`, `merge`) with the bits of the single call.
`KNNClassifier` is a vote over the neighbours' labels (`dh_embed_knn_votes`: integer counts, the nearer neighbour ahead at equal
counts); `leave_one_out` is the same call over the bank itself with the own row dropped (`drop_self`).  `similar_tiles` is
retrieval: the tiles of this slide, or of another, that look most like one tile.

Everything is bit-deterministic (no atomics, one arithmetic order), so after `extract_embeddings(..., gather=True)` every rank
computes the same neighbours and nothing is exchanged; one rank's share (`gather=False`) is refused.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import tiles
from ._lib import check, lib
from .embeddings import SlideEmbeddings, _count, _out_buffer, _rows, _stream, normalize_rows

MAX_K = 64   # of dh_embed_knn
_FORMAT = "deephisto_amd.KNNClassifier/1"


def nearest_rows(queries: torch.Tensor, bank: torch.Tensor, k: int, out_index: torch.Tensor | None = None,
                 out_dist: torch.Tensor | None = None, m0: int = 0, merge: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(int32[n, k] indices, float32[n, k] squared distances): per row of float32[n, D] `queries` the `k` nearest rows of
    float32[m, D] `bank` (`dh_embed_knn`, 1 <= k <= 64), nearest first.  A distance is one chain over the columns in ascending
    order of t = q - b, acc = fma(t, t, acc); a row holds the k smallest pairs (distance, `m0` + bank row), the lower index first
    at equal distances; a NaN distance never enters, and where fewer than k rows have a finite distance the tail is (-1, +inf).
    `merge`: the lists already in `out_index` / `out_dist` (both required then) count as candidates too: a bank in several
    tensors goes through in passes with rising `m0` and gives the bits of one call.  A row's result does not depend on the other
    rows of the launch."""
    q, b = _rows(queries, "queries"), _rows(bank, "bank")
    if b.shape[1] != q.shape[1] or b.device != q.device:
        raise ValueError(f"the bank is {tuple(b.shape)} but the queries have {q.shape[1]} columns (one device)")
    n, k = int(q.shape[0]), _count(k, MAX_K, "k")
    if merge and (out_index is None or out_dist is None):
        raise ValueError("merge=True starts from out_index and out_dist: both must be given")
    out_index = _out_buffer(out_index, torch.int32, (n, k), q.device,
                            "out_index must be a contiguous int32[n, k] GPU tensor on the queries' device")
    out_dist = _out_buffer(out_dist, torch.float32, (n, k), q.device,
                           "out_dist must be a contiguous float32[n, k] GPU tensor on the queries' device")
    check(lib().dh_embed_knn(q.data_ptr(), n, b.data_ptr(), int(b.shape[0]), int(q.shape[1]), k, int(m0), int(bool(merge)),
                             out_index.data_ptr(), out_dist.data_ptr(), _stream(q.device)), "dh_embed_knn")
    return out_index, out_dist


def neighbour_votes(index: torch.Tensor, bank_labels: torch.Tensor, n_classes: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(int32[n, C] votes, int32[n] labels) of int32[n, k] neighbour lists over int32[m] `bank_labels` (`dh_embed_knn_votes`): one
    vote per neighbour; an index of -1 or outside [0, m) and a label outside [0, C) cast none.  The label is the class with the
    most votes, at equal votes the one whose first member comes earliest in the list, -1 when nobody voted."""
    if not isinstance(index, torch.Tensor) or not index.is_cuda or index.dtype != torch.int32 or index.dim() != 2:
        raise ValueError("index must be an int32[n, k] GPU tensor")
    idx = index.contiguous()
    lb = bank_labels.to(device=idx.device, dtype=torch.int32).contiguous()
    if lb.dim() != 1:
        raise ValueError("bank_labels must be int32[m]")
    n, k, C = int(idx.shape[0]), int(idx.shape[1]), int(n_classes)
    votes = torch.empty((n, C), dtype=torch.int32, device=idx.device)
    label = torch.empty(n, dtype=torch.int32, device=idx.device)
    check(lib().dh_embed_knn_votes(idx.data_ptr(), n, k, lb.data_ptr(), int(lb.shape[0]), C, votes.data_ptr(), label.data_ptr(),
                                   _stream(idx.device)), "dh_embed_knn_votes")
    return votes, label


def drop_self(index, dist, own):
    """(index[:, :-1], dist[:, :-1]) with one entry removed per row: the one whose index equals `own[i]`, if the row holds it,
    otherwise the last; the stored order is kept.  This is how leave-one-out and "similar to this tile" leave the tile itself
    out of a list of k + 1: with duplicate rows the own index need not come first, so indices are compared, not positions.
    Tensors or arrays, [n, k + 1] each and [n] `own`; the result is of the kind that came in."""
    if isinstance(index, torch.Tensor):
        own_t = torch.as_tensor(own, device=index.device).reshape(-1).to(index.dtype)
        n, K = index.shape
        if dist.shape != index.shape or own_t.shape[0] != n or K < 1:
            raise ValueError(f"index {tuple(index.shape)}, dist {tuple(dist.shape)} and own {tuple(own_t.shape)} do not fit")
        hit = index == own_t[:, None]
        pos = torch.where(hit.any(dim=1), hit.to(torch.int8).argmax(dim=1), torch.full((n,), K - 1, device=index.device))
        keep = torch.arange(K, device=index.device)[None, :] != pos[:, None]
        return index[keep].reshape(n, K - 1), dist[keep].reshape(n, K - 1)
    index, dist, own = np.asarray(index), np.asarray(dist), np.asarray(own).reshape(-1)
    n, K = index.shape
    if dist.shape != index.shape or own.shape[0] != n or K < 1:
        raise ValueError(f"index {index.shape}, dist {dist.shape} and own {own.shape} do not fit")
    hit = index == own[:, None]
    pos = np.where(hit.any(axis=1), hit.argmax(axis=1), K - 1)
    keep = np.arange(K)[None, :] != pos[:, None]
    return index[keep].reshape(n, K - 1), dist[keep].reshape(n, K - 1)


def cap_per_class(labels, n_classes: int, cap: int) -> np.ndarray:
    """int32[n]: `labels` with every class cut down to at most `cap` tiles: of a class with `count` labelled tiles, every
    ceil(count / cap)-th one in tile order stays (the first among them), the others become -1.  No draw: the same tiles every run."""
    if int(cap) < 1:
        raise ValueError(f"the cap per class must be >= 1, not {cap}")
    lb = np.array(labels, dtype=np.int32).reshape(-1)
    for c in range(int(n_classes)):
        rows = np.flatnonzero(lb == c)
        step = -(-len(rows) // int(cap))
        if step > 1:
            drop = np.ones(len(rows), dtype=bool)
            drop[::step] = False
            lb[rows[drop]] = -1
    return lb


def _all_rows(item, who: str) -> torch.Tensor:
    if isinstance(item, SlideEmbeddings):
        if item.row_range is not None:
            raise ValueError(f"these embeddings hold one rank's rows only (gather=False): {who} needs every rank to hold all rows "
                             "(extract_embeddings(..., gather=True))")
        return item.features
    return item


class KNNClassifier:
    """k-nearest-neighbour classification of embeddings against a bank of labelled tiles: a class may be several blobs, which one
    mean per class (`PrototypeClassifier`) cannot describe.

    `fit` keeps the labelled rows as `bank` float32[m, D] and their `labels` int32[m] on the features' device and `counts`
    int64[C] on the host.  A row's class is the one most of its `k` nearest bank rows have; at equal votes the class of the
    nearer neighbour.  `normalize`: rows are divided by their norm first (into a copy), for the bank and the queries alike."""

    def __init__(self, n_classes: int, k: int = 5, normalize: bool = True):
        if not 1 <= int(n_classes) <= 64:
            raise ValueError(f"n_classes must be in [1, 64], not {n_classes}")
        self.n_classes, self.k, self.normalize = int(n_classes), _count(k, MAX_K, "k"), bool(normalize)
        self.bank = self.labels = self.counts = None

    def _prepared(self, features) -> torch.Tensor:
        if isinstance(features, (list, tuple)):
            if not features:
                raise ValueError("an empty list of embeddings")
            x = torch.cat([_rows(_all_rows(f, "a k-NN bank"), "features") for f in features], dim=0)
        else:
            x = _rows(_all_rows(features, "a k-NN bank"), "features")
        return normalize_rows(x) if self.normalize else x   # normalize_rows writes a new tensor: the caller's rows stay

    def _fitted(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        if self.bank is None:
            raise ValueError("the classifier has no bank: fit() or load() first")
        if self.bank.shape[1] != x.shape[1]:
            raise ValueError(f"the bank has {self.bank.shape[1]} columns, the features {x.shape[1]}")
        return self.bank.to(x.device), self.labels.to(x.device)

    def fit(self, features, labels) -> "KNNClassifier":
        """`features`: float32[n, D] on the device, a SlideEmbeddings, or a list of either (rows concatenated in list order);
        `labels`: int32[n] (or a list of them, concatenated alike) with -1, or anything outside [0, C), for unlabelled tiles,
        which do not enter the bank."""
        x = self._prepared(features)
        if isinstance(labels, (list, tuple)) and len(labels) and not np.isscalar(labels[0]):
            labels = np.concatenate([lb.detach().cpu().numpy() if isinstance(lb, torch.Tensor) else np.asarray(lb) for lb in labels])
        lb = labels.to(device=x.device, dtype=torch.int32) if isinstance(labels, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(x.device)
        if lb.dim() != 1 or lb.shape[0] != x.shape[0]:
            raise ValueError(f"{tuple(lb.shape)} labels for {x.shape[0]} rows")
        rows = torch.nonzero((lb >= 0) & (lb < self.n_classes)).reshape(-1)
        self.bank, self.labels = x[rows].contiguous(), lb[rows].contiguous()
        self.counts = torch.bincount(self.labels.to(torch.int64), minlength=self.n_classes).cpu().numpy().astype(np.int64)
        return self

    def neighbours(self, features) -> tuple[torch.Tensor, torch.Tensor]:
        """(int32[n, k] bank rows, float32[n, k] squared distances), nearest first (`nearest_rows`)."""
        x = self._prepared(features)
        bank, _ = self._fitted(x)
        return nearest_rows(x, bank, self.k)

    def _votes(self, features) -> tuple[torch.Tensor, torch.Tensor]:
        x = self._prepared(features)
        bank, labels = self._fitted(x)
        index, _ = nearest_rows(x, bank, self.k)
        return neighbour_votes(index, labels, self.n_classes)

    def votes(self, features) -> torch.Tensor:
        """int32[n, C]: how many of each row's k neighbours have each class."""
        return self._votes(features)[0]

    def predict(self, features) -> torch.Tensor:
        """int32[n]: the class of most neighbours, the nearer neighbour's at equal votes; -1 for a row without a neighbour."""
        return self._votes(features)[1]

    def predict_map(self, emb: SlideEmbeddings, downscale: int = 16, fill_class: int = -1) -> torch.Tensor:
        """int64[h // d, w // d] class map: the vote rows (as float32: small integers, exact) accumulated over the tiles'
        footprints in tile order, like logits (`tiles.accumulate_logits`), then the first maximum per cell.  Cells no tile of
        `emb` covers, and cells none of whose tiles has a neighbour, get `fill_class`."""
        votes, label = self._votes(emb)
        emb.require_all_rows()
        if len(emb) == 0:
            return torch.full((emb.h // downscale, emb.w // downscale), fill_class, dtype=torch.int64, device=votes.device)
        canvas, cmap = tiles.accumulate_logits(votes.to(torch.float32).contiguous(), emb.origins, emb.patch_size, downscale, emb.h, emb.w)
        emb.fill_uncovered(cmap, downscale, fill_class)
        if bool((label < 0).any()):
            cmap[canvas.sum(dim=2) == 0] = fill_class
        return cmap

    def leave_one_out(self) -> tuple[float, np.ndarray]:
        """(accuracy, int64[C, C] confusion with the bank's label along the first axis) of classifying every bank row by its k
        nearest OTHER bank rows: k + 1 neighbours with the own row dropped (`drop_self`).  A row nobody votes for counts as
        wrong and stays out of the confusion matrix."""
        if self.bank is None or len(self.bank) == 0:
            raise ValueError("leave_one_out needs a fitted bank with at least one row")
        k1 = _count(self.k + 1, MAX_K, "k")   # k <= 63 here
        m = int(self.bank.shape[0])
        index, dist = nearest_rows(self.bank, self.bank, k1)
        index, _ = drop_self(index, dist, torch.arange(m, dtype=torch.int32, device=index.device))
        _, pred = neighbour_votes(index.contiguous(), self.labels, self.n_classes)
        truth, pred = self.labels.cpu().numpy().astype(np.int64), pred.cpu().numpy().astype(np.int64)
        confusion = np.zeros((self.n_classes, self.n_classes), dtype=np.int64)
        voted = pred >= 0
        np.add.at(confusion, (truth[voted], pred[voted]), 1)
        return float(np.count_nonzero(truth == pred)) / m, confusion

    # -- files ----------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One `.npz`: bank, labels, counts and the settings as a JSON string; nothing pickled."""
        if self.bank is None:
            raise ValueError("the classifier has no bank to save")
        meta = dict(format=_FORMAT, n_classes=self.n_classes, k=self.k, normalize=self.normalize)
        with open(path, "wb") as f:
            np.savez(f, bank=self.bank.detach().cpu().numpy(), labels=self.labels.detach().cpu().numpy().astype(np.int32),
                     counts=np.asarray(self.counts, dtype=np.int64), meta=np.array(json.dumps(meta)))

    @classmethod
    def load(cls, path, device="cpu") -> "KNNClassifier":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            if meta.get("format") != _FORMAT:
                raise ValueError(f"{path} is not a KNNClassifier file")
            knn = cls(meta["n_classes"], meta["k"], meta["normalize"])
            knn.bank = torch.from_numpy(z["bank"]).to(device)
            knn.labels = torch.from_numpy(z["labels"].astype(np.int32)).to(device)
            knn.counts = z["counts"].astype(np.int64)
            if knn.bank.dim() != 2 or knn.labels.shape != (knn.bank.shape[0],) or knn.counts.shape != (knn.n_classes,):
                raise ValueError(f"{path}: bank, labels and counts do not fit each other")
            return knn


def tile_at(emb: SlideEmbeddings, query) -> int:
    """The row of `emb` a query names: a row index, or a pixel (y, x) resolved to the first tile whose footprint contains it."""
    if np.ndim(query) == 0:
        row = int(query)
        if not 0 <= row < len(emb):
            raise ValueError(f"row {row} is not one of the {len(emb)} tiles")
        return row
    y, x = (int(v) for v in query)
    o, P = emb.origins.astype(np.int64), emb.patch_size
    hit = np.flatnonzero((o[:, 0] <= y) & (y < o[:, 0] + P) & (o[:, 1] <= x) & (x < o[:, 1] + P))
    if not len(hit):
        raise ValueError(f"no tile of these embeddings covers pixel ({y}, {x})")
    return int(hit[0])


def similar_tiles(emb: SlideEmbeddings, query, k: int = 16, bank: SlideEmbeddings | None = None, exclude_self: bool = True) -> dict:
    """The `k` tiles most like one tile of `emb`, nearest first: a dict of `rows` (int32[k], rows of the bank), `origins`
    (int32[k, 2], their (y, x)) and `dist` (float32[k], squared distances of the normalised rows), with `query_row` and
    `query_origin` beside them.  `query`: a row index, or a pixel (y, x) (`tile_at`).  `bank`: another slide's embeddings for a
    search across slides; by default `emb` itself, and then `exclude_self` leaves the query tile out (k + 1 neighbours,
    `drop_self`; k <= 63).  Where the bank has fewer than k rows to offer, the lists are that much shorter."""
    own_bank = bank is None
    src = emb if own_bank else bank
    x, b = _all_rows(emb, "retrieval"), _all_rows(src, "retrieval")
    if src.width != emb.width:
        raise ValueError(f"the bank's rows have {src.width} columns, the query's {emb.width}")
    drop = bool(exclude_self) and own_bank
    k = _count(k, MAX_K - 1 if drop else MAX_K, "k")
    row = tile_at(emb, query)
    xn = normalize_rows(x)
    bn = xn if own_bank else normalize_rows(b.to(xn.device))
    index, dist = nearest_rows(xn[row:row + 1], bn, k + 1 if drop else k)
    if drop:
        index, dist = drop_self(index, dist, [row])
    rows, dist = index[0].cpu().numpy().astype(np.int32), dist[0].cpu().numpy().astype(np.float32)
    rows, dist = rows[rows >= 0], dist[rows >= 0]
    return dict(rows=rows, origins=src.origins[rows].astype(np.int32), dist=dist, query_row=row,
                query_origin=emb.origins[row].astype(np.int32))
