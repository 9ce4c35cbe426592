"""Clustering from the embeddings, on the device: k-means, and how good a partition is on the graph.

    km = VertexClustering(g, dim=128, k=17, normalize=True)      # spherical k-means for SGNS tables
    row = km.fit(sg.emb_in)                    # {"inertia", "iterations", "converged", "counts", "history"}
    q = modularity(g, km.labels, k=17)         # on the graph as it is in HBM now
    row = km.fit(sg.emb_in, init=km.centroids) # after an edge batch and a re-train: a warm start
    row = evaluate_clustering(g, sg.emb_in, ids, y)     # {"nmi", "modularity", "inertia", "iterations"}

The table is read where it lies by the HIP kernels behind wharf_kmeans_* (no count x k distance
matrix, no float atomics: the same inputs give the same bits); wharf_partition_stats reads the
handle's current graph.  Seeding is host plumbing.  Semantics: DESIGN.md §13.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


class VertexClustering:
    """Lloyd's k-means over rows of an embedding table that stays where it is.

    g: a WharfMH handle on the table's GPU (an empty one will do).  normalize: every row takes part
    divided by its norm (k-means on the unit sphere), through a buffer of reciprocal norms that
    fit / predict refresh from the table; the table itself is never copied.
    centroids: float32 [k, dim] on the GPU; labels: int32 [count] on the GPU after fit."""

    def __init__(self, g, dim: int, k: int, normalize: bool = False):
        import torch

        self.g, self.dim, self.k, self.normalize = g, int(dim), int(k), bool(normalize)
        self.device = torch.device("cuda", g.device)
        self.centroids = torch.zeros(self.k, self.dim, dtype=torch.float32, device=self.device)
        self.labels = None
        self.rnorm = None

    # -- arguments --------------------------------------------------------------------------
    def _params(self) -> L.wharf_kmeans_params:
        p = L.wharf_kmeans_params()
        p.dim, p.k, p.flags, p.reserved = self.dim, self.k, 0, 0
        return p

    def _list(self, a):
        """None, or a u32 list on the GPU: numpy / sequence (copied), or a contiguous 32-bit device tensor."""
        import torch

        if a is None:
            return None
        if getattr(a, "is_cuda", False):
            if a.dtype not in (torch.int32, torch.uint32) or not a.is_contiguous() or a.device != self.device:
                raise ValueError(f"device vertices must be a contiguous 32-bit tensor on {self.device}")
            return a.reshape(-1)
        host = np.ascontiguousarray(np.asarray(a), dtype=np.uint32).reshape(-1)
        return torch.from_numpy(host.view(np.int32)).to(self.device)

    def _table(self, emb):
        import torch

        if (emb.dtype != torch.float32 or emb.dim() != 2 or emb.shape[1] != self.dim or not emb.is_contiguous()
                or emb.device != self.device):
            raise ValueError(f"emb must be a contiguous float32 [n, {self.dim}] tensor on {self.device}")
        return emb.shape[0]

    def _sync(self) -> None:
        # the library runs on the handle's own stream: torch's pending work on its inputs first
        import torch
        torch.cuda.synchronize(self.device)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _refresh(self, emb, n: int) -> None:
        import torch

        if not self.normalize:
            self.rnorm = None
            return
        if self.rnorm is None or self.rnorm.numel() != n:
            self.rnorm = torch.empty(n, dtype=torch.float32, device=self.device)
        self._sync()
        L.check(L.lib.wharf_emb_row_norms(self.g._h, self._p(emb), n, self.dim, self._p(self.rnorm)), self.g._h,
                "emb_row_norms")

    # -- kernels ----------------------------------------------------------------------------
    def assign(self, emb, vids=None, want_score: bool = False):
        """(labels int32 [count] on the GPU, scores float32 [count] or None, inertia) for the centroids as
        they are; vids: a device list from _list, or None for every row."""
        import torch

        n = self._table(emb)
        count = n if vids is None else vids.numel()
        labels = torch.empty(count, dtype=torch.int32, device=self.device)
        scores = torch.empty(count, dtype=torch.float32, device=self.device) if want_score else None
        inertia = C.c_double(0.0)
        p = self._params()
        self._sync()
        L.check(L.lib.wharf_kmeans_assign(self.g._h, C.byref(p), self._p(emb), n, self._p(self.rnorm), self._p(vids),
                                          count, self._p(self.centroids), self._p(labels), self._p(scores),
                                          C.byref(inertia)), self.g._h, "kmeans_assign")
        return labels, scores, float(inertia.value)

    def update(self, emb, labels, vids=None) -> np.ndarray:
        """Move every centroid to the mean of its rows (in place); the clusters' sizes, uint64 [k]."""
        n = self._table(emb)
        count = n if vids is None else vids.numel()
        counts = np.zeros(self.k, dtype=np.uint64)
        p = self._params()
        self._sync()
        L.check(L.lib.wharf_kmeans_update(self.g._h, C.byref(p), self._p(emb), n, self._p(self.rnorm), self._p(vids),
                                          count, self._p(labels), self._p(self.centroids),
                                          counts.ctypes.data_as(C.c_void_p)), self.g._h, "kmeans_update")
        return counts

    # -- seeding (host) ---------------------------------------------------------------------
    def _rows(self, emb, vids, pos: np.ndarray) -> np.ndarray:
        """The listed rows at the positions pos as float64 on the host, normalised when the model is."""
        import torch

        idx = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int64)).to(self.device)
        if vids is not None:
            idx = vids[idx].to(torch.int64) & 0xFFFFFFFF
        rows = emb[idx]
        if self.normalize:
            rows = rows * self.rnorm[idx][:, None]
        return rows.cpu().numpy().astype(np.float64)

    def _seed(self, emb, vids, count: int, init: str, seed: int) -> np.ndarray:
        if count < self.k:
            raise ValueError(f"{count} rows cannot seed {self.k} centroids")
        rng = np.random.default_rng(seed)
        if init == "sample":
            return self._rows(emb, vids, rng.choice(count, self.k, replace=False))
        if init != "kmeans++":
            raise ValueError('init must be "kmeans++", "sample" or an array of centroids')
        m = min(count, 64 * self.k)
        x = self._rows(emb, vids, rng.choice(count, m, replace=False))
        chosen = np.zeros(m, dtype=bool)
        first = int(rng.integers(m))
        chosen[first] = True
        picks = [first]
        d2 = ((x - x[first]) ** 2).sum(axis=1)
        for _ in range(1, self.k):
            d2[chosen] = 0.0
            total = d2.sum()
            if total > 0:
                nxt = int(min(np.searchsorted(np.cumsum(d2), rng.random() * total, side="right"), m - 1))
                if chosen[nxt] or d2[nxt] == 0:      # the draw fell on a boundary: the farthest row
                    nxt = int(np.argmax(d2))
            else:                                   # every row coincides with a centroid: uniform among the rest
                nxt = int(rng.choice(np.flatnonzero(~chosen)))
            chosen[nxt] = True
            picks.append(nxt)
            d2 = np.minimum(d2, ((x - x[nxt]) ** 2).sum(axis=1))
        return x[picks]

    # -- the model --------------------------------------------------------------------------
    def fit(self, emb, vertices=None, init="kmeans++", seed: int = 0, max_iter: int = 100) -> dict:
        """Lloyd's iterations, assign then update, until an assign pass changes no label or max_iter
        updates are done.  init: "kmeans++", "sample", or [k, dim] centroids (a warm start).  Returns
        {"inertia", "iterations" (updates done), "converged", "counts", "history" (the inertia of every
        assign pass)}; labels and inertia belong to the centroids as they are left."""
        import torch

        n = self._table(emb)
        vids = self._list(vertices)
        count = n if vids is None else vids.numel()
        if count < 1:
            raise ValueError("fit needs at least one row")
        self._refresh(emb, n)
        if isinstance(init, str):
            start = self._seed(emb, vids, count, init, seed)
        else:
            start = _host(init)
            if start.shape != (self.k, self.dim):
                raise ValueError(f"init centroids must have the shape [{self.k}, {self.dim}]")
        self.centroids = torch.from_numpy(np.array(start, dtype=np.float32, order="C")).to(self.device)
        prev, history, iterations, converged = None, [], 0, False
        for it in range(max_iter + 1):
            labels, _, inertia = self.assign(emb, vids)
            history.append(inertia)
            converged = prev is not None and bool(torch.equal(labels, prev))
            prev = labels
            if converged or it == max_iter:
                break
            self.update(emb, labels, vids)
            iterations += 1
        self.labels = prev
        counts = torch.bincount(prev.to(torch.int64), minlength=self.k).cpu().numpy().astype(np.uint64)
        return {"inertia": history[-1], "iterations": iterations, "converged": converged, "counts": counts,
                "history": history}

    def predict(self, emb, vertices=None):
        """The nearest centroid of every listed row: int32 [count] on the GPU."""
        n = self._table(emb)
        self._refresh(emb, n)
        return self.assign(emb, self._list(vertices))[0]


def nmi(a, b) -> float:
    """Normalised mutual information of two labelings, scikit-learn's definition: the mutual
    information over the arithmetic mean of the two entropies, natural logarithm, float64 on the
    host.  1.0 when both sides have a single class; 0.0 when the mean entropy is 0 otherwise."""
    a, b = _host(a).reshape(-1), _host(b).reshape(-1)
    if len(a) != len(b) or not len(a):
        raise ValueError("nmi needs two labelings of one length >= 1")
    ca, ia = np.unique(a, return_inverse=True)
    cb, ib = np.unique(b, return_inverse=True)
    if len(ca) == 1 and len(cb) == 1:
        return 1.0
    table = np.zeros((len(ca), len(cb)), dtype=np.float64)
    np.add.at(table, (ia.reshape(-1), ib.reshape(-1)), 1.0)
    total = float(len(a))
    pa, pb = table.sum(axis=1) / total, table.sum(axis=0) / total
    ha, hb = -float((pa * np.log(pa)).sum()), -float((pb * np.log(pb)).sum())
    mean = 0.5 * (ha + hb)
    if mean <= 0:
        return 0.0
    i, j = np.nonzero(table)
    pij = table[i, j] / total
    mi = float((pij * (np.log(pij) - np.log(pa[i]) - np.log(pb[j]))).sum())
    return max(mi, 0.0) / mean


def modularity_from_stats(intra, vol) -> float:
    """Q = sum_c (intra_c / M - (vol_c / M)^2), M = sum vol; 0.0 for a graph without edges.  The counts are
    integers, so the sum is taken exactly, as sum_c (intra_c M - vol_c^2) over M^2, and rounded once to float64."""
    intra = [int(x) for x in np.asarray(intra).reshape(-1)]
    vol = [int(x) for x in np.asarray(vol).reshape(-1)]
    m = sum(vol)
    if m == 0:
        return 0.0
    return sum(i * m - v * v for i, v in zip(intra, vol)) / (m * m)


def modularity(g, part, k: int | None = None) -> float:
    """Newman's modularity of the partition part [n] (entries < k) on g's current graph, taken
    as the symmetric graph it stores (every edge as two slots)."""
    if k is None:
        k = int(part.max()) + 1
    intra, vol = g.partition_stats(part, k)
    return modularity_from_stats(intra, vol)


def evaluate_clustering(g, emb, vertices, y, k: int | None = None, normalize: bool = True, seed: int = 0,
                        max_iter: int = 100) -> dict:
    """Cluster all n rows of emb (k: the number of classes of y by default) and score the partition
    twice: against the labels y of the labelled vertices, and on g's current graph.  Returns
    {"nmi", "modularity", "inertia", "iterations"}."""
    vertices, y = _host(vertices).reshape(-1).astype(np.int64), _host(y).reshape(-1)
    if k is None:
        k = len(np.unique(y))
    km = VertexClustering(g, emb.shape[1], k, normalize=normalize)
    row = km.fit(emb, seed=seed, max_iter=max_iter)
    labels = km.labels.cpu().numpy()
    return {"nmi": nmi(y, labels[vertices]), "modularity": modularity(g, km.labels, k), "inertia": row["inertia"],
            "iterations": row["iterations"]}
