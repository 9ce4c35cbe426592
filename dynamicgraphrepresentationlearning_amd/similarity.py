"""Queries over the embeddings, on the device: nearest neighbours and link scores.

    sim = Similarity(g, sg.emb_in, sg.emb_out, metric="dot")   # SGNS trains emb_in[u] . emb_out[v]
    scores = sim.score(next_batch)                      # before insert_edges_batch applies it
    ids, s = sim.most_similar(queries, k=10, exclude_neighbours=True)   # recommend non-neighbours
    row = link_prediction(g, sim, next_batch)           # {"auc", "positives", "negatives"}

The tables are read where they lie by the HIP kernels behind wharf_emb_* (exact search, no
q x n score matrix); neighbour exclusion and has_edges read the handle's current graph in HBM.
Semantics (the one dot product, the total order, eligibility): DESIGN.md §12.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_METRICS = {"dot": L.WHARF_EMB_DOT, "cosine": L.WHARF_EMB_COSINE}


class Similarity:
    """Scores rows of `emb` (the query side) against rows of `other` (default: `emb` itself).

    g: a WharfMH handle on the tables' GPU; an empty one will do unless neighbours are excluded.
    The tables stay where they are; call refresh() after training changed them (cosine)."""

    def __init__(self, g, emb, other=None, metric: str = "cosine"):
        import torch

        if metric not in _METRICS:
            raise ValueError(f"metric must be one of {sorted(_METRICS)}")
        self.g, self.metric = g, metric
        self.device = torch.device("cuda", g.device)
        self.emb_q, self.emb_r = emb, emb if other is None else other
        for t in (self.emb_q, self.emb_r):
            if (t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.device != self.device
                    or t.shape != self.emb_q.shape):
                raise ValueError(f"the tables must be contiguous float32 [n, dim] tensors of one shape on {self.device}")
        self.n, self.dim = self.emb_q.shape
        self.rnorm_q = self.rnorm_r = None
        if metric == "cosine":
            self.refresh()

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _sync(self) -> None:
        # the library runs on the handle's own stream: torch's pending work on its inputs first
        import torch
        torch.cuda.synchronize(self.device)

    def _list(self, a, what: str, width: int):
        """A u32 list on the GPU: numpy / sequence (copied), or a contiguous 32-bit device tensor (as it is)."""
        import torch

        if getattr(a, "is_cuda", False):
            if a.dtype not in (torch.int32, torch.uint32) or not a.is_contiguous() or a.device != self.device:
                raise ValueError(f"device {what} must be a contiguous 32-bit tensor on {self.device}")
            t = a
        else:
            host = np.ascontiguousarray(np.asarray(a, dtype=np.uint32))
            t = torch.from_numpy(host.view(np.int32)).to(self.device)
        if width == 2 and (t.dim() != 2 or t.shape[1] != 2):
            raise ValueError(f"{what} must have the shape [count, 2]")
        return t.reshape(-1, width) if width == 2 else t.reshape(-1)

    def _params(self, k: int = 1, flags: int = 0, splits: int = 0) -> L.wharf_emb_params:
        p = L.wharf_emb_params()
        p.dim, p.metric, p.k, p.flags, p.splits, p.reserved = self.dim, _METRICS[self.metric], k, flags, splits, 0
        return p

    def _norms(self, emb):
        import torch

        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        L.check(L.lib.wharf_emb_row_norms(self.g._h, self._p(emb), self.n, self.dim, self._p(out)), self.g._h,
                "emb_row_norms")
        return out

    def refresh(self) -> None:
        """Recompute the reciprocal row norms (cosine) from the tables as they are now."""
        self._sync()
        self.rnorm_q = self._norms(self.emb_q)
        self.rnorm_r = self.rnorm_q if self.emb_r is self.emb_q else self._norms(self.emb_r)

    def score(self, pairs):
        """The score of every (u, v) of pairs [count, 2]: a float32 tensor [count] on the GPU."""
        import torch

        pairs = self._list(pairs, "pairs", 2)
        out = torch.empty(pairs.shape[0], dtype=torch.float32, device=self.device)
        if not pairs.shape[0]:
            return out
        p = self._params()
        self._sync()
        L.check(L.lib.wharf_emb_score_pairs(self.g._h, C.byref(p), self._p(self.emb_q), self._p(self.emb_r), self.n,
                                            self._p(self.rnorm_q), self._p(self.rnorm_r), self._p(pairs),
                                            pairs.shape[0], self._p(out)), self.g._h, "emb_score_pairs")
        return out

    def most_similar(self, queries, k: int = 10, exclude_self: bool = True, exclude_neighbours: bool = False,
                     splits: int = 0):
        """(ids int64 [q, k], scores float32 [q, k]) on the GPU: for every query vertex the k best
        eligible rows, best first.  Past the eligible rows: id 0xFFFFFFFF, score -inf."""
        import torch

        queries = self._list(queries, "queries", 1)
        q = queries.numel()
        ids = torch.empty(q, k, dtype=torch.int32, device=self.device)
        scores = torch.empty(q, k, dtype=torch.float32, device=self.device)
        if q:
            flags = (L.WHARF_EMB_EXCLUDE_SELF if exclude_self else 0) | \
                    (L.WHARF_EMB_EXCLUDE_NEIGHBOURS if exclude_neighbours else 0)
            p = self._params(k, flags, splits)
            self._sync()
            L.check(L.lib.wharf_emb_topk(self.g._h, C.byref(p), self._p(self.emb_q), self._p(self.emb_r), self.n,
                                         self._p(self.rnorm_q), self._p(self.rnorm_r), self._p(queries), q,
                                         self._p(ids), self._p(scores)), self.g._h, "emb_topk")
        return ids.to(torch.int64) & 0xFFFFFFFF, scores


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def auc(pos_scores, neg_scores) -> float:
    """ROC AUC as the Mann-Whitney statistic with average ranks: the share of (positive, negative)
    pairs the positive wins, a tie counting one half.  float64 on the host."""
    pos = _host(pos_scores).astype(np.float64).reshape(-1)
    neg = _host(neg_scores).astype(np.float64).reshape(-1)
    if not len(pos) or not len(neg):
        raise ValueError("auc needs at least one positive and one negative score")
    both = np.concatenate([pos, neg])
    order = np.argsort(both, kind="stable")
    vals = both[order]
    start = np.flatnonzero(np.concatenate([[True], vals[1:] != vals[:-1]]))   # the runs of equal values
    end = np.concatenate([start[1:], [len(vals)]])
    run = np.cumsum(np.concatenate([[True], vals[1:] != vals[:-1]])) - 1
    avg = (start + end + 1) / 2.0                                             # mean of the 1-based ranks of a run
    ranks = np.empty(len(both), dtype=np.float64)
    ranks[order] = avg[run]
    u = ranks[: len(pos)].sum() - len(pos) * (len(pos) + 1) / 2.0
    return float(u / (len(pos) * float(len(neg))))


def hits_at_k(ids, targets) -> float:
    """The share of queries whose target id is in their list: ids [q, k], targets [q]."""
    ids = _host(ids).astype(np.int64)
    targets = _host(targets).astype(np.int64).reshape(-1)
    if ids.ndim != 2 or len(ids) != len(targets) or not len(targets):
        raise ValueError("ids must be [q, k] and targets [q], q >= 1")
    return float((ids == targets[:, None]).any(axis=1).mean())


def sample_non_edges(g, count: int, seed: int = 0) -> np.ndarray:
    """count pairs (u, v), u != v, that are no edges of g's current graph: uint32 [count, 2].
    numpy.random.default_rng(seed) draws uniform pairs in rounds of `count`; a round keeps what is
    neither a self loop nor marked by g.has_edges.  Deterministic in (graph, count, seed)."""
    n = g.number_of_vertices()
    rng = np.random.default_rng(seed)
    kept, have = [], 0
    for _ in range(64):
        if have >= count:
            break
        draw = rng.integers(0, n, size=(count, 2), dtype=np.int64).astype(np.uint32)
        draw = draw[draw[:, 0] != draw[:, 1]]
        if len(draw):
            draw = draw[~g.has_edges(draw)]
        kept.append(draw)
        have += len(draw)
    if have < count:
        raise RuntimeError(f"sample_non_edges: {have} of {count} pairs after 64 rounds")
    return np.ascontiguousarray(np.concatenate(kept)[:count])


def link_prediction(g, sim: Similarity, pos_pairs, neg_pairs=None, seed: int = 0) -> dict:
    """Score pos_pairs (e.g. the next batch, before it is inserted) against negatives (default:
    as many sampled non-edges) and return {"auc", "positives", "negatives"}."""
    pos = sim.score(pos_pairs)
    if neg_pairs is None:
        neg_pairs = sample_non_edges(g, int(pos.numel()), seed)
    neg = sim.score(neg_pairs)
    return {"auc": auc(pos, neg), "positives": int(pos.numel()), "negatives": int(neg.numel())}
