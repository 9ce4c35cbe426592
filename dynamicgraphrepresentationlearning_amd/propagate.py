"""Feature propagation over the live graph, on the device: Y = alpha D_l (A + s I) D_r X + beta R.

    prop = GraphPropagation(g, norm="sym", self_loops=True)     # the weights from the current degrees
    feats = sgc_features(g, sg.emb_in, hops=2)                  # (D^-1/2 (A + I) D^-1/2)^2 X, into evaluate_embeddings
    lp = LabelPropagation(g, classes=17).fit(train_ids, train_y)   # F <- a A^ F + (1 - a) Y, no training
    print(lp.score(test_ids, test_y))
    g.insert_edges_batch(batch); prop.refresh()
    rows = prop.apply(sg.emb_in, ids=new_vertices)              # the neighbours' mean for vertices the trainer has not seen

The graph is read where it lies, next to the table, by the HIP kernels behind wharf_graph_propagate
(no copy of the CSR, no float atomics: the same inputs give the same bits).  Semantics: DESIGN.md §14.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .clf import metrics

DIMS = (16, 32, 64, 128, 192, 256)   # the widths wharf_graph_propagate takes


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class GraphPropagation:
    """One sparse product with the handle's current graph per apply().

    norm: "sym": wsrc = wdst = (deg + s)^-1/2; "mean": wdst = 1 / (deg + s); "sum": no weights; s = 1 with
    self_loops, which also adds the vertex's own row.  The weights are computed from g.degrees() in
    float64, cast to float32, and are 0 where the denominator is; refresh() recomputes them after an
    update batch (the caller decides when)."""

    def __init__(self, g, norm: str = "sym", self_loops: bool = True):
        import torch

        if norm not in ("sym", "mean", "sum"):
            raise ValueError('norm must be "sym", "mean" or "sum"')
        self.g, self.norm, self.self_loops = g, norm, bool(self_loops)
        self.device = torch.device("cuda", g.device)
        self.n = g.number_of_vertices()
        self.wsrc = self.wdst = None
        self.refresh()

    def refresh(self) -> None:
        import torch

        if self.norm == "sum":
            return
        den = self.g.degrees().cpu().numpy().view(np.uint32).astype(np.float64) + (1.0 if self.self_loops else 0.0)
        power = -0.5 if self.norm == "sym" else -1.0
        w = np.where(den > 0, np.where(den > 0, den, 1.0) ** power, 0.0).astype(np.float32)
        self.wdst = torch.from_numpy(w).to(self.device)
        self.wsrc = self.wdst if self.norm == "sym" else None

    # -- arguments --------------------------------------------------------------------------
    def _table(self, t, what: str, dim=None):
        import torch

        if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != self.n or not t.is_contiguous()
                or t.device != self.device or (dim is not None and t.shape[1] != dim)):
            raise ValueError(f"{what} must be a contiguous float32 [{self.n}, {dim or 'dim'}] tensor on {self.device}")
        return t.shape[1]

    def _ids(self, ids):
        """None, or a u32 list on the GPU: numpy / sequence (copied), or a contiguous 32-bit device tensor."""
        import torch

        if ids is None:
            return None
        if getattr(ids, "is_cuda", False):
            if ids.dtype not in (torch.int32, torch.uint32) or not ids.is_contiguous() or ids.device != self.device:
                raise ValueError(f"device ids must be a contiguous 32-bit tensor on {self.device}")
            return ids.reshape(-1)
        host = np.ascontiguousarray(np.asarray(ids), dtype=np.uint32).reshape(-1)
        return torch.from_numpy(host.view(np.int32)).to(self.device)

    # -- the kernel -------------------------------------------------------------------------
    def apply(self, x, ids=None, out=None, alpha: float = 1.0, beta: float = 0.0, resid=None):
        """out[i] = alpha * (the weighted sum over the neighbours of ids[i], or of i) + beta * resid[ids[i]]:
        float32 [count or n, dim] on the GPU.  out must not overlap x or resid."""
        import torch

        dim = self._table(x, "x")
        if resid is not None:
            self._table(resid, "resid", dim)
        ids = self._ids(ids)
        rows = self.n if ids is None else ids.numel()
        if out is None:
            out = torch.empty(rows, dim, dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or tuple(out.shape) != (rows, dim) or not out.is_contiguous()
                or out.device != self.device):
            raise ValueError(f"out must be a contiguous float32 [{rows}, {dim}] tensor on {self.device}")
        p = L.wharf_prop_params()
        p.dim, p.flags, p.alpha, p.beta = dim, (L.WHARF_PROP_SELF if self.self_loops else 0), alpha, beta
        torch.cuda.synchronize(self.device)   # the library runs on the handle's own stream
        L.check(L.lib.wharf_graph_propagate(self.g._h, C.byref(p), _ptr(x), self.n, _ptr(self.wsrc), _ptr(self.wdst),
                                            _ptr(resid), _ptr(ids), rows, _ptr(out)), self.g._h, "graph_propagate")
        return out

    def power(self, x, hops: int):
        """hops applications to the whole table, between two buffers of its size; x is never written."""
        import torch

        if hops < 1:
            return x.clone()
        cur, bufs = x, [torch.empty_like(x), torch.empty_like(x) if hops > 1 else None]
        for h in range(hops):
            cur = self.apply(cur, out=bufs[h & 1])
        return cur


def sgc_features(g, emb, hops: int = 2):
    """Simplified graph convolution: (D~^-1/2 (A + I) D~^-1/2)^hops emb, a table VertexClassifier /
    evaluate_embeddings take as it is."""
    return GraphPropagation(g, "sym", True).power(emb, hops)


class LabelPropagation:
    """Label spreading F <- alpha A^ F + (1 - alpha) Y from the one-hot labels Y of the listed vertices,
    one kernel call an iteration.  scores: F, float32 [n, dim] on the GPU, its first `classes` columns
    the classes (dim: the next width the kernel takes, the other columns stay 0)."""

    def __init__(self, g, classes: int, alpha: float = 0.9, max_iter: int = 50, tol: float = 1e-4, norm: str = "sym",
                 self_loops: bool = False):
        if not 1 <= classes <= DIMS[-1]:
            raise ValueError(f"classes must be 1..{DIMS[-1]}")
        self.prop = GraphPropagation(g, norm, self_loops)
        self.g, self.classes, self.alpha, self.max_iter, self.tol = g, int(classes), float(alpha), int(max_iter), tol
        self.dim = next(d for d in DIMS if d >= classes)
        self.device = self.prop.device
        self.scores = None

    def _labels(self, ids, y):
        import torch

        ids, y = self.prop._ids(ids), self.prop._ids(y)
        if ids.numel() != y.numel():
            raise ValueError("ids and labels differ in length")
        ids, y = ids.to(torch.int64) & 0xFFFFFFFF, y.to(torch.int64) & 0xFFFFFFFF
        if ids.numel() and (int(ids.max()) >= self.prop.n or int(y.max()) >= self.classes):
            raise ValueError("a vertex id or a label is out of range")
        return ids, y

    def fit(self, ids, y) -> dict:
        import torch

        ids, y = self._labels(ids, y)
        Y = torch.zeros(self.prop.n, self.dim, dtype=torch.float32, device=self.device)
        Y[ids, y] = 1.0
        F, nxt = Y.clone(), torch.empty_like(Y)
        it, delta = 0, float("inf")
        while it < self.max_iter:
            self.prop.apply(F, out=nxt, alpha=self.alpha, beta=1.0 - self.alpha, resid=Y)
            delta = float((nxt - F).abs().max())
            F, nxt = nxt, F
            it += 1
            if delta < self.tol:
                break
        self.scores = F
        return {"iterations": it, "converged": delta < self.tol, "delta": delta}

    def predict(self, ids):
        """The class of every listed vertex, int32 [count] on the GPU: the lowest index of the maximal score."""
        import torch

        idx = self.prop._ids(ids).to(torch.int64) & 0xFFFFFFFF
        f = self.scores[idx, :self.classes]
        cols = torch.arange(self.classes, device=self.device).expand_as(f)
        best = f.max(dim=1, keepdim=True).values
        return torch.where(f == best, cols, self.classes).min(dim=1).values.to(torch.int32)

    def score(self, ids, y) -> dict:
        """clf.metrics of the listed vertices, plus "confusion" (u64 [classes, classes], row: true class)."""
        _, yt = self._labels(ids, y)
        pred = self.predict(ids).cpu().numpy()
        conf = np.zeros((self.classes, self.classes), dtype=np.uint64)
        np.add.at(conf, (yt.cpu().numpy(), pred), 1)
        return {**metrics(conf), "confusion": conf}
