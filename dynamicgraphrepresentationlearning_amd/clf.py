"""Vertex classification from the embeddings, on the device.

The last stage of the reference's experiment (experiments/bin/vertex-classification.py,
run by vertex-classification.cpp:153-194 after every yskip run): min-max scale
the embeddings, fit a multinomial logistic regression on 75 % of the labelled
vertices, report accuracy and macro / micro / weighted F1:

    ids, y, classes = read_labels("wiki-labels")
    row = evaluate_embeddings(g, sg.emb_in, ids, y)     # the results.csv row, as a dict

The embedding table is read where it lies: every loss / gradient evaluation and
every prediction is one pass of the HIP kernels behind wharf_clf_* over the
listed rows.  L-BFGS itself is torch.optim.LBFGS on the [C, dim + 1] weights
(plumbing).  Semantics: DESIGN.md §11.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def read_labels(path):
    """The reference's label file, one "<vertex> <label>" per line: (ids u32, y u32, classes), where
    classes holds the file's label values in ascending order and y[i] indexes it."""
    data = np.loadtxt(path, dtype=np.int64, ndmin=2)
    if data.shape[1] != 2:
        raise ValueError(f"{path}: expected two columns, vertex and label")
    classes, y = np.unique(data[:, 1], return_inverse=True)
    return data[:, 0].astype(np.uint32), y.reshape(-1).astype(np.uint32), classes


def lbfgs(closure, shape, max_iter: int = 500, history: int = 20, tol_grad: float = 1e-7, tol_change: float = 1e-9,
          dtype=None, device=None, x0=None):
    """Minimise closure(x) -> (loss, grad) from zeros(shape) (or x0) with torch.optim.LBFGS and its
    strong-Wolfe line search: at most max_iter iterations and 5/4 as many evaluations, until the
    gradient's max-norm is below tol_grad or a step changes the loss by less than tol_change.
    loss is a float; grad is a tensor, or an array, of x's shape.  Returns (x, loss at x, iterations)."""
    import torch

    dtype = dtype or torch.float64
    x = torch.zeros(shape, dtype=dtype, device=device) if x0 is None else torch.as_tensor(x0).detach().clone().to(
        dtype=dtype, device=device)
    x.requires_grad_(True)
    opt = torch.optim.LBFGS([x], lr=1.0, max_iter=max_iter, max_eval=max_iter * 5 // 4, history_size=history,
                            tolerance_grad=tol_grad, tolerance_change=tol_change, line_search_fn="strong_wolfe")

    def step():
        loss, grad = closure(x.detach())
        x.grad = torch.as_tensor(grad, dtype=dtype, device=x.device).reshape(x.shape).clone()
        return torch.tensor(float(loss), dtype=torch.float64)

    opt.step(step)
    x = x.detach()
    return x, float(closure(x)[0]), int(opt.state[opt._params[0]]["n_iter"])


def metrics(confusion) -> dict:
    """accuracy, f1_macro, f1_micro, f1_weighted of a confusion matrix (row: true, column: predicted)
    with scikit-learn's definitions: a class absent from truth and prediction is left out of the
    macro mean, an F1 with a zero denominator is 0.  float64 on the host."""
    cm = np.asarray(confusion, dtype=np.float64)
    total = cm.sum()
    tp = np.diag(cm)
    support, predicted = cm.sum(axis=1), cm.sum(axis=0)
    present = (support + predicted) > 0
    denom = support + predicted          # 2 tp + fp + fn
    f1 = np.where(denom > 0, 2 * tp / np.where(denom > 0, denom, 1.0), 0.0)
    acc = float(tp.sum() / total) if total else 0.0
    return {
        "accuracy": acc,
        "f1_macro": float(f1[present].mean()) if present.any() else 0.0,
        "f1_micro": acc,                 # single-label: micro F1 is the accuracy
        "f1_weighted": float((f1 * support).sum() / total) if total else 0.0,
    }


class VertexClassifier:
    """Softmax regression on min-max scaled rows of an embedding table that stays where it is.

    g: a WharfMH handle on the table's GPU (an empty one will do); it gives the kernels their
    device and stream.  wb: [classes, dim + 1] float32 on that GPU, a class's weights then its bias."""

    def __init__(self, g, dim: int, classes: int, l2: float = 1.0):
        import torch

        self.g, self.dim, self.classes, self.l2 = g, dim, classes, float(l2)
        self.device = torch.device("cuda", g.device)
        self.lo = self.hi = self.scale = None
        self.wb = torch.zeros(classes, dim + 1, dtype=torch.float32, device=self.device)
        self.iterations = 0
        self.objective = None

    # -- arguments --------------------------------------------------------------------------
    def _params(self) -> L.wharf_clf_params:
        p = L.wharf_clf_params()
        p.dim, p.classes = self.dim, self.classes
        return p

    def _list(self, a, what: str):
        """A u32 list on the GPU: numpy / sequence (copied), or a contiguous 32-bit device tensor (as it is)."""
        import torch

        if getattr(a, "is_cuda", False):
            if a.dtype not in (torch.int32, torch.uint32) or not a.is_contiguous() or a.device != self.device:
                raise ValueError(f"device {what} must be a contiguous 32-bit tensor on {self.device}")
            return a.reshape(-1)
        host = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        return torch.from_numpy(host.view(np.int32)).to(self.device)

    def _table(self, emb):
        import torch

        if (emb.dtype != torch.float32 or emb.dim() != 2 or emb.shape[1] != self.dim or not emb.is_contiguous()
                or emb.device != self.device):
            raise ValueError(f"emb must be a contiguous float32 [n, {self.dim}] tensor on {self.device}")
        return C.c_void_p(emb.data_ptr()), emb.shape[0]

    def _sync(self) -> None:
        # the library runs on the handle's own stream: torch's pending work on its inputs first
        import torch
        torch.cuda.synchronize(self.device)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    # -- kernels ----------------------------------------------------------------------------
    def minmax(self, emb, ids):
        """(lo, hi): per-column minimum and maximum of the listed rows, float32 [dim] on the GPU."""
        import torch

        ptr, n = self._table(emb)
        ids = self._list(ids, "ids")
        lo = torch.empty(self.dim, dtype=torch.float32, device=self.device)
        hi = torch.empty_like(lo)
        self._sync()
        L.check(L.lib.wharf_clf_minmax(self.g._h, ptr, n, self.dim, self._p(ids), ids.numel(), self._p(lo),
                                       self._p(hi)), self.g._h, "clf_minmax")
        return lo, hi

    def set_scaler(self, lo, hi) -> None:
        """MinMaxScaler's rule: scale = 1 / (hi - lo), 1 where hi == lo."""
        import torch

        span = hi - lo
        self.lo, self.hi = lo, hi
        self.scale = torch.where(span > 0, 1.0 / span, torch.ones_like(span)).contiguous()

    def loss_grad(self, emb, ids, y, wb=None, grad=None):
        """(sum of -log p_y as a float, its gradient [classes, dim + 1] on the GPU), no regulariser."""
        import torch

        ptr, n = self._table(emb)
        ids, y = self._list(ids, "ids"), self._list(y, "labels")
        if ids.numel() != y.numel():
            raise ValueError("ids and labels differ in length")
        wb = self.wb if wb is None else wb
        if grad is None:
            grad = torch.empty(self.classes, self.dim + 1, dtype=torch.float32, device=self.device)
        loss = C.c_double()
        p = self._params()
        self._sync()
        L.check(L.lib.wharf_clf_loss_grad(self.g._h, C.byref(p), ptr, n, self._p(ids), self._p(y), ids.numel(),
                                          self._p(self.lo), self._p(self.scale), self._p(wb), self._p(grad),
                                          C.byref(loss)), self.g._h, "clf_loss_grad")
        return loss.value, grad

    def _predict(self, emb, ids, y):
        import torch

        ptr, n = self._table(emb)
        ids = self._list(ids, "ids")
        y = None if y is None else self._list(y, "labels")
        if y is not None and ids.numel() != y.numel():
            raise ValueError("ids and labels differ in length")
        pred = torch.empty(ids.numel(), dtype=torch.int32, device=self.device)
        conf = np.zeros((self.classes, self.classes), dtype=np.uint64) if y is not None else None
        p = self._params()
        self._sync()
        L.check(L.lib.wharf_clf_predict(self.g._h, C.byref(p), ptr, n, self._p(ids), ids.numel(), self._p(self.lo),
                                        self._p(self.scale), self._p(self.wb), None if y is None else self._p(y),
                                        self._p(pred), None if conf is None else conf.ctypes.data_as(C.c_void_p)),
                self.g._h, "clf_predict")
        return pred, conf

    # -- the estimator ----------------------------------------------------------------------
    def objective_grad(self, emb, ids, y, wb):
        """sum loss + l2/2 ||W||^2 (bias unpenalised) and its gradient at wb."""
        loss, grad = self.loss_grad(emb, ids, y, wb)
        W = wb[:, :self.dim]
        grad[:, :self.dim] += self.l2 * W
        return loss + 0.5 * self.l2 * float((W.double() ** 2).sum()), grad

    def fit(self, emb, ids, y, scale_ids=None, max_iter: int = 500):
        import torch

        ids, y = self._list(ids, "ids"), self._list(y, "labels")
        self.set_scaler(*self.minmax(emb, ids if scale_ids is None else scale_ids))
        wb, obj, it = lbfgs(lambda w: self.objective_grad(emb, ids, y, w.contiguous()),
                            (self.classes, self.dim + 1), max_iter=max_iter, dtype=torch.float32, device=self.device)
        self.wb, self.objective, self.iterations = wb.contiguous(), obj, it
        return self

    def predict(self, emb, ids):
        """The predicted class of every listed row: int32 [count] on the GPU."""
        return self._predict(emb, ids, None)[0]

    def score(self, emb, ids, y) -> dict:
        """metrics() of the listed rows, plus "confusion" (u64 [classes, classes], row: true class)."""
        _, conf = self._predict(emb, ids, y)
        return {**metrics(conf), "confusion": conf}


def evaluate_embeddings(g, emb, ids, y, test_size: float = 0.25, seed: int = 0, classes: int | None = None,
                        l2: float = 1.0, max_iter: int = 500) -> dict:
    """The reference script's recipe: the scaler over all labelled vertices, a seeded permutation
    split, a fit on the training part and the results.csv row of the held-out part."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.uint32).reshape(-1)
    if len(ids) != len(y):
        raise ValueError("ids and labels differ in length")
    classes = int(y.max()) + 1 if classes is None else classes
    perm = np.random.default_rng(seed).permutation(len(ids))
    n_test = int(np.ceil(test_size * len(ids)))   # train_test_split's rounding
    test, train = perm[:n_test], perm[n_test:]
    clf = VertexClassifier(g, emb.shape[1], classes, l2=l2)
    clf.fit(emb, ids[train], y[train], scale_ids=ids, max_iter=max_iter)
    row = clf.score(emb, ids[test], y[test])
    row.update(train=len(train), test=len(test), iterations=clf.iterations, objective=clf.objective,
               classifier=clf, test_index=test)
    return row
