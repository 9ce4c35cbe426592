"""numpy restatement of the classifier contracts of DESIGN.md §11 (TEST INFRASTRUCTURE ONLY).

Written from that section, not from the kernels: min / max of the listed rows, the scaled rows,
logits, softmax loss and gradient, prediction, confusion matrix and metrics, in the dtype asked
for (float64, or float32 with numpy's own summation, exp and log).
"""
from __future__ import annotations

import numpy as np


def minmax(emb, vids):
    rows = np.asarray(emb)[np.asarray(vids, dtype=np.int64)]
    return rows.min(axis=0), rows.max(axis=0)


def scale_of(lo, hi):
    """MinMaxScaler's rule in float32: 1 / (hi - lo), 1 where hi == lo."""
    span = np.asarray(hi, dtype=np.float32) - np.asarray(lo, dtype=np.float32)
    return np.where(span > 0, np.float32(1) / np.where(span > 0, span, np.float32(1)), np.float32(1)).astype(np.float32)


def scaled(emb, vids, lo, scale, dtype):
    """x' = (x - lo) * scale: a subtract, then a multiply, in dtype."""
    x = np.asarray(emb)[np.asarray(vids, dtype=np.int64)].astype(dtype)
    return (x - np.asarray(lo).astype(dtype)) * np.asarray(scale).astype(dtype)


def logits(emb, vids, lo, scale, wb, dtype):
    wb = np.asarray(wb).astype(dtype)
    return scaled(emb, vids, lo, scale, dtype) @ wb[:, :-1].T + wb[:, -1]


def loss_grad(emb, vids, labels, lo, scale, wb, dtype):
    """(sum_i -log p_{i, y_i}, sum_i (p_i - onehot_i) (x'_i, 1)^T) in dtype, no regulariser."""
    x = scaled(emb, vids, lo, scale, dtype)
    wb = np.asarray(wb).astype(dtype)
    y = np.asarray(labels, dtype=np.int64)
    z = x @ wb[:, :-1].T + wb[:, -1]
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    rows = np.arange(len(y))
    loss = (np.log(s[:, 0]) - z[rows, y]).sum(dtype=dtype)
    d = e / s
    d[rows, y] -= dtype(1)
    x1 = np.concatenate([x, np.ones((len(y), 1), dtype=dtype)], axis=1)
    return dtype(loss), (d.T @ x1).astype(dtype)


def objective_grad(emb, vids, labels, lo, scale, wb, l2, dtype):
    """loss + l2/2 ||W||^2 with the bias unpenalised, and its gradient."""
    loss, grad = loss_grad(emb, vids, labels, lo, scale, wb, dtype)
    W = np.asarray(wb).astype(dtype)[:, :-1]
    grad = grad.copy()
    grad[:, :-1] += dtype(l2) * W
    return dtype(loss + dtype(0.5 * l2) * (W * W).sum(dtype=dtype)), grad


def predict(z):
    """The lowest class index that attains the row maximum."""
    return np.argmax(z, axis=1).astype(np.uint32)


def top_two_gap(z):
    s = np.sort(np.asarray(z, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def confusion(y_true, y_pred, C):
    y_true, y_pred = np.asarray(y_true, dtype=np.int64), np.asarray(y_pred, dtype=np.int64)
    return np.bincount(y_true * C + y_pred, minlength=C * C).reshape(C, C).astype(np.uint64)


def metrics(cm):
    """accuracy and the three F1 averages of a confusion matrix, scikit-learn's definitions, class by class."""
    cm = np.asarray(cm, dtype=np.float64)
    C, total = len(cm), cm.sum()
    f1, weight, present = [], [], []
    for c in range(C):
        tp, fp, fn = cm[c, c], cm[:, c].sum() - cm[c, c], cm[c].sum() - cm[c, c]
        f1.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0)
        weight.append(cm[c].sum())
        present.append(cm[c].sum() + cm[:, c].sum() > 0)
    f1, weight, present = np.array(f1), np.array(weight), np.array(present)
    tp_all = np.trace(cm)
    return {"accuracy": tp_all / total, "f1_macro": f1[present].mean(),
            "f1_micro": 2 * tp_all / (2 * tp_all + 2 * (total - tp_all)),
            "f1_weighted": (f1 * weight).sum() / total}
