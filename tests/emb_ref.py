"""numpy restatement of the embedding queries: scores in float64 and float32,
the total order, eligibility from a CSR, top-k, has_edges, and AUC by its O(P N) definition.

float32: the k-ordered chain s = fmaf(x[k], y[k], s).  numpy has no fma; a step is computed as
float32(float64(x) * float64(y) + float64(s)): the product is exact in float64, the sum is rounded
to 53 bits and then to 24, which differs from one rounding only on a double-rounding tie.  On
integer data (every partial sum exact) it is the chain itself.
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
NO_ID = 0xFFFFFFFF


# -- scores ---------------------------------------------------------------------------------
def chain32(x, y):
    """The chain over the last axis of broadcastable float32 arrays."""
    x, y = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(y, np.float32))
    s = np.zeros(x.shape[:-1], dtype=np.float32)
    for k in range(x.shape[-1]):
        s = (x[..., k].astype(np.float64) * y[..., k].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def rnorm32(emb):
    s = chain32(emb, emb)
    with np.errstate(divide="ignore"):
        r = np.float32(1.0) / np.sqrt(s, dtype=np.float32)
    return np.where(s == 0, np.float32(0), r).astype(np.float32)


def rnorm64(emb):
    s = (np.asarray(emb, np.float64) ** 2).sum(axis=-1)
    with np.errstate(divide="ignore"):
        return np.where(s == 0, 0.0, 1.0 / np.sqrt(s))


def abs_dot64(x, y):
    """sum_k |x_k y_k| in float64 (the scale of the dot's error bound)."""
    return np.abs(np.asarray(x, np.float64) * np.asarray(y, np.float64)).sum(axis=-1)


def pair_scores64(eq, er, pairs, metric="dot"):
    x, y = np.asarray(eq, np.float64)[pairs[:, 0]], np.asarray(er, np.float64)[pairs[:, 1]]
    s = (x * y).sum(axis=-1)
    if metric == "cosine":
        s = s * rnorm64(eq)[pairs[:, 0]] * rnorm64(er)[pairs[:, 1]]
    return s


def pair_scores32(eq, er, pairs, metric="dot", rq=None, rr=None):
    """The contract in float32; rq / rr default to rnorm32 of the tables."""
    s = chain32(eq[pairs[:, 0]], er[pairs[:, 1]])
    if metric == "cosine":
        rq = rnorm32(eq) if rq is None else rq
        rr = rnorm32(er) if rr is None else rr
        s = ((s * rq[pairs[:, 0]]).astype(np.float32) * rr[pairs[:, 1]]).astype(np.float32)
    return s


def all_pairs(queries, n):
    q = np.asarray(queries, np.int64)
    return np.stack([np.repeat(q, n), np.tile(np.arange(n, dtype=np.int64), len(q))], axis=1)


def score_matrix64(eq, er, queries, metric="dot"):
    return pair_scores64(eq, er, all_pairs(queries, len(er)), metric).reshape(len(queries), len(er))


def score_matrix32(eq, er, queries, metric="dot", rq=None, rr=None):
    return pair_scores32(eq, er, all_pairs(queries, len(er)), metric, rq, rr).reshape(len(queries), len(er))


# -- bounds (derived in DESIGN.md §12, not measured) ---------------------------------------
def dot_bound(x, y):
    """|chain - exact| <= 1.01 dim u sum|x_k y_k| per pair."""
    return 1.01 * np.shape(x)[-1] * U * abs_dot64(x, y)


def cosine_bound(dim):
    return (2 * dim + 16) * U


def rnorm_bound(dim):
    """relative"""
    return (dim / 2 + 4) * U


# -- order, eligibility, top-k ---------------------------------------------------------------
def order(scores, ids=None):
    """Indices that list the candidates best first: score descending, on equal scores (float ==) id ascending."""
    scores = np.asarray(scores)
    ids = np.arange(len(scores)) if ids is None else np.asarray(ids)
    return np.lexsort((ids, -scores))


def has_edges(off, adj, pairs):
    out = np.zeros(len(pairs), dtype=bool)
    for i, (u, v) in enumerate(np.asarray(pairs, np.int64)):
        row = adj[int(off[u]):int(off[u + 1])]
        j = np.searchsorted(row, v)
        out[i] = j < len(row) and row[j] == v
    return out


def eligible(n, query, exclude_self=True, csr=None):
    """bool [n]; csr = (off, adj) excludes the targets of the query's row."""
    ok = np.ones(n, dtype=bool)
    if exclude_self:
        ok[query] = False
    if csr is not None:
        off, adj = csr
        ok[adj[int(off[query]):int(off[query + 1])]] = False
    return ok


def topk_row(scores, ok, k):
    """(ids u32 [k], scores [k]) of one query; the tail past the eligible rows is {NO_ID, -inf}."""
    cand = np.flatnonzero(ok)
    best = cand[order(scores[cand], cand)][:k]
    ids = np.full(k, NO_ID, dtype=np.uint32)
    out = np.full(k, -np.inf, dtype=scores.dtype)
    ids[: len(best)] = best
    out[: len(best)] = scores[best]
    return ids, out


def topk(score_matrix, queries, k, exclude_self=True, csr=None):
    n = score_matrix.shape[1]
    rows = [topk_row(score_matrix[i], eligible(n, int(v), exclude_self, csr), k) for i, v in enumerate(queries)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


# -- the inputs the CPU and the GPU tests share ----------------------------------------------
def integer_tables(n, dim, seed=1):
    """Entries uniform integers in [-4, 4]: every dot is an exact integer, ties are plentiful."""
    rng = np.random.default_rng(seed + dim)
    return (rng.integers(-4, 5, (n, dim)).astype(np.float32), rng.integers(-4, 5, (n, dim)).astype(np.float32))


def onehot_tables(n, dim):
    """emb_q[r] = (1 + r) e_{r mod dim}, emb_r[r] = (2 + r mod 5) e_{(7 r + 3) mod dim}: asymmetric,
    so a transposed operand or a wrong accumulator map shows."""
    eq, er = np.zeros((n, dim), np.float32), np.zeros((n, dim), np.float32)
    r = np.arange(n)
    eq[r, r % dim] = 1 + r
    er[r, (7 * r + 3) % dim] = 2 + r % 5
    return eq, er


def float_tables(n, dim, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n, dim)).astype(np.float32), rng.normal(0, 1, (n, dim)).astype(np.float32))


def float_queries(n=1100, q=70, seed=3):
    """q query ids with repeats."""
    qs = np.random.default_rng(seed).integers(0, n, q).astype(np.uint32)
    qs[-1] = qs[0]
    qs[q // 2] = qs[1]
    return qs


# -- evaluation ------------------------------------------------------------------------------
def auc(pos, neg):
    """The definition: the share of (positive, negative) pairs the positive wins, a tie one half."""
    pos, neg = np.asarray(pos, np.float64).reshape(-1), np.asarray(neg, np.float64).reshape(-1)
    wins = 0.0
    for p in pos:
        wins += float((p > neg).sum()) + 0.5 * float((p == neg).sum())
    return wins / (len(pos) * len(neg))
