"""numpy restatement of the k-means contract: scores, assignment, inertia and
the centroid update in float64 and in float32 (the k-ordered chain of tests/emb_ref.py), the
derived bounds, partition statistics and NMI by their definitions, and the inputs the CPU and
the GPU tests share.

x is always the listed rows in list order, [count, dim] (emb[vids]); r their rnorm values or None.
"""
import numpy as np

from emb_ref import U, chain32

F32 = np.float32


# -- float32: the contract ---------------------------------------------------------------------
def hn32(cent):
    return (F32(0.5) * chain32(cent, cent)).astype(F32)


def scores32(x, cent, r=None):
    """s(i, c) [count, k]: the chain, one multiply (if r), one subtract; -0 folded into +0."""
    s = chain32(x[:, None, :], cent[None, :, :])
    if r is not None:
        s = (s * np.asarray(r, F32)[:, None]).astype(F32)
    s = (s - hn32(cent)[None, :]).astype(F32)
    return (s + F32(0.0)).astype(F32)


def assign_of(scores):
    """The lowest c that attains the maximum under ==; its score."""
    a = np.argmax(scores, axis=1)
    return a.astype(np.uint32), scores[np.arange(len(a)), a]


def xx32(x, r=None):
    s = chain32(x, x)
    if r is not None:
        r = np.asarray(r, F32)
        s = ((s * r).astype(F32) * r).astype(F32)
    return s


def inertia_of(xx, s):
    """sum_i ((double)xx_i - 2 (double)s_i), in list order."""
    return float((np.asarray(xx, np.float64) - 2.0 * np.asarray(s, np.float64)).sum())


def update32(x, assign, cent, r=None):
    """(centroids, counts): f32 sums in list order, one f32 division; an empty cluster keeps its bits."""
    k, dim = cent.shape
    xs = x if r is None else (np.asarray(r, F32)[:, None] * x).astype(F32)
    sums = np.zeros((k, dim), F32)
    for i, c in enumerate(np.asarray(assign, np.int64)):
        sums[c] = (sums[c] + xs[i]).astype(F32)
    counts = np.bincount(np.asarray(assign, np.int64), minlength=k).astype(np.uint64)
    out = cent.copy()
    nz = counts > 0
    out[nz] = (sums[nz] / counts[nz].astype(F32)[:, None]).astype(F32)
    return out, counts


# -- float64 -----------------------------------------------------------------------------------
def scores64(x, cent, r=None):
    x, cent = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    s = x @ cent.T
    if r is not None:
        s = s * np.asarray(r, np.float64)[:, None]
    return s - 0.5 * (cent * cent).sum(axis=1)[None, :]


def xx64(x, r=None):
    s = (np.asarray(x, np.float64) ** 2).sum(axis=1)
    return s if r is None else s * np.asarray(r, np.float64) ** 2


def sums64(x, assign, k, r=None):
    """(sums [k, dim], sums of absolute values [k, dim], counts)"""
    xs = np.asarray(x, np.float64)
    if r is not None:
        xs = xs * np.asarray(r, np.float64)[:, None]
    a = np.asarray(assign, np.int64)
    sums, mags = np.zeros((k, xs.shape[1])), np.zeros((k, xs.shape[1]))
    np.add.at(sums, a, xs)
    np.add.at(mags, a, np.abs(xs))
    return sums, mags, np.bincount(a, minlength=k).astype(np.uint64)


# -- bounds (derived in DESIGN.md §13, not measured) ----------------------------------------------
def score_bound(x, cent, r=None):
    """|s32 - s64| <= 1.01 u ((dim + 2) A r + (dim + 1) hn), A = sum_k |x_k c_k|: [count, k]."""
    dim = x.shape[1]
    A = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(cent, np.float64)).T
    if r is not None:
        A = A * np.abs(np.asarray(r, np.float64))[:, None]
    hn = 0.5 * (np.asarray(cent, np.float64) ** 2).sum(axis=1)
    return 1.01 * U * ((dim + 2) * A + (dim + 1) * hn[None, :])


def xx_bound(x, r=None):
    """the chain x . x (dim u) and the two multiplies by r"""
    return 1.01 * U * (x.shape[1] + 2) * xx64(x, r)


def inertia_bound(x, cent, assign, r=None):
    """the per-row score bounds at the assigned centroids, doubled, plus the xx bounds"""
    sb = score_bound(x, cent, r)[np.arange(len(x)), np.asarray(assign, np.int64)]
    return float((2.0 * sb + xx_bound(x, r)).sum())


def centroid_bound(mags, counts, cent64):
    """sums of m rows: 1.01 (m + 1) u sum |r x_ik| per element; the division: one more u relative."""
    m = np.maximum(counts.astype(np.float64), 1.0)[:, None]
    return 1.01 * (m + 1) * U * mags / m + 1.01 * U * np.abs(cent64)


def decisive(s64, bound):
    """(rows whose float64 best score less its bound exceeds every other score plus its bound,
    per row the centroids whose interval overlaps the best's)."""
    best = np.argmax(s64, axis=1)
    rows = np.arange(len(s64))
    low = s64[rows, best] - bound[rows, best]
    allowed = (s64 + bound) >= low[:, None]
    return allowed.sum(axis=1) == 1, allowed


# -- partition statistics, NMI -------------------------------------------------------------------
def partition_stats(off, adj, part, k):
    off, part = np.asarray(off, np.int64), np.asarray(part, np.int64)
    deg = np.diff(off)
    src = np.repeat(np.arange(len(deg)), deg)
    same = part[src] == part[np.asarray(adj, np.int64)]
    intra = np.bincount(part[src][same], minlength=k).astype(np.uint64)
    vol = np.bincount(part, weights=deg, minlength=k).astype(np.uint64)
    return intra, vol


def modularity(intra, vol):
    """sum_c (intra_c / M - (vol_c / M)^2) in rationals, rounded once"""
    from fractions import Fraction
    m = sum(int(v) for v in vol)
    if not m:
        return 0.0
    return float(sum(Fraction(int(i), m) - Fraction(int(v), m) ** 2 for i, v in zip(intra, vol) if v))


def two_triangles():
    """0-1-2 and 3-4-5, joined by 2-3: (off, adj) with every edge as two slots."""
    nb = {0: [1, 2], 1: [0, 2], 2: [0, 1, 3], 3: [2, 4, 5], 4: [3, 5], 5: [3, 4]}
    off = np.concatenate([[0], np.cumsum([len(nb[v]) for v in range(6)])]).astype(np.uint64)
    adj = np.array([w for v in range(6) for w in nb[v]], dtype=np.uint32)
    return off, adj


def nmi(a, b):
    """The definition from the contingency table, entry by entry."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    ca, cb = sorted(set(a.tolist())), sorted(set(b.tolist()))
    if len(ca) == 1 and len(cb) == 1:
        return 1.0
    n = float(len(a))
    table = {(u, v): 0 for u in ca for v in cb}
    for u, v in zip(a.tolist(), b.tolist()):
        table[(u, v)] += 1
    na = {u: sum(table[(u, v)] for v in cb) for u in ca}
    nb = {v: sum(table[(u, v)] for u in ca) for v in cb}
    ha = -sum(na[u] / n * np.log(na[u] / n) for u in ca)
    hb = -sum(nb[v] / n * np.log(nb[v] / n) for v in cb)
    mi = sum(t / n * np.log(t * n / (na[u] * nb[v])) for (u, v), t in table.items() if t)
    mean = 0.5 * (ha + hb)
    return float(mi / mean) if mean > 0 else 0.0


# -- the inputs the CPU and the GPU tests share --------------------------------------------------
FLOAT_SHAPES = [(65, 64, 7), (333, 64, 2), (1100, 128, 17), (4097, 192, 64), (2049, 256, 256)]


def integer_case(count, dim, k, seed=1):
    """A table of n = count + 3 rows and k centroids with integer entries in [-4, 4], and a list of
    `count` ids with repeats: every score, sum and inertia term is exact."""
    rng = np.random.default_rng(seed + 1000 * dim + 10 * k + count)
    n = count + 3
    emb = rng.integers(-4, 5, (n, dim)).astype(F32)
    cent = rng.integers(-4, 5, (k, dim)).astype(F32)
    vids = rng.integers(0, n, count).astype(np.uint32)
    if count > 2:
        vids[-1] = vids[0]
    return emb, cent, vids


def onehot_case(count, dim, k):
    """rows (1 + i) e_{i mod dim}, centroids (2 + c mod 5) e_{(7 c + 3) mod dim}: asymmetric, so a
    transposed operand or a wrong accumulator map shows."""
    emb, cent = np.zeros((count, dim), F32), np.zeros((k, dim), F32)
    i, c = np.arange(count), np.arange(k)
    emb[i, i % dim] = 1 + i
    cent[c, (7 * c + 3) % dim] = 2 + c % 5
    return emb, cent


def float_case(kind, count, dim, k):
    """(emb [count, dim], centroids [k, dim], vids: a permutation of the rows), default_rng(7).
    structured: centres N(0, 1), rows = a centre + 0.8 N(0, 1), centroids = centres + 0.25 N(0, 1);
    unstructured: rows U(-1, 1), centroids = 0.5 x k distinct rows."""
    rng = np.random.default_rng(7)
    if kind == "structured":
        centres = rng.normal(0, 1, (k, dim))
        member = rng.integers(0, k, count)
        emb = centres[member] + 0.8 * rng.normal(0, 1, (count, dim))
        cent = centres + 0.25 * rng.normal(0, 1, (k, dim))
    else:
        emb = rng.uniform(-1, 1, (count, dim))
        cent = 0.5 * emb[rng.choice(count, k, replace=False)]
    vids = rng.permutation(count).astype(np.uint32)
    return emb.astype(F32), cent.astype(F32), vids


def planted_partition(clusters=8, per=64, dim=64, seed=7):
    """Integer rows: cluster c sits at 256 e_c, its rows add entries in [-1, 1], so two centres are
    362 apart and a row is about 7 from its own; (emb, truth)."""
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(clusters), per)
    emb = rng.integers(-1, 2, (clusters * per, dim)).astype(F32)
    emb[np.arange(len(truth)), truth] += 256
    order = rng.permutation(len(truth))
    return np.ascontiguousarray(emb[order]), truth[order].astype(np.uint32)
