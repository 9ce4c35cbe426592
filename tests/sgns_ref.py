"""numpy restatement of the skip-gram semantics of DESIGN.md §10 (TEST INFRASTRUCTURE ONLY).

Written from that section, not from the kernel: the alias-table distribution,
the two Philox streams of a centre, and the centre update in list order, in
float64 and in float32 (numpy's own summation and exp).
"""
from __future__ import annotations

import numpy as np

SENT = 0xFFFFFFFE
DROPPED = 0xFFFFFFFF
STREAM_WINDOW, STREAM_NEGATIVE = 4, 5
_M = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123) on arrays: returns (x0, x1, x2, x3) as uint64 arrays below 2^32.
    Checked against oracle.oracle.philox4x32_10 in tests/test_sgns_cpu.py."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M
    return c0, c1, c2, c3


def alias_distribution(thr, alias):
    """P(v) of the table: (thr[v]/2^32 + sum over i != v with alias[i] == v of (1 - thr[i]/2^32)) / n."""
    thr = np.asarray(thr, dtype=np.float64) / 2.0**32
    alias = np.asarray(alias, dtype=np.int64)
    n = len(thr)
    P = thr.copy()
    other = alias != np.arange(n)
    np.add.at(P, alias[other], 1.0 - thr[other])
    return P / n


def walk_lengths(rows):
    """Vertices in front of the first SENT of each walk-major row."""
    rows = np.asarray(rows)
    return np.where((rows == SENT).any(axis=1), (rows == SENT).argmax(axis=1), rows.shape[1])


def draws(rows, wids, seed, pass_, window, K, thr=None, alias=None):
    """The draws of every centre of the listed walks: u32 [m, L, 1 + K].
    rows: [m, L] walk-major, SENT-padded; wids: their global walk ids.
    Entry 0 is b (0 where pos >= len); the rest are the negatives (DROPPED when equal to the
    centre, and where pos >= len)."""
    rows = np.asarray(rows, dtype=np.uint32)
    m, L = rows.shape
    wid = np.asarray(wids, dtype=np.uint64).reshape(m, 1)
    pos = np.arange(L, dtype=np.uint64).reshape(1, L)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    live = pos < walk_lengths(rows).reshape(m, 1)
    out = np.zeros((m, L, 1 + K), dtype=np.uint32)
    x0, _, _, _ = philox4x32_10(wid & _M, wid >> np.uint64(32), pos, (pass_ << 4) | STREAM_WINDOW, k0, k1)
    b = np.uint64(1) + ((x0 * np.uint64(window)) >> np.uint64(32))
    out[:, :, 0] = np.where(live, b, 0)
    if K:
        n = np.uint64(len(thr))
        thr = np.asarray(thr, dtype=np.uint64)
        alias = np.asarray(alias, dtype=np.uint64)
    for j in range(K):
        x = philox4x32_10(wid & _M, wid >> np.uint64(32), pos | np.uint64((j >> 1) << 8),
                          (pass_ << 4) | STREAM_NEGATIVE, k0, k1)
        xa, xb = (x[2], x[3]) if j & 1 else (x[0], x[1])
        i = (xa * n) >> np.uint64(32)
        v = np.where(xb < thr[i], i, alias[i])
        out[:, :, 1 + j] = np.where(live & (v != rows), v, DROPPED)
    return out


def _softplus(x):
    """-log sigma(-x) = log(1 + e^x), stable, in x's precision."""
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def train(rows, samples, emb_in, emb_out, lr, dtype=np.float64):
    """One serial pass in list order, in place on emb_in / emb_out (arrays of `dtype`).
    Returns (loss, terms, centres); the loss terms are computed in `dtype` and summed in float64."""
    assert emb_in.dtype == dtype and emb_out.dtype == dtype
    lr = dtype(lr)
    one = dtype(1)
    lens = walk_lengths(rows)
    loss, terms, centres = 0.0, 0, 0
    rows = np.asarray(rows).astype(np.int64)
    samples = np.asarray(samples).astype(np.int64)
    with np.errstate(over="ignore"):
        for w in range(rows.shape[0]):
            n_w = int(lens[w])
            row = rows[w]
            for pos in range(n_w):
                centres += 1
                s = samples[w, pos]
                b = int(s[0])
                q0, q1 = max(pos - b, 0), min(pos + b, n_w - 1)
                ctx = np.concatenate((row[q0:pos], row[pos + 1:q1 + 1]))       # ascending q, q != pos
                if len(ctx) == 0:
                    continue
                neg = s[1:]
                tgt = np.concatenate((row[pos:pos + 1], neg[neg != DROPPED]))  # t_0 = the centre, label 1
                O = emb_out[tgt]                                               # every read ...
                H = emb_in[ctx]
                F = H @ O.T                                                    # f[u, k] = h_u . O_k
                label = np.zeros(len(tgt), dtype=dtype)
                label[0] = one
                G = lr * (label - one / (one + np.exp(-F)))
                sign = np.where(label > 0, one, -one)
                loss += float(_softplus(-(F * sign)).astype(np.float64).sum())   # -log sigma(+-f)
                terms += F.size
                dO = G.T @ H
                dH = G @ O
                np.add.at(emb_in, ctx, dH)                                     # ... precedes every write;
                np.add.at(emb_out, tgt, dO)                                    # duplicates each make their own add
    return loss, terms, centres


# ---------------------------------------------------------------------------
# the planted-partition graph of the convergence tests
# ---------------------------------------------------------------------------
def planted_graph(communities=8, size=32, inner=6, outer=1, seed=1234):
    """(offsets u64[n+1], targets u32[m], community[n]): per vertex `inner` random in-community
    edges and `outer` random edges, undirected, no self loops."""
    rng = np.random.default_rng(seed)
    n = communities * size
    comm = np.arange(n) // size
    pairs = set()
    for v in range(n):
        for _ in range(inner):
            u = int(comm[v] * size + rng.integers(size))
            if u != v:
                pairs.add((v, u))
                pairs.add((u, v))
        for _ in range(outer):
            u = int(rng.integers(n))
            if u != v:
                pairs.add((v, u))
                pairs.add((u, v))
    e = np.array(sorted(pairs), dtype=np.int64)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=off[1:])
    return off, e[:, 1].astype(np.uint32), comm


def uniform_walks(off, adj, wpv, L, seed=99):
    """[n * wpv, L] uniform random walks with numpy's generator; walk r * n + v starts at v."""
    rng = np.random.default_rng(seed)
    n = len(off) - 1
    off = off.astype(np.int64)
    rows = np.full((n * wpv, L), SENT, dtype=np.uint32)
    for w in range(n * wpv):
        v = w % n
        for p in range(L):
            rows[w, p] = v
            d = off[v + 1] - off[v]
            if d == 0:
                break
            v = int(adj[off[v] + rng.integers(d)])
    return rows


def cosine_gap(emb, comm):
    """(mean cosine between different rows of one community, mean cosine across communities)."""
    e = np.asarray(emb, dtype=np.float64)
    e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    c = e @ e.T
    same = comm[:, None] == comm[None, :]
    off_diag = ~np.eye(len(comm), dtype=bool)
    return float(c[same & off_diag].mean()), float(c[~same].mean())


def word2vec_init(n, dim, seed=7, dtype=np.float64):
    """emb_in uniform in +-0.5/dim, emb_out zero."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, dim)) - 0.5) / dim).astype(dtype), np.zeros((n, dim), dtype=dtype)
