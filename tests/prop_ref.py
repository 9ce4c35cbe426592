"""The contract of wharf_graph_propagate (include/wharf_gpu.h) restated in numpy on a
plain CSR, and the graph and features the propagation tests share.

ref32 follows the seven steps literally in float32: numpy's float32 multiply and add are single
round-to-nearest operations, the bits of __fmul_rn / __fadd_rn.  ref64 is the same sum in float64 and
bound() the first-order distance allowed between the two.
"""
import numpy as np

CHUNK = 512
F32 = np.float32


def _rows(n, vids):
    return np.arange(n, dtype=np.int64) if vids is None else np.asarray(vids, dtype=np.int64).reshape(-1)


def ref32(off, adj, x, wsrc=None, wdst=None, resid=None, alpha=1.0, beta=0.0, self_=False, vids=None):
    x = np.ascontiguousarray(x, dtype=F32)
    dim = x.shape[1]
    rows = _rows(x.shape[0], vids)
    alpha, beta = F32(alpha), F32(beta)
    out = np.empty((len(rows), dim), dtype=F32)
    done = {}
    for i, v in enumerate(rows):
        if v in done:                                   # a repeated id: the same inputs, the same row
            out[i] = out[done[v]]
            continue
        done[v] = i
        us = adj[int(off[v]):int(off[v + 1])].astype(np.int64)
        t = x[us] if wsrc is None else wsrc[us].astype(F32)[:, None] * x[us]             # step 1
        parts = []
        for c0 in range(0, len(us), CHUNK):                                              # steps 2, 3
            acc = np.zeros(dim, dtype=F32)
            for e in range(c0, min(len(us), c0 + CHUNK)):
                acc = acc + t[e]
            parts.append(acc)
        A = parts[0] if parts else np.zeros(dim, dtype=F32)                              # step 4
        for p in parts[1:]:
            A = A + p
        if self_:                                                                        # step 5
            A = A + (x[v] if wsrc is None else F32(wsrc[v]) * x[v])
        y = A if wdst is None else F32(wdst[v]) * A                                      # step 6
        o = alpha * y                                                                    # step 7
        if resid is not None:
            o = o + beta * resid[v].astype(F32)
        assert o.dtype == F32
        out[i] = o
    return out


def ref64(off, adj, x, wsrc=None, wdst=None, resid=None, alpha=1.0, beta=0.0, self_=False, vids=None):
    """(the float64 value, the magnitude sum S, the number of terms d) per output element / row."""
    x64 = np.asarray(x, dtype=F32).astype(np.float64)
    rows = _rows(x64.shape[0], vids)
    alpha, beta = float(F32(alpha)), float(F32(beta))
    ws = None if wsrc is None else np.asarray(wsrc, dtype=F32).astype(np.float64)
    wd = None if wdst is None else np.asarray(wdst, dtype=F32).astype(np.float64)
    val = np.empty((len(rows), x64.shape[1]))
    mag = np.empty_like(val)
    terms = np.empty(len(rows), dtype=np.int64)
    for i, v in enumerate(rows):
        us = adj[int(off[v]):int(off[v + 1])].astype(np.int64)
        if self_:
            us = np.append(us, v)
        t = x64[us] if ws is None else ws[us][:, None] * x64[us]
        a = alpha * (1.0 if wd is None else wd[v])
        val[i] = a * t.sum(axis=0)
        mag[i] = abs(a) * np.abs(t).sum(axis=0)
        if resid is not None:
            r = beta * np.asarray(resid[v], dtype=F32).astype(np.float64)
            val[i] += r
            mag[i] += np.abs(r)
        terms[i] = len(us)
    return val, mag, terms


def bound(mag, terms):
    """1.01 (d + 5) 2^-24 S: a term passes one multiply, at most d - 1 chain adds together with the
    chunk combines, and the three closing operations; first order in 2^-24."""
    return 1.01 * (terms[:, None] + 5) * 2.0 ** -24 * mag


# ---- the shared case ------------------------------------------------------------------------

N = 1403
HUB, ONE_CHUNK, CHUNK_PLUS_ONE = 0, 1399, 1398


def build_graph(extra_edges):
    """(off u64 [N + 1], adj u32): symmetric; vertex 0 adjacent to 1..1300 (chunks of 512, 512, 276), 1399
    to 1..512 (one chunk exactly), 1398 to 1..513 (a chunk plus one), 1400..1402 isolated, and the given
    edges (generate_batch_of_edges(2000, 1398, 3, False, False)) among the ids 1..1397."""
    e = np.asarray(extra_edges, dtype=np.int64).reshape(-1, 2)
    e = e[(e >= 1).all(axis=1) & (e <= 1397).all(axis=1) & (e[:, 0] != e[:, 1])]
    star = lambda c, hi: np.stack([np.full(hi, c, dtype=np.int64), np.arange(1, hi + 1, dtype=np.int64)], axis=1)
    e = np.concatenate([e, star(HUB, 1300), star(ONE_CHUNK, 512), star(CHUNK_PLUS_ONE, 513)])
    e = np.unique(np.concatenate([e, e[:, ::-1]]), axis=0)          # both directions, sorted by (src, dst)
    off = np.zeros(N + 1, dtype=np.uint64)
    np.cumsum(np.bincount(e[:, 0], minlength=N), out=off[1:])
    return off, np.ascontiguousarray(e[:, 1], dtype=np.uint32)


def features(dim, seed=0, n=N):
    """normal * 2^randint(-8, 8) per element: any change of the summation order shows in the bits."""
    rng = np.random.default_rng(1000 + 17 * dim + seed)
    return (rng.standard_normal((n, dim)) * 2.0 ** rng.integers(-8, 9, (n, dim))).astype(F32)


def weights(off, norm, self_):
    """(wsrc, wdst) of GraphPropagation: float64, cast to float32, 0 where the denominator is."""
    den = np.diff(off.astype(np.int64)).astype(np.float64) + (1.0 if self_ else 0.0)
    if norm == "sum":
        return None, None
    w = np.where(den > 0, np.where(den > 0, den, 1.0) ** (-0.5 if norm == "sym" else -1.0), 0.0).astype(F32)
    return (w, w) if norm == "sym" else (None, w)


def id_list(count=777, seed=5):
    """Unordered, with repeats, containing the hub, 1398, 1399 and an isolated vertex."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, N, count).astype(np.uint32)
    ids[[3, 100, 101, 500, 776]] = [HUB, CHUNK_PLUS_ONE, ONE_CHUNK, 1401, HUB]
    return ids
