"""GPU tests of the clustering stage against the numpy restatement tests/kmeans_ref.py.

Assignments, scores, inertia, counts and updated centroids on integer tables are compared bit for
bit.  Float results are held to the derived bounds of §13 (kmeans_ref.score_bound / inertia_bound /
centroid_bound), never to a measured one; every comparison prints its measured ratio to the bound
before it asserts.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID, E_RANGE = -1, -5
PLANT_ID, PLANT_SCORE, PLANT_INERTIA, PLANT_COUNT = 0x5A5A5A5A, np.float32(-7.25), -3.5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def W():
    import dynamicgraphrepresentationlearning_amd as W
    return W


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture
def g(W):
    # an empty handle: the passes need its device and stream only (conftest frees it after the test)
    return W.WharfMH(16)


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def kparams(dim, k, flags=0, reserved=0):
    from dynamicgraphrepresentationlearning_amd import _lib as L
    p = L.wharf_kmeans_params()
    p.dim, p.k, p.flags, p.reserved = dim, k, flags, reserved
    return p


def raw_norms(torch, g, emb):
    from dynamicgraphrepresentationlearning_amd import _lib as L
    out = torch.empty(emb.shape[0], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.lib.wharf_emb_row_norms(g._h, ptr(emb), emb.shape[0], emb.shape[1], ptr(out)) == 0
    return out


def raw_assign(torch, g, emb, cent, vids=None, rnorm=None, dim=None, k=None, n=None, count=None, flags=0, reserved=0,
               null=(), want_score=True, want_inertia=True):
    """(rc, assign u32, score f32, inertia); emb, cent, rnorm: device tensors; vids: numpy or None.  The
    outputs hold a planted pattern before the call."""
    from dynamicgraphrepresentationlearning_amd import _lib as L
    vd = None if vids is None else dev(torch, np.asarray(vids, np.uint32))
    rows = emb.shape[0] if vids is None else len(vids)
    assign = torch.full((max(rows, 1),), PLANT_ID, dtype=torch.int32, device="cuda")
    score = torch.full((max(rows, 1),), float(PLANT_SCORE), dtype=torch.float32, device="cuda")
    inertia = C.c_double(PLANT_INERTIA)
    p = kparams(emb.shape[1] if dim is None else dim, cent.shape[0] if k is None else k, flags, reserved)
    args = dict(emb=ptr(emb), cent=ptr(cent), assign=ptr(assign), params=C.byref(p))
    for name in null:
        args[name] = None
    torch.cuda.synchronize()
    rc = L.lib.wharf_kmeans_assign(g._h, args["params"], args["emb"], emb.shape[0] if n is None else n, ptr(rnorm),
                                   ptr(vd), rows if count is None else count, args["cent"], args["assign"],
                                   ptr(score) if want_score else None, C.byref(inertia) if want_inertia else None)
    return rc, assign.cpu().numpy().view(np.uint32)[:rows], score.cpu().numpy()[:rows], inertia.value


def raw_update(torch, g, emb, cent, assign, vids=None, rnorm=None, dim=None, k=None, n=None, count=None, flags=0,
               reserved=0, null=()):
    """(rc, centroids after the call, counts u64); cent: numpy, copied to the device for the call."""
    from dynamicgraphrepresentationlearning_amd import _lib as L
    vd = None if vids is None else dev(torch, np.asarray(vids, np.uint32))
    ad = dev(torch, np.asarray(assign, np.uint32))
    cd = dev(torch, cent)
    rows = len(assign)
    kk = cent.shape[0] if k is None else k
    counts = np.full(max(kk, cent.shape[0]), PLANT_COUNT, dtype=np.uint64)
    p = kparams(emb.shape[1] if dim is None else dim, kk, flags, reserved)
    args = dict(emb=ptr(emb), cent=ptr(cd), assign=ptr(ad), counts=counts.ctypes.data_as(C.c_void_p), params=C.byref(p))
    for name in null:
        args[name] = None
    torch.cuda.synchronize()
    rc = L.lib.wharf_kmeans_update(g._h, args["params"], args["emb"], emb.shape[0] if n is None else n, ptr(rnorm),
                                   ptr(vd), rows if count is None else count, args["assign"], args["cent"],
                                   args["counts"])
    return rc, cd.cpu().numpy(), counts[:kk]


def exact_reference(x, cent, r=None):
    """Integer data: every product, partial sum and score is exact, so float64 arithmetic rounded once
    to float32 is the chain (tests/test_cluster_cpu.py holds kmeans_ref.scores32 to that)."""
    s = R.scores64(x, cent, r).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), R.scores64(x, cent, r))
    s = (s + np.float32(0)).astype(np.float32)
    a, best = R.assign_of(s)
    inertia = float((R.xx64(x, r) - 2.0 * best.astype(np.float64)).sum())
    sums, _, counts = R.sums64(x, a, len(cent), r)
    want = cent.copy()
    nz = counts > 0
    want[nz] = (sums[nz].astype(np.float32) / counts[nz].astype(np.float32)[:, None]).astype(np.float32)
    assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)
    return a, best, inertia, counts, want


def check_exact(torch, g, name, emb, cent, vids, r=None):
    x = emb if vids is None else emb[vids]
    rr = None if r is None else (r if vids is None else r[vids])
    a, best, inertia, counts, want = exact_reference(x, cent, rr)
    de, dc, dr = dev(torch, emb), dev(torch, cent), None if r is None else dev(torch, r)
    rc, ga, gs, gi = raw_assign(torch, g, de, dc, vids, dr)
    assert rc == 0, name
    np.testing.assert_array_equal(ga, a, err_msg=name)
    np.testing.assert_array_equal(bits(gs), bits(best), err_msg=name)
    assert gi == inertia, (name, gi, inertia)
    rc, gc, gn = raw_update(torch, g, de, cent, ga, vids, dr)
    assert rc == 0, name
    np.testing.assert_array_equal(gn, counts, err_msg=name)
    np.testing.assert_array_equal(bits(gc), bits(want), err_msg=name)


# 1. ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128, 192, 256])
def test_integer_tables_match_bit_for_bit(torch, g, dim):
    cases = 0
    for k in (1, 2, 7, 32, 33, 256):
        for count in (1, 31, 33, 65, 257):
            emb, cent, vids = R.integer_case(count, dim, k)
            check_exact(torch, g, f"dim {dim} k {k} count {count} vids", emb, cent, vids)
            check_exact(torch, g, f"dim {dim} k {k} count {count} all rows", emb, cent, None)
            cases += 2
    # rnorm as data: exact factors
    emb, cent, vids = R.integer_case(257, dim, 33)
    r = np.random.default_rng(dim).choice(np.array([0.5, 1.0, 2.0], np.float32), len(emb))
    check_exact(torch, g, f"dim {dim} rnorm", emb, cent, vids, r)
    check_exact(torch, g, f"dim {dim} rnorm all rows", emb, cent, None, r)
    print(f"dim {dim}: {cases + 2} cases bit for bit")


# 2. ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128, 256])
def test_operand_map_on_asymmetric_onehot_tables(torch, g, dim):
    emb, cent = R.onehot_case(300, dim, 70)
    s = R.scores32(emb, cent)
    a, best = R.assign_of(s)
    rc, ga, gs, gi = raw_assign(torch, g, dev(torch, emb), dev(torch, cent))
    assert rc == 0
    print(f"dim {dim}: {len(set(a.tolist()))} distinct centroids assigned, {int((best > -1).sum())} rows meet their centroid's axis")
    np.testing.assert_array_equal(ga, a)
    np.testing.assert_array_equal(bits(gs), bits(best))
    assert gi == R.inertia_of(R.xx32(emb), best)


# 3. ------------------------------------------------------------------------------------------
def test_ties_take_the_lowest_id(torch, g):
    dim = 64
    emb, cent, _ = R.integer_case(200, dim, 40)
    cent[5], cent[39], cent[17] = cent[2], cent[2], cent[11]            # duplicate centroids
    cent[0] = 0
    cent[0, 0] = 2                                                      # 2 e_0
    cent[1] = 0
    cent[1, 1] = 2                                                      # 2 e_1
    emb[0] = 0
    emb[0, :2] = 1                                                      # level between centroids 0 and 1
    check_exact(torch, g, "duplicates", emb, cent, None)
    a = exact_reference(emb, cent)[0]
    assert not np.isin(a, [5, 39, 17]).any() and a[0] == 0
    # -0 and +0: with r = -1 the zero centroids 0 and 1 score -0, centroid 2 scores (-2)(-1) - 2 = +0
    cent = np.zeros((3, dim), np.float32)
    cent[2, 0] = 2
    emb = np.zeros((40, dim), np.float32)
    emb[:, 0] = -1
    r = np.full(40, -1, np.float32)
    s = (R.chain32(emb[:, None, :], cent[None]) * r[:, None]).astype(np.float32) - R.hn32(cent)[None]
    assert (np.signbit(s[:, :2])).all() and not np.signbit(s[:, 2]).any() and (s == 0).all()
    rc, ga, gs, gi = raw_assign(torch, g, dev(torch, emb), dev(torch, cent), None, dev(torch, r))
    assert rc == 0
    assert (ga == 0).all() and (bits(gs) == 0).all()                    # the lowest id, reported as +0
    assert gi == 40.0


# 4. ------------------------------------------------------------------------------------------
def test_empty_clusters_keep_their_centroid(torch, g):
    dim, k = 128, 9
    emb, cent, vids = R.integer_case(100, dim, k)
    cent[4] = np.float32(-0.0)
    cent[7, ::2] = np.float32(1e-41)                                    # a subnormal keeps its bits too
    assign = np.array([0, 1, 2, 3, 5, 6, 8], np.uint32)[np.random.default_rng(3).integers(0, 7, 100)]
    rc, gc, gn = raw_update(torch, g, dev(torch, emb), cent, assign, vids)
    assert rc == 0
    assert gn[4] == 0 and gn[7] == 0 and gn.sum() == 100
    np.testing.assert_array_equal(bits(gc[[4, 7]]), bits(cent[[4, 7]]))
    sums, _, counts = R.sums64(emb[vids], assign, k)
    nz = counts > 0
    np.testing.assert_array_equal(gn, counts)
    np.testing.assert_array_equal(bits(gc[nz]), bits(sums[nz].astype(np.float32) / counts[nz].astype(np.float32)[:, None]))


# 5. ------------------------------------------------------------------------------------------
_float_refs = {}


def float_ref(kind, shape):
    """A case's inputs, computed once and left unchanged."""
    if (kind, shape) not in _float_refs:
        emb, cent, vids = R.float_case(kind, *shape)
        for a in (emb, cent, vids):
            a.setflags(write=False)
        _float_refs[(kind, shape)] = (emb, cent, vids)
    return _float_refs[(kind, shape)]


@pytest.mark.parametrize("with_rnorm", [False, True], ids=["plain", "rnorm"])
@pytest.mark.parametrize("kind", ["structured", "unstructured"])
@pytest.mark.parametrize("shape", R.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_tables_are_within_the_bounds(torch, g, shape, kind, with_rnorm):
    count, dim, k = shape
    emb, cent, vids = float_ref(kind, shape)
    name = f"{kind} {shape} rnorm {with_rnorm}"
    de, dc = dev(torch, emb), dev(torch, cent)
    dr = raw_norms(torch, g, de) if with_rnorm else None
    x = emb[vids]
    r = dr.cpu().numpy()[vids] if with_rnorm else None                  # the contract treats rnorm as data
    s64, bound = R.scores64(x, cent, r), R.score_bound(x, cent, r)
    rc, ga, gs, gi = raw_assign(torch, g, de, dc, vids, dr)
    assert rc == 0
    rows = np.arange(count)
    assert (ga < k).all()
    ratio = float((np.abs(gs.astype(np.float64) - s64[rows, ga]) / bound[rows, ga]).max())
    dec, allowed = R.decisive(s64, bound)
    print(f"{name}: score err / bound {ratio:.3f}; {int((~dec).sum())} of {count} rows indecisive")
    assert ratio <= 1.0, name
    assert (~dec).sum() <= 0.01 * count, name
    np.testing.assert_array_equal(ga[dec], np.argmax(s64, axis=1)[dec], err_msg=name)
    assert allowed[rows, ga].all(), name
    i64 = float((R.xx64(x, r) - 2.0 * s64[rows, ga]).sum())
    ib = R.inertia_bound(x, cent, ga, r)
    print(f"  inertia {gi:.6f}: err / bound {abs(gi - i64) / ib:.3f}")
    assert abs(gi - i64) <= ib, name
    rc, gc, gn = raw_update(torch, g, de, cent, ga, vids, dr)
    assert rc == 0
    sums, mags, counts = R.sums64(x, ga, k, r)
    np.testing.assert_array_equal(gn, counts, err_msg=name)
    nz = counts > 0
    c64 = sums[nz] / counts[nz].astype(np.float64)[:, None]
    cb = R.centroid_bound(mags[nz], counts[nz], c64)
    err = np.abs(gc[nz].astype(np.float64) - c64)
    print(f"  centroid err / bound {float((err / cb).max()):.3f}; {int((~nz).sum())} empty clusters")
    assert (err <= cb).all(), name
    np.testing.assert_array_equal(bits(gc[~nz]), bits(cent[~nz]), err_msg=name)
    if kind == "structured" and with_rnorm:   # tests/test_cluster_cpu.py: which cases hold empty clusters
        assert int((~nz).sum()) == {7: 1, 2: 0, 17: 14, 64: 59, 256: 223}[k], name


# 6. ------------------------------------------------------------------------------------------
def test_three_calls_give_the_same_bits(torch, g):
    emb, cent, vids = float_ref("unstructured", (4097, 192, 64))
    de, dc = dev(torch, emb), dev(torch, cent)
    dr = raw_norms(torch, g, de)
    others = [float_ref("structured", (1100, 128, 17)), float_ref("structured", (65, 64, 7))]
    runs = []
    for i in range(3):
        rc, ga, gs, gi = raw_assign(torch, g, de, dc, vids, dr)
        rc2, gc, gn = raw_update(torch, g, de, cent, ga, vids, dr)
        assert rc == 0 and rc2 == 0
        runs.append([ga, bits(gs), np.array([gi]).view(np.uint64), bits(gc), gn])
        if i < 2:
            oe, oc, ov = others[i]
            rc, oa, _, _ = raw_assign(torch, g, dev(torch, oe), dev(torch, oc), ov)
            assert rc == 0 and raw_update(torch, g, dev(torch, oe), oc, oa, ov)[0] == 0
    for run in runs[1:]:
        for a, b in zip(runs[0], run):
            np.testing.assert_array_equal(a, b)


# 7. ------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(W, torch, g):
    from dynamicgraphrepresentationlearning_amd import _lib as L
    emb, cent, vids = float_ref("structured", (333, 64, 2))
    n = len(emb)
    de, dc = dev(torch, emb), dev(torch, cent)
    bad = vids.copy()
    bad[40] = n
    cases = [
        ("id >= n", E_RANGE, dict(vids=bad)),
        ("dim 96", E_INVALID, dict(dim=96)),
        ("dim 320", E_INVALID, dict(dim=320)),
        ("dim 0", E_INVALID, dict(dim=0)),
        ("k 0", E_INVALID, dict(k=0)),
        ("k 257", E_INVALID, dict(k=257)),
        ("flags", E_INVALID, dict(flags=1)),
        ("reserved", E_INVALID, dict(reserved=1)),
        ("null emb", E_INVALID, dict(null=("emb",))),
        ("null centroids", E_INVALID, dict(null=("cent",))),
        ("null params", E_INVALID, dict(null=("params",))),
        ("count 0 with a list", E_INVALID, dict(count=0)),
        ("n 0", E_INVALID, dict(n=0)),
    ]
    for name, code, kw in cases:
        args = dict(vids=vids)
        args.update(kw)
        rc, ga, gs, gi = raw_assign(torch, g, de, dc, **args)
        assert rc == code, (name, rc, L.last_error(g._h))
        assert (ga == PLANT_ID).all() and (gs == PLANT_SCORE).all() and gi == PLANT_INERTIA, name
        assert L.last_error(g._h), name
    assert raw_assign(torch, g, de, dc, vids, null=("assign",))[0] == E_INVALID
    rc, ga, _, _ = raw_assign(torch, g, de, dc, vids, want_score=False, want_inertia=False)   # both optional
    assert rc == 0 and (ga < 2).all()

    assign = (np.arange(len(vids)) % 2).astype(np.uint32)
    worse = assign.copy()
    worse[100] = 2
    cases = [
        ("id >= n", E_RANGE, dict(vids=bad)),
        ("assignment >= k", E_RANGE, dict(assign=worse)),
        ("assignment >= k, all rows", E_RANGE, dict(assign=worse, vids=None)),
        ("dim 96", E_INVALID, dict(dim=96)),
        ("k 0", E_INVALID, dict(k=0)),
        ("k 257", E_INVALID, dict(k=257)),
        ("flags", E_INVALID, dict(flags=2)),
        ("reserved", E_INVALID, dict(reserved=7)),
        ("null emb", E_INVALID, dict(null=("emb",))),
        ("null assign", E_INVALID, dict(null=("assign",))),
        ("null centroids", E_INVALID, dict(null=("cent",))),
        ("null counts", E_INVALID, dict(null=("counts",))),
        ("count 0 with a list", E_INVALID, dict(count=0)),
    ]
    for name, code, kw in cases:
        args = dict(assign=assign, vids=vids)
        args.update(kw)
        rc, gc, gn = raw_update(torch, g, de, cent, **args)
        assert rc == code, (name, rc, L.last_error(g._h))
        np.testing.assert_array_equal(bits(gc), bits(cent), err_msg=name)
        assert (gn == PLANT_COUNT).all(), name

    # partition statistics: g has 16 vertices and no edges
    part = np.zeros(16, np.uint32)
    intra, vol = g.partition_stats(part, 3)
    assert not intra.any() and not vol.any()
    pd = dev(torch, part)
    out = np.full(8, PLANT_COUNT, np.uint64)
    o = out.ctypes.data_as(C.c_void_p)
    stats = L.lib.wharf_partition_stats
    part[9] = 3
    assert stats(g._h, ptr(dev(torch, part)), 16, 3, o, o) == E_RANGE
    assert stats(g._h, ptr(pd), 15, 3, o, o) == E_INVALID                  # n other than the handle's
    assert stats(g._h, ptr(pd), 16, 0, o, o) == E_INVALID
    assert stats(g._h, ptr(pd), 16, 65537, o, o) == E_INVALID
    assert stats(g._h, None, 16, 3, o, o) == E_INVALID
    assert stats(g._h, ptr(pd), 16, 3, None, o) == E_INVALID
    assert (out == PLANT_COUNT).all()
    with pytest.raises(RuntimeError):
        g.partition_stats(part, 3)


# 8. ------------------------------------------------------------------------------------------
def test_partition_stats_follow_the_graph(W, torch):
    n = 512
    g = W.WharfMH.from_rmat(n, 3000, 1024, seed=1, config=W.WharfConfig(walks_per_vertex=1, walk_length=5))
    g.generate_initial_random_walks()
    rng = np.random.default_rng(7)
    parts = {k: rng.integers(0, min(k, 4000), n).astype(np.uint32) for k in (1, 5, 65536)}
    parts[65536][:3] = (65535, 0, 65535)
    batch = W.generate_batch_of_edges(400, n, 3, False, False)

    def compare(stage):
        off, adj = g.flatten_graph()
        for k, part in parts.items():
            want_intra, want_vol = R.partition_stats(off, adj, part, k)
            intra, vol = g.partition_stats(part, k)
            np.testing.assert_array_equal(intra, want_intra, err_msg=f"{stage} k {k}")
            np.testing.assert_array_equal(vol, want_vol, err_msg=f"{stage} k {k}")
            assert int(vol.sum()) == g.number_of_edges() == len(adj), stage
            ti, tv = g.partition_stats(dev(torch, part), k)                   # a device tensor
            assert np.array_equal(ti, intra) and np.array_equal(tv, vol)
            assert W.modularity(g, part, k) == R.modularity(want_intra, want_vol)
        print(f"{stage}: {len(adj)} slots, Q(k = 5) = {W.modularity(g, parts[5], 5):.6f}")
        return len(adj)

    m0 = compare("base graph")
    g.insert_edges_batch(batch)
    moved = g.stats()["last_moved_row_slots"]
    print(f"the insert relocated rows into {moved} slots")
    assert moved > 0
    assert compare("after the insert") > m0
    g.delete_edges_batch(batch)
    compare("after the delete")
    assert g.stats()["rev_fallbacks"] == 0

    off, adj = R.two_triangles()
    t = W.WharfMH.from_csr(off, adj)
    part = np.array([0, 0, 0, 1, 1, 1], np.uint32)
    intra, vol = t.partition_stats(part, 2)
    assert list(intra) == [6, 6] and list(vol) == [7, 7]
    assert W.modularity(t, part) == 5 / 14
    assert W.modularity(t, dev(torch, part), 2) == 5 / 14


# 9. ------------------------------------------------------------------------------------------
def test_python_fit_predict_and_warm_start(W, torch, g):
    emb, truth = R.planted_partition()
    t = dev(torch, emb)
    km = W.VertexClustering(g, 64, 8)
    row = km.fit(t, seed=0)
    hist = row["history"]
    print(f"planted partition: {row['iterations']} iterations, inertia {hist}")
    assert row["converged"] and row["iterations"] < 100
    assert W.nmi(truth, km.labels) == 1.0
    assert all(b <= a for a, b in zip(hist, hist[1:])) and row["inertia"] == hist[-1]
    assert list(row["counts"]) == [64] * 8 and row["counts"].dtype == np.uint64
    assert km.centroids.shape == (8, 64) and km.centroids.dtype == torch.float32 and km.centroids.is_cuda
    labels, cents = km.labels.clone(), km.centroids.clone()
    assert torch.equal(km.predict(t), labels)
    # the inertia is the rows' squared distances to their cluster's mean, within the bound (the means are
    # multiples of 1/64: hn is not exact in float32)
    x = emb.astype(np.float64)
    a = labels.cpu().numpy()
    c = cents.cpu().numpy()
    want = float(((x - c.astype(np.float64)[a]) ** 2).sum())
    ib = R.inertia_bound(emb, c, a)
    print(f"inertia {row['inertia']} against {want}: err / bound {abs(row['inertia'] - want) / ib:.3f}")
    assert abs(row["inertia"] - want) <= ib
    # a warm start from its own centroids: one update, which changes nothing
    warm = W.VertexClustering(g, 64, 8)
    row2 = warm.fit(t, init=cents)
    assert row2["converged"] and row2["iterations"] == 1
    assert torch.equal(warm.labels, labels) and torch.equal(warm.centroids, cents) and row2["inertia"] == row["inertia"]
    # seed reproduces fit bit for bit; another seed starts elsewhere and still finds the partition
    again = W.VertexClustering(g, 64, 8)
    row3 = again.fit(t, seed=0)
    assert torch.equal(again.labels, labels) and torch.equal(again.centroids, cents) and row3["history"] == hist
    for init in ("sample", "kmeans++"):
        other = W.VertexClustering(g, 64, 8)
        row4 = other.fit(t, init=init, seed=5)
        print(f"{init}, seed 5: {row4['iterations']} iterations, NMI {W.nmi(truth, other.labels):.3f}")
        assert row4["history"] == sorted(row4["history"], reverse=True)
    # a list of vertices: the labels are the list's
    ids = np.arange(0, 512, 2, dtype=np.uint32)
    sub = W.VertexClustering(g, 64, 8)
    sub.fit(t, vertices=ids, seed=0)
    assert sub.labels.shape == (256,) and W.nmi(truth[ids], sub.labels) == pytest.approx(1.0, abs=1e-12)
    assert torch.equal(sub.predict(t, dev(torch, ids)), sub.labels)
    with pytest.raises(ValueError):
        km.fit(t, init="forgy")
    with pytest.raises(ValueError):
        km.fit(t, init=np.zeros((3, 64), np.float32))
    with pytest.raises(ValueError):
        km.fit(dev(torch, emb[:, :32].copy()))


def test_python_normalize_equals_a_normalised_copy(W, torch, g):
    emb, cent, _ = float_ref("unstructured", (1100, 128, 17))
    t = dev(torch, emb)
    a = W.VertexClustering(g, 128, 17, normalize=True)
    a.fit(t, init=cent, max_iter=0)
    r = a.rnorm.cpu().numpy()
    copy = (r[:, None] * emb).astype(np.float32)
    b = W.VertexClustering(g, 128, 17)
    b.fit(dev(torch, copy), init=cent, max_iter=0)
    s64, bound = R.scores64(emb, cent, r), R.score_bound(emb, cent, r)
    # the copy's scores carry one more rounding per element: its own bound, on the same float64 scores
    dec, _ = R.decisive(s64, bound + R.score_bound(copy, cent))
    la, lb = a.labels.cpu().numpy(), b.labels.cpu().numpy()
    print(f"normalize: {int((~dec).sum())} of {len(emb)} rows indecisive, {int((la != lb).sum())} labels differ")
    assert (~dec).sum() <= 0.01 * len(emb)
    np.testing.assert_array_equal(la[dec], lb[dec])
    np.testing.assert_array_equal(la[dec], np.argmax(s64, axis=1)[dec])
    # evaluate_clustering on a graph: the keys, and labels that do not matter by name
    n = 512
    gg = W.WharfMH.from_rmat(n, 3000, 1024, seed=1, config=W.WharfConfig(walks_per_vertex=1, walk_length=5))
    planted, truth = R.planted_partition()
    ids = np.arange(0, n, 3)
    row = W.evaluate_clustering(gg, dev(torch, planted), ids, truth[ids] + 10, normalize=True, seed=0)
    print(f"evaluate_clustering: {row}")
    assert set(row) == {"nmi", "modularity", "inertia", "iterations"}
    assert row["nmi"] == pytest.approx(1.0, abs=1e-12) and -0.5 <= row["modularity"] <= 1.0
