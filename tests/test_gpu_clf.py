"""GPU tests of the vertex classifier against the numpy restatement tests/clf_ref.py.

Integer outputs (predictions on decisive rows, confusion matrices) and min / max are compared bit
for bit.  Float outputs follow the rule of tests/test_gpu_sgns.py: max|gpu - ref64| <= 8 x
max|ref32 - ref64|, where ref32 / ref64 are the restatement in float32 / float64; every comparison
prints its measured ratio before it asserts.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clf_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
E_INVALID, E_RANGE = -1, -5


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
    # an empty handle: the classifier needs its device and stream only (conftest frees it after the test)
    return W.WharfMH(16)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "clf_golden.npz")))


def close(name, gpu, ref32, ref64):
    """max|gpu - ref64| <= 8 x max|ref32 - ref64| (module docstring)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    base = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())
    err = float(np.abs(np.asarray(gpu, dtype=np.float64) - ref64).max())
    print(f"{name}: max|gpu-ref64| {err:.3e}, max|ref32-ref64| {base:.3e}, ratio {err / base if base else math.inf:.3f}")
    assert np.isfinite(np.asarray(gpu, dtype=np.float64)).all(), name
    assert err <= 8 * base, name


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def problem(count, dim, C, n=300, seed=5, wscale=0.5):
    """A table, a list with repeats, labels that leave class C - 1 without rows, N(0, wscale) weights."""
    rng = np.random.default_rng(seed + count + dim + C)
    table = rng.normal(0, 1, (n, dim)).astype(np.float32)
    ids = rng.integers(0, n, count).astype(np.uint32)
    if count > 2:
        ids[-1] = ids[0]
    y = rng.integers(0, C - 1, count).astype(np.uint32)
    wb = rng.normal(0, wscale, (C, dim + 1)).astype(np.float32)
    lo, hi = R.minmax(table, np.arange(n))
    return table, ids, y, wb, lo, R.scale_of(lo, hi)


def classifier(W, torch, g, dim, C, lo, scale, wb):
    clf = W.VertexClassifier(g, dim, C)
    clf.lo, clf.scale, clf.wb = dev(torch, lo), dev(torch, scale), dev(torch, wb)
    return clf


# a. ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 256])
def test_minmax_is_exact(W, torch, g, dim):
    rng = np.random.default_rng(dim)
    table = rng.normal(0, 1, (300, dim)).astype(np.float32)
    table[:, 7] = np.float32(0.25)                      # a constant column
    emb = dev(torch, table)
    clf = W.VertexClassifier(g, dim, 2)
    for count in (1, 63, 64, 65, 1000):
        ids = rng.integers(0, 300, count).astype(np.uint32)
        if count >= 63:
            assert len(np.unique(ids)) < count          # repeats
        lo, hi = clf.minmax(emb, ids)
        rlo, rhi = R.minmax(table, ids)
        np.testing.assert_array_equal(lo.cpu().numpy(), rlo)
        np.testing.assert_array_equal(hi.cpu().numpy(), rhi)
        clf.set_scaler(lo, hi)
        np.testing.assert_array_equal(clf.scale.cpu().numpy(), R.scale_of(rlo, rhi))
        assert clf.scale[7].item() == 1.0
    lo, hi = clf.minmax(emb, dev(torch, np.arange(300, dtype=np.uint32)))   # a device id list
    np.testing.assert_array_equal(lo.cpu().numpy(), table.min(axis=0))
    np.testing.assert_array_equal(hi.cpu().numpy(), table.max(axis=0))


# b. ------------------------------------------------------------------------------------------
def check_loss_grad(W, torch, g, name, table, ids, y, wb, lo, scale):
    dim, C = table.shape[1], wb.shape[0]
    clf = classifier(W, torch, g, dim, C, lo, scale, wb)
    loss, grad = clf.loss_grad(dev(torch, table), ids, y)
    l32, g32 = R.loss_grad(table, ids, y, lo, scale, wb, np.float32)
    l64, g64 = R.loss_grad(table, ids, y, lo, scale, wb, np.float64)
    assert grad.shape == (C, dim + 1)
    close(f"{name} loss", loss, l32, l64)
    close(f"{name} grad", grad.cpu().numpy(), g32, g64)
    return loss, grad


@pytest.mark.parametrize("count,dim,C", [(1, 64, 2), (65, 64, 7), (1000, 128, 17), (333, 192, 64), (257, 256, 256),
                                         (4097, 128, 3)])
def test_loss_grad_matches_the_restatement(W, torch, g, count, dim, C):
    table, ids, y, wb, lo, scale = problem(count, dim, C)
    assert count < 3 or len(np.unique(ids)) < count
    assert not (y == C - 1).any()
    _, grad = check_loss_grad(W, torch, g, f"({count},{dim},{C})", table, ids, y, wb, lo, scale)
    # the class without rows: its gradient is sum_i p_ic (x', 1), positive in the bias
    assert grad[C - 1, dim].item() > 0


def test_loss_grad_large_logits(W, torch, g):
    table, ids, y, wb, lo, scale = problem(500, 128, 17)
    z = R.logits(table, ids, lo, scale, wb, np.float64)
    wb = (wb * np.float32(80.0 / np.abs(z).max())).astype(np.float32)
    z = R.logits(table, ids, lo, scale, wb, np.float64)
    assert 79 < np.abs(z).max() < 81 and z.max() > 40 and z.min() < -40
    check_loss_grad(W, torch, g, "logits +-80", table, ids, y, wb, lo, scale)


# c. ------------------------------------------------------------------------------------------
def test_loss_grad_is_deterministic(W, torch, g):
    table, ids, y, wb, lo, scale = problem(4097, 128, 17)
    emb = dev(torch, table)
    clf = classifier(W, torch, g, 128, 17, lo, scale, wb)
    l0, g0 = clf.loss_grad(emb, ids, y)
    l1, g1 = clf.loss_grad(emb, ids, y)
    assert l0 == l1 and torch.equal(g0, g1)
    t2, i2, y2, w2, lo2, s2 = problem(333, 192, 64)     # another shape in between: stale scratch would show
    classifier(W, torch, g, 192, 64, lo2, s2, w2).loss_grad(dev(torch, t2), i2, y2)
    t3, i3, y3, w3, lo3, s3 = problem(257, 256, 256)    # and one with tiled classes
    classifier(W, torch, g, 256, 256, lo3, s3, w3).loss_grad(dev(torch, t3), i3, y3)
    l2, g2 = clf.loss_grad(emb, ids, y)
    assert l0 == l2 and torch.equal(g0, g2)
    print(f"loss {l0!r} on three calls")


# d. ------------------------------------------------------------------------------------------
def test_predict_and_confusion(W, torch, g, gold):
    table, lo, scale = gold["table"], gold["lo"], gold["scale"]
    wb = gold["W_opt"].astype(np.float32)
    ids = np.concatenate([gold["train"], gold["test"], gold["train"][:37]]).astype(np.uint32)
    y = gold["labels"][ids]
    emb = dev(torch, table)
    clf = classifier(W, torch, g, 64, 7, lo, scale, wb)
    z32 = R.logits(table, ids, lo, scale, wb, np.float32)
    z64 = R.logits(table, ids, lo, scale, wb, np.float64)
    decisive = R.top_two_gap(z64) > 8 * np.abs(z32 - z64).max()
    print(f"decisive rows {decisive.mean():.4f} (max|z32-z64| {np.abs(z32 - z64).max():.3e})")
    assert decisive.mean() >= 0.99
    pred = clf.predict(emb, ids).cpu().numpy().astype(np.uint32)
    np.testing.assert_array_equal(pred[decisive], R.predict(z64)[decisive])
    s = clf.score(emb, dev(torch, ids), dev(torch, y))              # device lists
    np.testing.assert_array_equal(s["confusion"], R.confusion(y, pred, 7))
    assert s["confusion"].dtype == np.uint64 and s["confusion"].sum() == len(ids)
    assert s["accuracy"] == R.metrics(s["confusion"])["accuracy"]
    # two identical class rows that always win: the lower index
    tie = wb.copy()
    tie[4] = tie[2]
    tie[[2, 4], -1] += np.float32(100)
    clf.wb = dev(torch, tie)
    assert (clf.predict(emb, ids).cpu().numpy() == 2).all()


def test_predict_many_classes(W, torch, g):
    """More classes than the 16 parts of a row's argmax, more tiles than one block's."""
    table, ids, y, wb, lo, scale = problem(1000, 128, 195, wscale=0.5)
    clf = classifier(W, torch, g, 128, 195, lo, scale, wb)
    z32 = R.logits(table, ids, lo, scale, wb, np.float32)
    z64 = R.logits(table, ids, lo, scale, wb, np.float64)
    decisive = R.top_two_gap(z64) > 8 * np.abs(z32 - z64).max()
    pred = clf.predict(dev(torch, table), ids).cpu().numpy().astype(np.uint32)
    assert decisive.mean() > 0.9
    np.testing.assert_array_equal(pred[decisive], R.predict(z64)[decisive])
    s = clf.score(dev(torch, table), ids, y)
    np.testing.assert_array_equal(s["confusion"], R.confusion(y, pred, 195))


# e. ------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(W, torch, g):
    from dynamicgraphrepresentationlearning_amd import _lib as L
    n, dim, Cn, count = 300, 64, 7, 65
    table, ids, y, wb, lo, scale = problem(count, dim, Cn)
    t = {k: dev(torch, v) for k, v in dict(emb=table, ids=ids, y=y, wb=wb, lo=lo, scale=scale).items()}
    bad_id, bad_y = ids.copy(), y.copy()
    bad_id[40] = n
    bad_y[64] = Cn
    t["bad_id"], t["bad_y"] = dev(torch, bad_id), dev(torch, bad_y)
    grad = torch.full((Cn, dim + 1), 7.0, device="cuda")
    pred = torch.full((count,), -3, dtype=torch.int32, device="cuda")
    lo_out, hi_out = torch.full((dim,), 5.0, device="cuda"), torch.full((dim,), 6.0, device="cuda")
    conf = np.full((Cn, Cn), 9, dtype=np.uint64)
    loss = C.c_double(-1.0)
    P = lambda x: C.c_void_p(x.data_ptr())
    torch.cuda.synchronize()

    def params(d=dim, c=Cn):
        p = L.wharf_clf_params()
        p.dim, p.classes = d, c
        return C.byref(p)

    def loss_grad(p=None, emb="emb", ids="ids", y="y", cnt=count, wb="wb", out=grad, h=g._h, lossp=C.byref(loss)):
        return L.lib.wharf_clf_loss_grad(h, p or params(), P(t[emb]) if emb else None, n, P(t[ids]) if ids else None,
                                         P(t[y]) if y else None, cnt, P(t["lo"]), P(t["scale"]),
                                         P(t[wb]) if wb else None, P(out) if out is not None else None, lossp)

    def predict(p=None, ids="ids", y="y", cnt=count, out=pred, cm=conf):
        return L.lib.wharf_clf_predict(g._h, p or params(), P(t["emb"]), n, P(t[ids]), cnt, P(t["lo"]), P(t["scale"]),
                                       P(t["wb"]), P(t[y]) if y else None, P(out) if out is not None else None,
                                       cm.ctypes.data_as(C.c_void_p) if cm is not None else None)

    def minmax(d=dim, ids="ids", cnt=count, lo_=lo_out):
        return L.lib.wharf_clf_minmax(g._h, P(t["emb"]), n, d, P(t[ids]), cnt, P(lo_) if lo_ is not None else None,
                                      P(hi_out))

    assert loss_grad(ids="bad_id") == E_RANGE and "entry 40" in L.last_error(g._h)
    assert predict(ids="bad_id") == E_RANGE
    assert minmax(ids="bad_id") == E_RANGE
    assert loss_grad(y="bad_y") == E_INVALID and "entry 64" in L.last_error(g._h)
    assert predict(y="bad_y") == E_INVALID
    for d in (0, 32, 96, 320):
        assert loss_grad(params(d=d)) == E_INVALID and predict(params(d=d)) == E_INVALID and minmax(d=d) == E_INVALID
    for c in (0, 1, 257):
        assert loss_grad(params(c=c)) == E_INVALID and predict(params(c=c)) == E_INVALID
    assert loss_grad(cnt=0) == E_INVALID and predict(cnt=0) == E_INVALID and minmax(cnt=0) == E_INVALID
    for kw in (dict(emb=None), dict(ids=None), dict(y=None), dict(wb=None), dict(out=None), dict(h=None),
               dict(lossp=None)):
        assert loss_grad(**kw) == E_INVALID, kw
    assert predict(out=None) == E_INVALID and predict(y=None) == E_INVALID     # a confusion matrix without labels
    assert minmax(lo_=None) == E_INVALID
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (pred == -3).all() and (lo_out == 5.0).all() and (hi_out == 6.0).all()
    assert (conf == 9).all() and loss.value == -1.0
    assert np.array_equal(t["emb"].cpu().numpy(), table) and np.array_equal(t["wb"].cpu().numpy(), wb)
    # and the same calls without the fault run
    assert loss_grad() == 0 and predict() == 0 and predict(y=None, cm=None) == 0 and minmax() == 0
    assert conf.sum() == count and loss.value > 0


# f. ------------------------------------------------------------------------------------------
def test_fit_reaches_the_float32_optimum(W, torch, g, gold):
    table, train, test, labels = gold["table"], gold["train"], gold["test"], gold["labels"]
    lo, scale, l2 = gold["lo"], gold["scale"], float(gold["l2"])
    W_opt, F_opt = gold["W_opt"], float(gold["F_opt"])
    y = labels[train]
    every = np.concatenate([train, test])

    def F(wb, dtype=np.float64):
        return R.objective_grad(table, train, y, lo, scale, wb, l2, dtype)

    def z(wb, ids=every):
        return R.logits(table, ids, lo, scale, wb, np.float64)

    import torch as T
    w32, _, it32 = W.lbfgs(lambda w: F(w.numpy(), np.float32), W_opt.shape, dtype=T.float32)
    w32 = w32.numpy().astype(np.float64)
    gap32 = float(F(w32)[0]) - F_opt
    dev32 = float(np.abs(z(w32) - z(W_opt)).max())

    emb = dev(torch, table)
    clf = W.VertexClassifier(g, 64, 7, l2=l2).fit(emb, train, y)
    np.testing.assert_array_equal(clf.lo.cpu().numpy(), lo)
    np.testing.assert_array_equal(clf.scale.cpu().numpy(), scale)
    w_dev = clf.wb.cpu().numpy().astype(np.float64)
    gap = float(F(w_dev)[0]) - F_opt
    deviation = float(np.abs(z(w_dev) - z(W_opt)).max())
    print(f"float32 restatement: {it32} iterations, gap32 {gap32:.3e}, dev32 {dev32:.3e}")
    print(f"device: {clf.iterations} iterations, F - F_opt {gap:.3e} (ratio {gap / gap32:.3f}), "
          f"logit deviation {deviation:.3e} (ratio {deviation / dev32:.3f}); F_recipe - F_opt "
          f"{float(gold['F_recipe']) - F_opt:.3e}")
    assert gap32 > 0 and dev32 > 0
    assert gap <= 8 * gap32
    assert deviation <= 8 * dev32
    z_opt = z(W_opt, test)
    decisive = R.top_two_gap(z_opt) > 2 * deviation
    print(f"decisive held-out rows {decisive.mean():.4f}")
    assert decisive.mean() >= 0.99
    pred = clf.predict(emb, test).cpu().numpy()
    np.testing.assert_array_equal(pred[decisive], R.predict(z_opt)[decisive])
    s = clf.score(emb, test, labels[test])
    assert 0.7 <= s["accuracy"] <= 0.97


# g. ------------------------------------------------------------------------------------------
def test_wiki_end_to_end(W, torch):
    d = np.load(os.path.join(GOLDEN, "wiki_csr.npz"))
    ids, y, classes = W.read_labels(os.path.join(GOLDEN, "wiki_labels.txt"))
    n = len(d["off"]) - 1
    assert n == len(ids) == 2405 and len(classes) == 17
    g = W.WharfMH.from_csr(d["off"], d["adj"], config=W.WharfConfig(walks_per_vertex=10, walk_length=80,
                                                                    model=W.DEEPWALK, seed=0x5EED))
    g.generate_initial_random_walks()
    sg = W.SkipGram(g, dim=128)
    sg.refresh_noise()
    for p in range(5):
        sg.train(pass_=p)

    def evaluate(tag):
        row = W.evaluate_embeddings(g, sg.emb_in, ids, y, classes=17)
        clf, test = row["classifier"], row["test_index"]
        pred = clf.predict(sg.emb_in, ids[test]).cpu().numpy()
        cm = R.confusion(y[test], pred, 17)
        np.testing.assert_array_equal(row["confusion"], cm)
        ref = R.metrics(cm)
        four = [row[k] for k in ("accuracy", "f1_macro", "f1_micro", "f1_weighted")]
        np.testing.assert_allclose(four, [ref[k] for k in ("accuracy", "f1_macro", "f1_micro", "f1_weighted")],
                                   rtol=0, atol=1e-12)
        assert np.isfinite(four).all()
        majority = np.bincount(y[test], minlength=17).max() / len(test)
        print(f"wiki {tag}: accuracy {four[0]:.4f}, f1 macro {four[1]:.4f}, micro {four[2]:.4f}, weighted {four[3]:.4f} "
              f"({row['train']} train / {row['test']} test rows, {row['iterations']} L-BFGS iterations, "
              f"majority share {majority:.4f})")
        return four[0], majority

    acc, majority = evaluate("initial")
    assert acc > majority
    out = torch.zeros(g.number_of_walks, dtype=torch.int32, device="cuda")
    aff = g.insert_edges_batch(O.generate_batch_of_edges(3000, n, 3, False, False), remove_dups=True, out=out)
    assert aff.numel() > 0
    sg.train(aff, pass_=5)
    evaluate("after one 3000-edge batch")
    g.destroy()
