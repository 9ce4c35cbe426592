"""CPU checks of the skip-gram trainer's host side: the ABI surface, the alias-table
builder, and the numpy restatement the GPU tests compare against.  No device calls."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgns_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wharf_gpu.h")
ENTRY_POINTS = ("wharf_sgns_build_alias", "wharf_sgns_build_noise", "wharf_sgns_get_noise", "wharf_sgns_samples",
                "wharf_sgns_train")


def test_header_declares_and_binding_binds_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wharf_[a-z0-9_]+)\s*\(", src))
    from dynamicgraphrepresentationlearning_amd import _lib as L
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in L.SIGNATURES, name
        assert hasattr(L.lib, name), name
    assert L.ABI_VERSION == 9 and L.lib.wharf_abi_version() == 9
    assert "#define WHARF_ABI_VERSION 9" in open(HEADER).read()
    # the PODs mirror the header: 6 x 4 bytes, and {double, u64, u64, float} padded to 32
    assert C.sizeof(L.wharf_sgns_params) == 24 and C.sizeof(L.wharf_sgns_result) == 32
    import dynamicgraphrepresentationlearning_amd as W
    assert W.SkipGram is not None


def test_numpy_philox_matches_the_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2**32, size=(16, 4), dtype=np.uint64)
    ctr[0] = 0
    ctr[1] = 0xFFFFFFFF
    for key in ((0x5EED, 0), (0xDEADBEEF, 0x12345678)):
        got = np.stack(R.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
        for row, c in zip(got, ctr):
            assert [int(x) for x in row] == O.philox4x32_10([int(x) for x in c], key)


def _zipf_counts(n=1000, seed=3):
    rng = np.random.default_rng(seed)
    counts = (1e5 / (1 + np.arange(n)) ** 1.1).astype(np.uint64) + 1
    rng.shuffle(counts)
    counts[rng.permutation(n)[: n // 3]] = 0
    return counts


def _build(counts, power):
    from dynamicgraphrepresentationlearning_amd.sgns import build_alias
    return build_alias(counts, power)


@pytest.mark.parametrize("power", [0.75, 1.0, 0.0])
def test_alias_table_distribution(power):
    counts = _zipf_counts()
    assert (counts == 0).sum() == len(counts) // 3
    thr, alias = _build(counts, power)
    assert (alias < len(counts)).all()
    w = np.where(counts > 0, counts.astype(np.float64) ** power, 0.0)
    P = R.alias_distribution(thr, alias)
    err = np.abs(P - w / w.sum()).max()
    print(f"power {power}: max |P - w/sum| = {err:.3e}")
    # each of at most n + 1 terms is quantised by 2^-32 / n: below 2^-32 = 2.3e-10 in all
    assert err < 1e-9
    assert (P[counts == 0] == 0).all()                 # exactly: thr == 0 and nothing aliases there
    assert (thr[counts == 0] == 0).all() and (counts[alias] > 0).all()
    # an entry whose own probability is 1 aliases itself
    assert (alias[thr == 0xFFFFFFFF] == np.nonzero(thr == 0xFFFFFFFF)[0]).all()
    # deterministic: the same input gives the same table
    thr2, alias2 = _build(counts, power)
    assert np.array_equal(thr, thr2) and np.array_equal(alias, alias2)


def test_alias_table_single_vertex_and_all_zero():
    counts = np.zeros(37, dtype=np.uint64)
    counts[11] = 5
    thr, alias = _build(counts, 0.75)
    # every bucket yields vertex 11, whatever the second word of the draw
    assert thr[11] == 0xFFFFFFFF and alias[11] == 11
    others = np.arange(37) != 11
    assert (thr[others] == 0).all() and (alias[others] == 11).all()
    from dynamicgraphrepresentationlearning_amd import _lib as L
    zero = np.zeros(8, dtype=np.uint64)
    t = np.zeros(8, dtype=np.uint32)
    a = np.zeros(8, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.lib.wharf_sgns_build_alias(p(zero), 8, 0.75, p(t), p(a)) == -1   # WHARF_E_INVALID


def test_draws_follow_the_alias_table_and_drop_the_centre():
    """The restatement's negatives come from the table's buckets, and a negative equal to the centre
    is dropped (checked on a graph small enough that it happens)."""
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 6, size=(40, 12)).astype(np.uint32)
    rows[3, 5:] = R.SENT
    counts = np.bincount(rows[rows != R.SENT], minlength=6).astype(np.uint64)
    thr, alias = _build(counts, 0.75)
    s0 = R.draws(rows, np.arange(40), 0x5EED, 0, 3, 4, thr, alias)
    s1 = R.draws(rows, np.arange(40), 0x5EED, 1, 3, 4, thr, alias)
    assert not np.array_equal(s0, s1)
    live = rows != R.SENT
    assert ((s0[..., 0] >= 1) & (s0[..., 0] <= 3))[live].all() and (s0[..., 0][~live] == 0).all()
    neg = s0[..., 1:]
    assert (neg[~live] == R.DROPPED).all()
    assert (neg == R.DROPPED)[live].any()
    kept = neg != R.DROPPED
    assert (neg[kept] < 6).all() and (neg != rows[..., None])[kept].all()


def test_restatement_converges_on_a_planted_graph():
    """Serial SGNS with the Philox draws separates 8 planted communities (the parameters of the
    issue: 256 vertices, wpv 4, L 20, D 64, window 3, K 3, lr 0.025, 3 passes)."""
    off, adj, comm = R.planted_graph()
    rows = R.uniform_walks(off, adj, wpv=4, L=20)
    wids = np.arange(len(rows))
    counts = np.bincount(rows[rows != R.SENT], minlength=256).astype(np.uint64)
    thr, alias = _build(counts, 0.75)
    emb_in, emb_out = R.word2vec_init(256, 64)
    per_term = []
    for p in range(3):
        s = R.draws(rows, wids, 0x5EED, p, 3, 3, thr, alias)
        loss, terms, centres = R.train(rows, s, emb_in, emb_out, 0.025)
        assert centres == int(R.walk_lengths(rows).sum()) and terms > centres
        per_term.append(loss / terms)
    intra, inter = R.cosine_gap(emb_in, comm)
    print(f"loss per term {per_term}, intra {intra:.3f}, inter {inter:.3f}")
    assert per_term[0] > per_term[1] > per_term[2]
    assert per_term[2] < math.log(2)
    assert intra > inter
