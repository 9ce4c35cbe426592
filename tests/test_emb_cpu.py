"""CPU tests of the embedding queries' host side: the exported symbols and the
parameter struct, the float32 restatement tests/emb_ref.py against float64 within the derived
bounds (on the inputs the GPU tests use), AUC and hits@k.  No GPU."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import emb_ref as R  # noqa: E402

NAMES = ("wharf_emb_row_norms", "wharf_emb_score_pairs", "wharf_emb_topk", "wharf_has_edges")


def test_symbols_are_exported():
    from dynamicgraphrepresentationlearning_amd import _lib as L
    header = open(os.path.join(REPO, "include", "wharf_gpu.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and getattr(L.lib, name) is not None
        assert name + "(" in header
    for name in ("wharf_emb_params", "WHARF_EMB_DOT", "WHARF_EMB_COSINE", "WHARF_EMB_EXCLUDE_SELF",
                 "WHARF_EMB_EXCLUDE_NEIGHBOURS"):
        assert name in header


def test_params_struct_is_24_bytes_and_the_abi_version_stays():
    from dynamicgraphrepresentationlearning_amd import _lib as L
    assert C.sizeof(L.wharf_emb_params) == 24
    assert L.lib.wharf_abi_version() == 9
    prog = r"""
#include <stdio.h>
#include <stddef.h>
#include "wharf_gpu.h"
int main(void) {
  printf("%zu %zu %zu %d %d %d %d %d\n", sizeof(wharf_emb_params), offsetof(wharf_emb_params, k),
         offsetof(wharf_emb_params, reserved), WHARF_EMB_DOT, WHARF_EMB_COSINE, WHARF_EMB_EXCLUDE_SELF,
         WHARF_EMB_EXCLUDE_NEIGHBOURS, WHARF_ABI_VERSION);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, L.wharf_emb_params.k.offset, L.wharf_emb_params.reserved.offset, L.WHARF_EMB_DOT,
                   L.WHARF_EMB_COSINE, L.WHARF_EMB_EXCLUDE_SELF, L.WHARF_EMB_EXCLUDE_NEIGHBOURS, 9]


def test_python_exports():
    import dynamicgraphrepresentationlearning_amd as W
    for name in ("Similarity", "auc", "hits_at_k", "sample_non_edges", "link_prediction"):
        assert hasattr(W, name) and name in W.__all__
    assert hasattr(W.WharfMH, "has_edges")


def test_float32_restatement_is_within_the_bounds():
    """The chain against float64 on the GPU tests' random tables (n = 1100, dim = 128, 70 queries)."""
    dim = 128
    eq, er = R.float_tables(1100, dim)
    qs = R.float_queries()
    pairs = R.all_pairs(qs, len(er))
    x, y = eq[pairs[:, 0]], er[pairs[:, 1]]
    err = np.abs(R.pair_scores32(eq, er, pairs).astype(np.float64) - R.pair_scores64(eq, er, pairs))
    bound = R.dot_bound(x, y)
    print(f"dot: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    err = np.abs(R.pair_scores32(eq, er, pairs, "cosine").astype(np.float64) - R.pair_scores64(eq, er, pairs, "cosine"))
    print(f"cosine: max err / bound {float(err.max() / R.cosine_bound(dim)):.3f}")
    assert err.max() <= R.cosine_bound(dim)
    for t in (eq, er):
        rel = np.abs(R.rnorm32(t).astype(np.float64) / R.rnorm64(t) - 1)
        print(f"rnorm: max rel err / bound {float(rel.max() / R.rnorm_bound(dim)):.3f}")
        assert rel.max() <= R.rnorm_bound(dim)


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_integer_tables_are_exact_in_float32(dim):
    for eq, er in (R.integer_tables(200, dim), R.onehot_tables(200, dim)):
        qs = np.arange(200)
        s32, s64 = R.score_matrix32(eq, er, qs), R.score_matrix64(eq, er, qs)
        assert np.array_equal(s32.astype(np.float64), s64)


def test_order_and_topk_of_the_restatement():
    scores = np.array([1.0, 3.0, 3.0, -0.0, 0.0, 2.0], dtype=np.float32)
    assert list(R.order(scores)) == [1, 2, 5, 0, 3, 4]           # ties by id; -0 == +0
    ok = R.eligible(6, 1, True, (np.array([0, 0, 2, 2, 2, 2, 2]), np.array([2, 5])))
    assert list(np.flatnonzero(ok)) == [0, 3, 4]
    ids, s = R.topk_row(scores, ok, 5)
    assert list(ids) == [0, 3, 4, R.NO_ID, R.NO_ID] and list(s[:3]) == [1.0, 0.0, 0.0] and np.isneginf(s[3:]).all()
    off, adj = np.array([0, 2, 2, 3]), np.array([1, 2, 0])
    assert list(R.has_edges(off, adj, np.array([[0, 1], [0, 2], [0, 0], [1, 0], [2, 0], [2, 1]]))) == \
        [True, True, False, False, True, False]


def test_auc_equals_the_definition():
    from dynamicgraphrepresentationlearning_amd import auc
    rng = np.random.default_rng(4)
    pos = rng.integers(0, 12, 300).astype(np.float32)       # many ties within and across the classes
    neg = rng.integers(-3, 9, 211).astype(np.float32)
    assert auc(pos, neg) == pytest.approx(R.auc(pos, neg), abs=1e-12)
    pos, neg = rng.normal(0.3, 1, 157), rng.normal(0, 1, 90)
    assert auc(pos, neg) == pytest.approx(R.auc(pos, neg), abs=1e-12)
    assert auc(np.ones(7), np.ones(5)) == 0.5                 # all tied
    assert auc([2.0, 3.0, 2.5], [1.0, -1.0]) == 1.0           # perfectly separated
    assert auc([0.0], [1.0, 2.0]) == 0.0
    with pytest.raises(ValueError):
        auc([], [1.0])


def test_hits_at_k():
    from dynamicgraphrepresentationlearning_amd import hits_at_k
    ids = np.array([[4, 7, 1], [0, 2, 9], [5, 5, 5], [3, 8, 6]])
    assert hits_at_k(ids, [7, 3, 5, 6]) == 0.75
    assert hits_at_k(ids, [9, 9, 9, 9]) == 0.25
    assert hits_at_k(ids[:, :1], [4, 0, 5, 3]) == 1.0
    with pytest.raises(ValueError):
        hits_at_k(ids, [1, 2])
