"""CPU tests of the clustering stage's host side: the exported symbols and the
parameter struct, the float32 restatement tests/kmeans_ref.py against float64 within the derived
bounds (on the inputs the GPU tests use), NMI and modularity.  No GPU."""
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
import kmeans_ref as R  # noqa: E402
from emb_ref import rnorm32  # noqa: E402

NAMES = ("wharf_kmeans_assign", "wharf_kmeans_update", "wharf_partition_stats")


def test_symbols_are_exported():
    from dynamicgraphrepresentationlearning_amd import _lib as L
    header = open(os.path.join(REPO, "include", "wharf_gpu.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and getattr(L.lib, name) is not None
        assert name + "(" in header
    assert "wharf_kmeans_params" in header


def test_params_struct_is_16_bytes_and_the_abi_version_stays():
    from dynamicgraphrepresentationlearning_amd import _lib as L
    assert C.sizeof(L.wharf_kmeans_params) == 16
    assert L.lib.wharf_abi_version() == 9 and L.ABI_VERSION == 9
    prog = r"""
#include <stdio.h>
#include <stddef.h>
#include "wharf_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d\n", sizeof(wharf_kmeans_params), offsetof(wharf_kmeans_params, dim),
         offsetof(wharf_kmeans_params, k), offsetof(wharf_kmeans_params, flags),
         offsetof(wharf_kmeans_params, reserved), WHARF_ABI_VERSION);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = L.wharf_kmeans_params
    assert got == [16, P.dim.offset, P.k.offset, P.flags.offset, P.reserved.offset, 9]


def test_python_exports():
    import dynamicgraphrepresentationlearning_amd as W
    for name in ("VertexClustering", "nmi", "modularity", "evaluate_clustering"):
        assert hasattr(W, name) and name in W.__all__
    assert hasattr(W.WharfMH, "partition_stats")
    for name in ("fit", "predict"):
        assert hasattr(W.VertexClustering, name)


@pytest.mark.parametrize("kind", ["structured", "unstructured"])
@pytest.mark.parametrize("shape", R.FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float32_restatement_is_within_the_bounds(shape, kind):
    """Scores, inertia and updated centroids of the chain against float64, with and without rnorm,
    on the GPU tests' inputs."""
    count, dim, k = shape
    emb, cent, vids = R.float_case(kind, count, dim, k)
    x = emb[vids]
    for r in (None, rnorm32(emb)[vids]):
        s32, s64, bound = R.scores32(x, cent, r), R.scores64(x, cent, r), R.score_bound(x, cent, r)
        ratio = float((np.abs(s32.astype(np.float64) - s64) / bound).max())
        dec, allowed = R.decisive(s64, bound)
        a32, best32 = R.assign_of(s32)
        print(f"{kind} {shape} rnorm {r is not None}: score err / bound {ratio:.3f}; {int((~dec).sum())} indecisive rows")
        assert ratio <= 1.0
        assert (~dec).sum() <= 0.01 * count
        assert allowed[np.arange(count), a32].all()
        assert np.array_equal(a32[dec], np.argmax(s64, axis=1)[dec])
        i32 = R.inertia_of(R.xx32(x, r), best32)
        i64 = float((R.xx64(x, r) - 2.0 * s64[np.arange(count), a32]).sum())
        ib = R.inertia_bound(x, cent, a32, r)
        print(f"  inertia err / bound {abs(i32 - i64) / ib:.3f}")
        assert abs(i32 - i64) <= ib
        c32, n32 = R.update32(x, a32, cent, r)
        sums, mags, n64 = R.sums64(x, a32, k, r)
        assert np.array_equal(n32, n64)
        nz = n64 > 0
        c64 = np.where(nz[:, None], sums / np.maximum(n64, 1)[:, None], cent.astype(np.float64))
        cb = R.centroid_bound(mags, n64, c64)
        err = np.abs(c32.astype(np.float64) - c64)
        print(f"  centroid err / bound {float((err[nz] / cb[nz]).max()):.3f}; {int((~nz).sum())} empty clusters")
        assert (err[nz] <= cb[nz]).all()
        assert np.array_equal(c32[~nz].view(np.uint32), cent[~nz].view(np.uint32))


def test_structured_rnorm_cases_contain_empty_clusters():
    """The update's empty-cluster path is exercised by the float cases themselves: with normalised rows
    the -hn term decides, and most centroids of the larger k attract no row.  (k = 7 has exactly one
    empty cluster with this generator, whichever order its draws are made in; only k = 2 has none.)"""
    empties = {}
    for count, dim, k in R.FLOAT_SHAPES:
        emb, cent, vids = R.float_case("structured", count, dim, k)
        x = emb[vids]
        a = np.argmax(R.scores64(x, cent, rnorm32(emb)[vids]), axis=1)
        empties[k] = int((np.bincount(a, minlength=k) == 0).sum())
    print(f"empty clusters by k: {empties}")
    assert empties == {7: 1, 2: 0, 17: 14, 64: 59, 256: 223}


@pytest.mark.parametrize("dim", [64, 256])
def test_integer_cases_are_exact_in_float32(dim):
    for k, count in ((7, 65), (33, 257)):
        emb, cent, vids = R.integer_case(count, dim, k)
        x = emb[vids]
        assert np.array_equal(R.scores32(x, cent).astype(np.float64), R.scores64(x, cent))
    emb, cent = R.onehot_case(100, dim, 40)
    assert np.array_equal(R.scores32(emb, cent).astype(np.float64), R.scores64(emb, cent))


def test_assign_takes_the_lowest_id_and_folds_zero():
    s = np.array([[1.0, 3.0, 3.0], [-0.0, 0.0, -1.0], [0.0, -0.0, -1.0]], dtype=np.float32)
    a, best = R.assign_of((s + np.float32(0)).astype(np.float32))
    assert list(a) == [1, 0, 0]
    assert list(best.view(np.uint32)) == [np.float32(3).view(np.uint32), 0, 0]


def test_nmi_equals_the_definition():
    from dynamicgraphrepresentationlearning_amd import nmi
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 5, 400), rng.integers(0, 7, 400)
    assert nmi(a, b) == pytest.approx(R.nmi(a, b), abs=1e-12)
    b = (a + (rng.random(400) < 0.2)) % 5                       # correlated
    assert nmi(a, b) == pytest.approx(R.nmi(a, b), abs=1e-12) and 0.2 < nmi(a, b) < 1.0
    assert nmi(a, b) == pytest.approx(nmi(b, a), abs=1e-12)
    perm = np.array([3, 0, 4, 1, 2])
    assert nmi(a, perm[a]) == pytest.approx(1.0, abs=1e-12)     # label names do not matter
    assert nmi(perm[a] + 100, b) == pytest.approx(nmi(a, b), abs=1e-12)
    assert nmi(np.zeros(9), np.zeros(9)) == 1.0                 # a single class on both sides
    assert nmi(np.zeros(9), np.arange(9) % 3) == 0.0            # on one side only
    assert nmi(np.arange(9) % 3, np.ones(9)) == 0.0
    assert nmi([0, 0, 1, 1], [0, 1, 0, 1]) == pytest.approx(0.0, abs=1e-15)   # independent
    with pytest.raises(ValueError):
        nmi([0, 1], [0])


def test_modularity_of_two_triangles_is_5_14():
    from dynamicgraphrepresentationlearning_amd import modularity_from_stats
    off, adj = R.two_triangles()
    part = np.array([0, 0, 0, 1, 1, 1])
    intra, vol = R.partition_stats(off, adj, part, 2)
    assert list(intra) == [6, 6] and list(vol) == [7, 7]
    assert modularity_from_stats(intra, vol) == 5 / 14
    assert R.modularity(intra, vol) == 5 / 14
    intra, vol = R.partition_stats(off, adj, np.zeros(6, int), 1)
    assert modularity_from_stats(intra, vol) == 0.0             # one cluster: 1 - 1
    assert modularity_from_stats([0, 0], [0, 0]) == 0.0         # no edges
