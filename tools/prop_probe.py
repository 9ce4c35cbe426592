#!/usr/bin/env python3
"""How fast is one propagation over the live graph?

On README's graph, from_rmat(1 << 20, 10_750_000), with norm="sym" and self loops, at dim 64, 128 and
256: the median wall time over --reps synchronous calls after a warm-up of the full-table call and of
a 100 k-id list call, the gathered bytes per second (m dim 4 / t; for the list, the listed rows'
targets), the same product by torch.sparse.mm on a CSR tensor built from flatten_graph() (the time
to build that tensor recorded separately: it has to be rebuilt after every update batch), the
maximal elementwise difference between the two, and the time of the same call on a degree-regular
graph of equal n and (nearly) equal m, which shows what the split of long rows leaves of the skew.

    python tools/prop_probe.py [--dims 64,128,256] [--reps 10] [--out profiles/prop_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps, torch):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def regular_graph(n, d, seed=1):
    """Every row d distinct targets, uniformly spread: pi[(v + o_j) mod n] for d distinct offsets o_j."""
    rng = np.random.default_rng(seed)
    pi = rng.permutation(n).astype(np.uint32)
    offs = rng.choice(np.arange(1, n), d, replace=False)
    adj = np.sort(pi[(np.arange(n)[:, None] + offs[None, :]) % n], axis=1)
    return np.arange(n + 1, dtype=np.uint64) * d, np.ascontiguousarray(adj.reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--edges", type=int, default=10_750_000)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--ids", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import dynamicgraphrepresentationlearning_amd as W
    g = W.WharfMH.from_rmat(a.n, a.edges)
    n, m = g.number_of_vertices(), g.number_of_edges()
    prop = W.GraphPropagation(g, "sym", True)
    deg = g.degrees().cpu().numpy().astype(np.int64)
    ids_host = np.random.default_rng(2).integers(0, n, a.ids).astype(np.uint32)
    ids = torch.from_numpy(ids_host.view(np.int32)).cuda()
    m_ids = int(deg[ids_host].sum())
    d_reg = max(1, round(m / n))
    greg = W.WharfMH.from_csr(*regular_graph(n, d_reg))
    preg = W.GraphPropagation(greg, "sym", True)
    m_reg = greg.number_of_edges()

    # the torch operand: the CSR to the host and back, D (A + I) D as one CSR tensor
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    off, adj = g.flatten_graph()
    w = prop.wdst
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(np.diff(off.astype(np.int64))).cuda())
    cols = torch.from_numpy(adj.astype(np.int64)).cuda()
    diag = torch.arange(n, device="cuda")
    rows, cols = torch.cat([rows, diag]), torch.cat([cols, diag])
    A = torch.sparse_coo_tensor(torch.stack([rows, cols]), w[rows] * w[cols], (n, n)).coalesce().to_sparse_csr()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    res = {"n": n, "m": m, "max_degree": int(deg.max()), "rows_over_512": int((deg > 512).sum()),
           "targets_in_rows_over_512": int(deg[deg > 512].sum()), "ids": a.ids, "m_ids": m_ids,
           "regular_degree": d_reg, "m_regular": m_reg, "torch_csr_build_ms": build_s * 1e3, "reps": a.reps, "shapes": []}
    print(f"n {n} m {m} max degree {res['max_degree']}, {res['rows_over_512']} rows over 512 targets holding "
          f"{100.0 * res['targets_in_rows_over_512'] / m:.1f} % of m; torch CSR build {build_s * 1e3:.1f} ms", flush=True)
    for dim in [int(x) for x in a.dims.split(",")]:
        x = torch.randn(n, dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(dim))
        out = torch.empty_like(x)
        out_ids = torch.empty(a.ids, dim, device="cuda")
        t_full, all_full = timed(lambda: prop.apply(x, out=out), a.reps, torch)
        t_ids, all_ids = timed(lambda: prop.apply(x, ids=ids, out=out_ids), a.reps, torch)
        t_reg, all_reg = timed(lambda: preg.apply(x, out=out), a.reps, torch)
        prop.apply(x, out=out)
        row = {"dim": dim, "full_ms_median": t_full * 1e3, "full_ms_all": [t * 1e3 for t in all_full],
               "full_gathered_bytes_per_s": m * dim * 4.0 / t_full,
               "ids_ms_median": t_ids * 1e3, "ids_ms_all": [t * 1e3 for t in all_ids],
               "ids_gathered_bytes_per_s": m_ids * dim * 4.0 / t_ids,
               "regular_ms_median": t_reg * 1e3, "regular_ms_all": [t * 1e3 for t in all_reg],
               "regular_gathered_bytes_per_s": m_reg * dim * 4.0 / t_reg,
               "rmat_over_regular_per_target": (t_full / m) / (t_reg / m_reg)}
        try:
            ref = torch.sparse.mm(A, x)
            t_torch, all_torch = timed(lambda: torch.sparse.mm(A, x), a.reps, torch)
            row.update(torch_ms_median=t_torch * 1e3, torch_ms_all=[t * 1e3 for t in all_torch],
                       torch_over_ours=t_torch / t_full, max_abs_diff_from_torch=float((ref - out).abs().max()),
                       max_abs_value=float(ref.abs().max()))
            del ref
        except RuntimeError as e:   # recorded, not hidden: the comparison is then missing from the file
            row["torch_error"] = str(e)[:200]
        res["shapes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    g.destroy()
    greg.destroy()


if __name__ == "__main__":
    main()
