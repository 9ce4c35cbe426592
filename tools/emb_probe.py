#!/usr/bin/env python3
"""How fast is the exact top-k search over an embedding table?

Times wharf_emb_topk (default: n = 2^20 rows, dim 128, 4096 random queries, k = 10, dot metric, the
query itself excluded) and reports the median wall time of the synchronous call (id check, tile
kernel, merge) over --reps calls after a warm-up, 2 q n dim / time, and the table bytes per second:
`streamed` counts every query tile's pass over the table (tiles * n * dim * 4, what the blocks
load through L2), `table` counts the table once.  The torch composition topk(eq[chunk] @ er.T, k + 1)
over 512-query chunks is timed in the same process, alternating with the library call, and the
share of queries whose id lists agree is reported (torch's GEMM sums in another order, so near
ties may swap).

    python tools/emb_probe.py [--n 1048576] [--dim 128] [--q 4096] [--k 10] [--out profiles/emb_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="rows of the table")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--q", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=512, help="queries per GEMM of the torch composition")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import dynamicgraphrepresentationlearning_amd as W
    gen = torch.Generator(device="cuda").manual_seed(1)
    eq = torch.randn(a.n, a.dim, device="cuda", generator=gen)
    er = torch.randn(a.n, a.dim, device="cuda", generator=gen)
    queries = torch.randint(0, a.n, (a.q,), device="cuda", generator=gen, dtype=torch.int32)
    g = W.WharfMH(16)
    sim = W.Similarity(g, eq, er, metric="dot")

    def ours():
        return sim.most_similar(queries, k=a.k, exclude_self=True, splits=a.splits)

    def composition():
        ids = []
        for c in range(0, a.q, a.chunk):
            qc = queries[c:c + a.chunk].long()
            ids.append(torch.topk(eq[qc] @ er.T, a.k + 1, dim=1).indices)   # k + 1: the query itself may be among them
        torch.cuda.synchronize()
        return ids

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    ours()
    composition()
    t_ours, t_torch = [], []
    for _ in range(a.reps):                               # alternated: both see the same clocks and caches
        t_ours.append(timed(ours))
        t_torch.append(timed(composition))
    s, st = statistics.median(t_ours), statistics.median(t_torch)

    # agreement of the id lists (as sets in list order: the composition's ids are compared position by position)
    ids, _ = ours()
    agree = 0
    for c in range(0, a.q, a.chunk):
        qc = queries[c:c + a.chunk].long()
        top = torch.topk(eq[qc] @ er.T, a.k + 1, dim=1).indices
        for row, mine, v in zip(top.tolist(), ids[c:c + a.chunk].tolist(), qc.tolist()):
            agree += [x for x in row if x != v][:a.k] == mine
    tiles = (a.q + 31) // 32
    flop = 2.0 * a.q * a.n * a.dim
    res = {"n": a.n, "dim": a.dim, "q": a.q, "k": a.k, "metric": "dot", "exclude_self": True, "splits": a.splits,
           "reps": a.reps, "ms_median": s * 1e3, "ms_all": [t * 1e3 for t in t_ours], "flop_per_s": flop / s,
           "streamed_bytes_per_s": tiles * a.n * a.dim * 4.0 / s, "table_bytes_per_s": a.n * a.dim * 4.0 / s,
           "torch_composition_ms_median": st * 1e3, "torch_composition_ms_all": [t * 1e3 for t in t_torch],
           "torch_chunk": a.chunk, "torch_flop_per_s": flop / st, "ratio_torch_over_ours": st / s,
           "id_lists_agree": agree / a.q}
    print(f"n {a.n} dim {a.dim} q {a.q} k {a.k}: {res['ms_median']:.2f} ms median, {res['flop_per_s'] / 1e12:.1f} TFLOP/s, "
          f"{res['streamed_bytes_per_s'] / 1e12:.2f} TB/s streamed; torch composition {res['torch_composition_ms_median']:.2f} ms "
          f"({res['torch_flop_per_s'] / 1e12:.1f} TFLOP/s); torch / ours {res['ratio_torch_over_ours']:.2f}; "
          f"id lists agree for {100 * res['id_lists_agree']:.2f} % of the queries", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    g.destroy()


if __name__ == "__main__":
    main()
