#!/usr/bin/env python3
"""How fast are the two k-means passes over an embedding table?

Times one synchronous wharf_kmeans_assign (id check excluded: all rows; hn, the tile kernel, the
inertia) and one wharf_kmeans_update (assignment check, block shares, reduction) at n = 2^20 rows,
dim 128, k in {8, 64, 256}: the median wall time over --reps calls after a warm-up, 2 n k dim / time
against the 155 TFLOP/s of the f32 MFMA, and the row bytes (n dim 4) per second.  The torch
composition (argmin over centroids of |c|^2 - 2 x c^T by chunked GEMM, then index_add_ and a
division) is timed in the same process, alternating with the library calls, and the share of rows
on which the two assignments agree is reported (torch's GEMM sums in another order, so near ties
may differ).

    python tools/kmeans_probe.py [--n 1048576] [--dim 128] [--ks 8,64,256] [--out profiles/kmeans_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MFMA_F32_FLOPS = 155e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="rows of the table")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--ks", default="8,64,256")
    ap.add_argument("--chunk", type=int, default=1 << 16, help="rows per GEMM of the torch composition")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import dynamicgraphrepresentationlearning_amd as W
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = torch.randn(a.n, a.dim, device="cuda", generator=gen)
    g = W.WharfMH(16)
    rows = []
    for k in [int(x) for x in a.ks.split(",")]:
        km = W.VertexClustering(g, a.dim, k)
        start = emb[torch.randperm(a.n, device="cuda", generator=gen)[:k]].clone()
        km.centroids = start.clone()
        labels = km.assign(emb)[0]

        def assign():
            return km.assign(emb)

        def update():
            km.centroids.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            km.update(emb, labels)
            return time.perf_counter() - t0

        def t_assign():
            hn = 0.5 * (start * start).sum(dim=1)
            out = []
            for c in range(0, a.n, a.chunk):
                out.append(torch.argmax(emb[c:c + a.chunk] @ start.T - hn, dim=1))
            out = torch.cat(out)
            torch.cuda.synchronize()
            return out

        tl = t_assign()

        def t_update():
            sums = torch.zeros(k, a.dim, device="cuda").index_add_(0, tl, emb)
            cnt = torch.bincount(tl, minlength=k).clamp(min=1)
            out = sums / cnt[:, None]
            torch.cuda.synchronize()
            return out

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        assign(), update(), t_assign(), t_update()
        ta, tu, tta, ttu = [], [], [], []
        for _ in range(a.reps):                               # alternated: both see the same clocks and caches
            ta.append(timed(assign))
            tta.append(timed(t_assign))
            tu.append(update())
            ttu.append(timed(t_update))
        sa, su, sta, stu = (statistics.median(t) for t in (ta, tu, tta, ttu))
        agree = float((labels.long() == tl).float().mean())
        flop = 2.0 * a.n * k * a.dim
        row = {"n": a.n, "dim": a.dim, "k": k, "reps": a.reps,
               "assign_ms_median": sa * 1e3, "assign_ms_all": [t * 1e3 for t in ta],
               "assign_flop_per_s": flop / sa, "assign_share_of_f32_mfma": flop / sa / MFMA_F32_FLOPS,
               "assign_row_bytes_per_s": a.n * a.dim * 4.0 / sa,
               "update_ms_median": su * 1e3, "update_ms_all": [t * 1e3 for t in tu],
               "update_row_bytes_per_s": a.n * a.dim * 4.0 / su,
               "torch_assign_ms_median": sta * 1e3, "torch_assign_ms_all": [t * 1e3 for t in tta],
               "torch_assign_flop_per_s": flop / sta, "torch_chunk": a.chunk,
               "torch_update_ms_median": stu * 1e3, "torch_update_ms_all": [t * 1e3 for t in ttu],
               "assign_torch_over_ours": sta / sa, "update_torch_over_ours": stu / su,
               "assignments_agree": agree}
        rows.append(row)
        print(f"n {a.n} dim {a.dim} k {k}: assign {sa * 1e3:.3f} ms ({flop / sa / 1e12:.1f} TFLOP/s, "
              f"{100 * flop / sa / MFMA_F32_FLOPS:.1f} % of the f32 MFMA, {a.n * a.dim * 4.0 / sa / 1e12:.2f} TB/s of rows), "
              f"torch {sta * 1e3:.3f} ms (torch / ours {sta / sa:.2f}); update {su * 1e3:.3f} ms "
              f"({a.n * a.dim * 4.0 / su / 1e12:.2f} TB/s of rows), torch {stu * 1e3:.3f} ms (torch / ours {stu / su:.2f}); "
              f"assignments agree on {100 * agree:.4f} % of the rows", flush=True)
    res = {"shapes": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    g.destroy()


if __name__ == "__main__":
    main()
