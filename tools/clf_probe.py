#!/usr/bin/env python3
"""How fast is one loss / gradient evaluation of the vertex classifier?

Times wharf_clf_loss_grad over a list of uniformly random rows of a float32 table (default 1 M rows
of a 1 M-row table, dim 128) for several class counts and reports rows/s and gathered bytes/s
(rows * dim * 4) beside the chip-wide random 16-B gather rate of profiles/gather_ceiling.json.  The
time is the wall time of the synchronous call (id check, pass, block-order reduction, loss
read-back), the best of --reps after a warm-up.  The same evaluation as a torch composition (gather,
scale, GEMM, log-softmax, GEMM) is timed for comparison.

    python tools/clf_probe.py [--rows 1048576] [--dim 128] [--classes 7,17,195] [--out profiles/clf_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def best_of(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20, help="rows of the table")
    ap.add_argument("--rows", type=int, default=1 << 20, help="listed rows")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--classes", default="7,17,195")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import dynamicgraphrepresentationlearning_amd as W
    with open(os.path.join(REPO, "profiles", "gather_ceiling.json")) as f:
        ceiling = json.load(f)["Ggathers_per_s"] * 1e9 * 16      # bytes/s of random 16-B gathers
    gen = torch.Generator(device="cuda").manual_seed(1)
    emb = torch.randn(a.n, a.dim, device="cuda", generator=gen)
    ids = torch.randint(0, a.n, (a.rows,), device="cuda", generator=gen, dtype=torch.int32)
    g = W.WharfMH(16)
    res = {"n": a.n, "rows": a.rows, "dim": a.dim, "gather_ceiling_bytes_per_s": ceiling, "cases": []}
    for C in [int(c) for c in a.classes.split(",")]:
        y = torch.randint(0, C, (a.rows,), device="cuda", generator=gen, dtype=torch.int32)
        clf = W.VertexClassifier(g, a.dim, C)
        clf.set_scaler(*clf.minmax(emb, ids))
        clf.wb = torch.randn(C, a.dim + 1, device="cuda", generator=gen) * 0.1
        grad = torch.empty_like(clf.wb)
        s = best_of(lambda: clf.loss_grad(emb, ids, y, grad=grad), a.reps)

        def composition():
            x = (emb[ids.long()] - clf.lo) * clf.scale
            logp = torch.log_softmax(x @ clf.wb[:, :-1].T + clf.wb[:, -1], dim=1)
            d = logp.exp()
            d[torch.arange(a.rows, device="cuda"), y.long()] -= 1
            gw = torch.cat([d.T @ x, d.sum(0)[:, None]], dim=1)
            loss = -logp[torch.arange(a.rows, device="cuda"), y.long()].sum().item()
            return loss, gw

        def timed_composition():
            composition()
            torch.cuda.synchronize()

        st = best_of(timed_composition, a.reps)
        loss, _ = clf.loss_grad(emb, ids, y, grad=grad)
        tl, tg = composition()
        e = {"classes": C, "ms": s * 1e3, "rows_per_s": a.rows / s, "gathered_bytes_per_s": a.rows * a.dim * 4 / s,
             "share_of_gather_ceiling": a.rows * a.dim * 4 / s / ceiling, "torch_composition_ms": st * 1e3,
             "loss": loss, "torch_loss": tl, "max_grad_difference": float((tg - grad).abs().max())}
        res["cases"].append(e)
        print(f"C {C}: {e['ms']:.3f} ms, {e['rows_per_s'] / 1e6:.1f} M rows/s, {e['gathered_bytes_per_s'] / 1e9:.1f} GB/s "
              f"gathered = {100 * e['share_of_gather_ceiling']:.1f} % of the 16-B gather rate "
              f"({ceiling / 1e9:.0f} GB/s); torch composition {e['torch_composition_ms']:.3f} ms; "
              f"loss {loss:.6g} / {tl:.6g}", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    g.destroy()


if __name__ == "__main__":
    main()
