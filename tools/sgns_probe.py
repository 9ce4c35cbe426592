#!/usr/bin/env python3
"""How fast does the skip-gram trainer run against the float-atomic rate?

Times one full pass over the corpus of an RMAT graph (k_sgns_train, one wave per walk) and one pass
over the affected walks of a 10 k-edge insert batch, and reports centres/s and added bytes/s as a
share of the chip-wide float-atomic rate (about 1.3 TB/s of added bytes on an MI355X).  A centre adds
(contexts + kept targets) * dim * 4 bytes; the mean of that factor is measured on a sample of walks
from the trainer's own draws.

    python tools/sgns_probe.py [--scale 20] [--out profiles/sgns_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ATOMIC_RATE = 1.3e12   # bytes/s of float atomic adds, chip-wide


def rows_per_centre(sg, ids):
    """Mean (contexts + kept targets) per centre over the listed walks, from the trainer's draws."""
    s = sg.samples(ids)
    L = s.shape[1]
    b = s[..., 0].astype(np.int64)
    lens = (b > 0).sum(axis=1)[:, None]
    pos = np.arange(L)[None, :]
    live = b > 0
    ctx = np.minimum(pos + b, lens - 1) - np.maximum(pos - b, 0)
    tgt = 1 + (s[..., 1:] != 0xFFFFFFFF).sum(axis=2)
    has = live & (ctx > 0)
    return float((ctx + tgt)[has].sum()) / max(int(live.sum()), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--samples", type=int, default=0, help="RMAT edge samples (default 10.25 per vertex)")
    ap.add_argument("--wpv", type=int, default=10)
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import dynamicgraphrepresentationlearning_amd as W
    n = 1 << a.scale
    cfg = W.WharfConfig(walks_per_vertex=a.wpv, walk_length=a.length, deterministic=False, seed=5, model=W.DEEPWALK)
    g = W.WharfMH.from_rmat(n, a.samples or (n * 41) // 4, 2 * n, seed=2, config=cfg)
    g.generate_initial_random_walks()
    sg = W.SkipGram(g, dim=a.dim, window=a.window, negatives=a.negatives)
    sg.refresh_noise()
    walks = g.number_of_walks
    ids = np.random.default_rng(1).choice(walks, size=min(walks, 20000), replace=False).astype(np.uint32)
    rows = rows_per_centre(sg, ids)
    res = {"scale": a.scale, "walks": walks, "walk_length": a.length, "dim": a.dim, "window": a.window,
           "negatives": a.negatives, "rows_added_per_centre": rows, "full": [], "affected": []}

    def record(r, what):
        s = r["kernel_ms"] * 1e-3
        added = r["centres"] * rows * a.dim * 4
        e = {"kernel_ms": r["kernel_ms"], "centres": r["centres"], "terms": r["terms"],
             "loss_per_term": r["loss"] / max(r["terms"], 1), "centres_per_s": r["centres"] / s,
             "added_bytes_per_s": added / s, "share_of_atomic_rate": added / s / ATOMIC_RATE}
        res[what].append(e)
        print(f"{what}: {e['kernel_ms']:.2f} ms, {e['centres_per_s'] / 1e6:.1f} M centres/s, "
              f"{e['added_bytes_per_s'] / 1e12:.3f} TB/s added = {100 * e['share_of_atomic_rate']:.1f} % of the "
              f"atomic rate, loss/term {e['loss_per_term']:.4f}", flush=True)
        return e

    for p in range(a.passes):
        record(sg.train(pass_=p), "full")
    out = torch.zeros(walks, dtype=torch.int32, device="cuda")
    for b in range(2):
        batch = W.generate_batch_of_edges(5000, n, 100 + b, False, False)
        aff = g.insert_edges_batch(batch, out=out)
        st = g.stats()
        e = record(sg.train(aff, pass_=a.passes + b), "affected")
        e.update(batch_edges=int(len(batch)), affected_walks=int(aff.numel()),
                 rewalk_ms=st["last_walk_update_ms"], graph_update_ms=st["last_graph_update_ms"])
        print(f"  batch {b}: {aff.numel()} affected walks, re-walk {st['last_walk_update_ms']:.2f} ms", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    g.destroy()


if __name__ == "__main__":
    main()
