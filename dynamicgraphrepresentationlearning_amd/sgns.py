"""Skip-gram with negative sampling over a WharfMH handle's walk matrix.

The representation-learning half of the reference's pipeline
(experiments/src/vertex-classification.cpp:142-192 runs yskip over walks.txt,
then `yskip --initial-model` over the affected walks of every batch), trained
on the device from the resident walk matrix:

    sg = SkipGram(g, dim=128)          # after g.generate_initial_random_walks()
    sg.train()                         # yskip over the whole corpus
    aff = g.insert_edges_batch(batch, out=ids_on_gpu)
    sg.train(aff, pass_=1)             # yskip --initial-model over the affected walks

The embedding tables are torch tensors (plumbing); the trainer is the HIP
kernel k_sgns_train behind wharf_sgns_train.  Semantics: DESIGN.md §10.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

DROPPED = L.SGNS_DROPPED


def build_alias(counts, power: float = 0.75):
    """wharf_sgns_build_alias on the host: (thr, alias) u32 arrays of the weights counts**power."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    thr = np.zeros(len(c), dtype=np.uint32)
    alias = np.zeros(len(c), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib.wharf_sgns_build_alias(p(c), len(c), power, p(thr), p(alias)), None, "sgns_build_alias")
    return thr, alias


class SkipGram:
    """Two [n, dim] float32 tables on the handle's GPU and the trainer over the handle's walks."""

    def __init__(self, g, dim: int = 128, window: int = 5, negatives: int = 5, lr: float = 0.025,
                 power: float = 0.75, emb_in=None, emb_out=None, seed: int = 0):
        import torch

        self.g = g
        self.dim, self.window, self.negatives, self.lr, self.power = dim, window, negatives, lr, power
        self.n = g.number_of_vertices()
        self.device = torch.device("cuda", g.device)
        if emb_in is None:   # word2vec's rule: emb_in uniform in +-0.5/dim, emb_out zero
            gen = torch.Generator(device="cpu").manual_seed(seed)
            emb_in = ((torch.rand(self.n, dim, generator=gen) - 0.5) / dim).to(self.device)
        if emb_out is None:
            emb_out = torch.zeros(self.n, dim, dtype=torch.float32, device=self.device)
        for name, t in (("emb_in", emb_in), ("emb_out", emb_out)):
            if (t.dtype != torch.float32 or tuple(t.shape) != (self.n, dim) or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name} must be a contiguous float32 [{self.n}, {dim}] tensor on {self.device}")
        self.emb_in, self.emb_out = emb_in, emb_out

    # -- noise ------------------------------------------------------------------------------
    def refresh_noise(self) -> None:
        """Count the vertices of the current walks and rebuild the negatives' alias table."""
        L.check(L.lib.wharf_sgns_build_noise(self.g._h, self.power), self.g._h, "sgns_build_noise")

    def noise(self):
        """(counts u64[n], thr u32[n], alias u32[n]) of the last refresh_noise()."""
        counts = np.zeros(self.n, dtype=np.uint64)
        thr = np.zeros(self.n, dtype=np.uint32)
        alias = np.zeros(self.n, dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.lib.wharf_sgns_get_noise(self.g._h, p(counts), p(thr), p(alias)), self.g._h, "sgns_get_noise")
        return counts, thr, alias

    # -- calls ------------------------------------------------------------------------------
    def _params(self, pass_: int, flags: int, lr=None) -> L.wharf_sgns_params:
        p = L.wharf_sgns_params()
        p.dim, p.window, p.negatives = self.dim, self.window, self.negatives
        p.lr = self.lr if lr is None else lr
        p.pass_ = pass_
        p.flags = flags
        return p

    def _ids(self, walk_ids):
        """(pointer, count, flags, keep-alive) of a walk id list: numpy / sequence, or a 32-bit torch tensor on the GPU."""
        if walk_ids is None:
            return None, 0, 0, None
        if getattr(walk_ids, "is_cuda", False):
            import torch
            if walk_ids.dtype not in (torch.int32, torch.uint32) or not walk_ids.is_contiguous() \
                    or walk_ids.device != self.device:
                raise ValueError(f"device walk_ids must be a contiguous 32-bit tensor on {self.device}")
            return C.c_void_p(walk_ids.data_ptr()), walk_ids.numel(), L.WHARF_SGNS_WIDS_DEVICE, walk_ids
        ids = np.ascontiguousarray(walk_ids, dtype=np.uint32).reshape(-1)
        return ids.ctypes.data_as(C.c_void_p), len(ids), 0, ids

    def _sync(self) -> None:
        # the library runs on the handle's own stream: torch's pending work on the tables
        # (and on a device id list) has to be done first
        import torch
        torch.cuda.synchronize(self.device)

    def samples(self, walk_ids=None, pass_: int = 0) -> np.ndarray:
        """The trainer's draws for the listed walks: u32 [walks, L, 1 + negatives], per position
        {b, negatives...}; b = 0 past the walk's end, DROPPED for a negative equal to the centre."""
        ptr, cnt, flags, keep = self._ids(walk_ids)
        walks = self.g.number_of_walks if walk_ids is None else cnt
        out = np.zeros((walks, self.g.config.walk_length, 1 + self.negatives), dtype=np.uint32)
        p = self._params(pass_, flags)
        self._sync()
        L.check(L.lib.wharf_sgns_samples(self.g._h, C.byref(p), ptr, cnt, out.ctypes.data_as(C.c_void_p)),
                self.g._h, "sgns_samples")
        return out

    def train(self, walk_ids=None, pass_: int = 0, serial: bool = False, lr=None) -> dict:
        """One pass over the listed walks (None: every owned walk), updating emb_in / emb_out in
        place.  serial=True runs the walks one after another in list order (the reference order)."""
        ptr, cnt, flags, keep = self._ids(walk_ids)
        p = self._params(pass_, flags | (L.WHARF_SGNS_SERIAL if serial else 0), lr)
        r = L.wharf_sgns_result()
        self._sync()
        L.check(L.lib.wharf_sgns_train(self.g._h, C.byref(p), C.c_void_p(self.emb_in.data_ptr()),
                                       C.c_void_p(self.emb_out.data_ptr()), ptr, cnt, C.byref(r)),
                self.g._h, "sgns_train")
        return {"loss": r.loss, "terms": int(r.terms), "centres": int(r.centres), "kernel_ms": float(r.kernel_ms)}
