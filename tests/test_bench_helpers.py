"""bench.py's host-side helpers that shape the JSON line (CPU only, no GPU, no library calls):
the gather-ceiling record, the committed PMC traffic lookup, the record-bytes readout and
the host CPU accounting behind `cpu_baseline.cores`."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_gather_ceiling_fractions_and_table_matched_probe():
    assert bench.gather_ceiling(45e9, None) is None
    rec = bench.gather_ceiling(45e9, [40.0, 45.0], {"table_GiB": 1.981, "probes": [44.0, 50.0]})
    assert rec["Ggathers_per_s_min"] == 40.0 and rec["Ggathers_per_s_max"] == 45.0
    assert rec["frac_of_min"] == pytest.approx(45 / 40, abs=1e-4)
    assert rec["frac_of_max"] == pytest.approx(1.0, abs=1e-4)
    tm = rec["table_matched"]
    assert tm["table_GiB"] == 1.981 and tm["probes"] == [44.0, 50.0]
    assert tm["frac_of_min"] == pytest.approx(45 / 44, abs=1e-4) and tm["frac_of_max"] == pytest.approx(0.9, abs=1e-4)
    # a matched record without probes (the probe binary missing) adds nothing
    assert "table_matched" not in bench.gather_ceiling(45e9, [40.0], {"table_GiB": 2.0, "probes": None})


def test_traffic_comes_from_the_newest_committed_pmc_summary():
    traffic, src = bench.load_traffic("gen_deepwalk_mh_s22")
    assert src.startswith(f"profiles/pmc_{bench.PMC_ROUNDS[0]}gen_deepwalk_mh_s22.json")
    with open(os.path.join(REPO, src.split(" ")[0])) as f:
        assert traffic == json.load(f)["hbm_bytes_per_launch"] > 0
    assert bench.load_traffic("no_such_kernel_tag") == (None, None)


class _Handle:
    """What record_bytes_per_slot reads: records_bytes = 16 B per vertex (vrec) + the edge
    records of every pool slot (the footprint counts node2vec's anchor half as samplers)."""

    def __init__(self, n, pool, per_slot):
        self.n, self.pool, self.per_slot = n, pool, per_slot

    def memory_footprint(self, verbose=False):
        return {"records_bytes": 16 * self.n + self.per_slot * self.pool}

    def stats(self):
        return {"pool_capacity": self.pool}


@pytest.mark.parametrize("per_slot,anchors,want", [(8, False, 8), (16, False, 16), (16, True, 32)])
def test_record_bytes_per_slot(per_slot, anchors, want):
    assert bench.record_bytes_per_slot(_Handle(1 << 12, 5 << 12, per_slot), 1 << 12, anchors) == want


class _Corpus:
    """What dump_outputs reads: number_of_walks, config.walk_length and export_walk_rows."""

    def __init__(self, walks):
        self.rows = walks
        self.number_of_walks = len(walks)
        self.config = type("C", (), {"walk_length": walks.shape[1]})()
        self.calls = 0

    def export_walk_rows(self, first, count, out):
        assert first + count <= len(self.rows) and out.flags.c_contiguous
        out[:count] = self.rows[first:first + count]
        self.calls += 1


@pytest.mark.parametrize("walks", [0, 1000, bench.DUMP_CHUNKS * bench.DUMP_CHUNK_ROWS + 777])
def test_dump_outputs_writes_a_fixed_sample_of_the_corpus(tmp_path, walks):
    import numpy as np
    rng = np.random.default_rng(walks)
    corpus = rng.integers(0, 1 << 32, size=(walks, 5), dtype=np.uint64).astype(np.uint32)
    if walks:
        corpus[0, -1] = 0xFFFFFFFF   # a SENTINEL pad survives the float conversion exactly
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(_Corpus(corpus), str(tmp_path / d))
        outs.append((np.load(tmp_path / d / "walks.npy"), np.load(tmp_path / d / "walk_rows.npy")))
    (w, r), (w2, r2) = outs
    assert w.dtype == np.float64 and r.dtype == np.float64
    assert np.array_equal(w, w2) and np.array_equal(r, r2)          # the same sample every run
    assert len(r) == min(walks, bench.DUMP_CHUNKS * bench.DUMP_CHUNK_ROWS) and len(np.unique(r)) == len(r)
    assert np.array_equal(w, corpus[r.astype(np.int64)].astype(np.float64))
    # the default workload's sample (L = 80) stays under the 64 MB a dump may take
    assert bench.DUMP_CHUNKS * bench.DUMP_CHUNK_ROWS * (80 + 1) * 8 <= 64 * 10 ** 6


def test_dump_outputs_names_the_rank_at_more_than_one_gpu(tmp_path):
    import numpy as np
    bench.dump_outputs(_Corpus(np.arange(20, dtype=np.uint32).reshape(4, 5)), str(tmp_path), rank=1, world=2)
    assert sorted(os.listdir(tmp_path)) == ["walk_rows_rank1.npy", "walks_rank1.npy"]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_cpu_cores_respects_an_explicit_request_and_the_host_share():
    info = bench.host_cpus()
    assert 1 <= info["usable"] <= info["nproc"]
    assert bench.cpu_cores(3) == 3
    assert bench.cpu_cores(0) == info["usable"]


def test_l2_request_rate_from_the_committed_summary():
    req = bench.load_requests("gen_deepwalk_mh_s22")
    assert req is not None and 1.0 <= req["per_step"] < 1.2 and req["source"].startswith("profiles/pmc_")
    rec = bench.request_rate(req, 3_297_052_360, 76.2)
    assert rec["G_per_s"] == pytest.approx(req["per_step"] * 3_297_052_360 / 0.0762 / 1e9, rel=1e-3)
    assert rec["path_kernels_measured_G_per_s"] == [40, 47]
    assert bench.load_requests("no_such_kernel_tag") is None and bench.request_rate(None, 1, 1.0) is None
