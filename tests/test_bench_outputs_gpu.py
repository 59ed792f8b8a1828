"""bench.py's plain run and --dump-outputs on the GPU: the line holds the headline and none of the legs that --full adds,
--steps / --warmup are the counts it ran, and the arrays it dumps are the oracle's assignment of the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--settle-ms", "5"] + list(args)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_plain_run_dumps_the_oracle_assignment(tmp_path):
    from kafka_lag_based_assignor_amd import synth
    from oracle import oracle
    d = _bench("--workload", "cfg3", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert d["metric"] == "partition-assignments/sec (whole node)" and d["unit"] == "partition-assignments/sec"
    assert d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"]["kernel_ms"] > 0
    for k in ("parity", "cpu_baseline", "host_boundary", "configs", "small_call", "sort_phase", "lag_ratio", "cold_call", "cold_call_ms"):
        assert d[k] is None, k
    w = synth.config("cfg3")
    lag = oracle.compute_lags(w.begin, w.end, w.committed, False)
    e_pid, e_rank, e_tot = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
    got = {n: np.load(os.path.join(tmp_path, n + ".npy")) for n in ("partition_id", "member_rank", "total_lag")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["partition_id"], e_pid.astype(np.float64))          # 256 000 and 32 000 elements: written whole
    assert np.array_equal(got["member_rank"], e_rank.astype(np.float64))
    assert np.array_equal(got["total_lag"], e_tot.astype(np.float64))


@pytest.mark.timeout(900)
def test_sort_phase_runs_the_steps_it_is_given_and_dumps_the_order(tmp_path):
    import bench
    n = 100000
    d = _bench("--phase", "sort", "--partitions", str(n), "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 4 and d["warmup"] == 2 and d["roofline"]["sorted_ok"] is True
    w = bench.sort_phase_workload(n)
    order = np.lexsort((w.partition_id, -w.lag))                                   # lag descending, then partition id
    assert np.array_equal(np.load(os.path.join(tmp_path, "partition_id.npy")), w.partition_id[order].astype(np.float64))
