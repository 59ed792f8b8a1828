"""Per-member roll-up of an assignment, the parts that need no device: the host restatement (sharding.member_loads_numpy) against a
deliberately naive loop over the ORACLE's results, the C ABI's declarations against the binding and the built library, and
the compiled ISA of csrc/la_loads.hip (hipcc cross-compiles gfx950 without a GPU)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc")
MASK = (1 << 64) - 1


def _fold(x):
    """An unbounded Python int as Java's long."""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def naive_loads(out_member_rank, cons_rank, out_total_lag, n_members):
    parts, lag, unassigned = {}, {}, 0
    for r in out_member_rank.tolist():
        if r == -1:
            unassigned += 1
        else:
            parts[r] = parts.get(r, 0) + 1
    for r, t in zip(cons_rank.tolist(), out_total_lag.tolist()):
        lag[r] = (lag.get(r, 0) + t) & MASK
    assert all(0 <= r < n_members for r in list(parts) + list(lag))
    return (np.array([parts.get(r, 0) for r in range(n_members)], np.int64),
            np.array([_fold(lag.get(r, 0)) for r in range(n_members)], np.int64), unassigned)


def _check(w, n_members, what):
    """member_loads_numpy == the naive loop over the oracle's assignment of `w`, plus the invariants; returns the true
    (unwrapped) per-member sums."""
    _, e_rank, e_tot = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    got = sharding.member_loads_numpy(e_rank, w.cons_rank, e_tot, n_members)
    exp = naive_loads(e_rank, w.cons_rank, e_tot, n_members)
    np.testing.assert_array_equal(got[0], exp[0], err_msg="partitions " + what)
    np.testing.assert_array_equal(got[1], exp[1], err_msg="lag " + what)
    assert got[2] == exp[2], what
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[0].shape == got[1].shape == (n_members,)
    assert int(got[0].sum()) + got[2] == w.n_partitions
    # every lag of a topic WITH consumers ends up in exactly one consumer's total
    has = np.repeat(np.diff(w.cons_off) > 0, np.diff(w.part_off))
    all_lags = sum(int(x) for x in w.lag[has].tolist())
    assert _fold(sum(int(x) for x in got[1].tolist())) == _fold(all_lags), what
    assert got[2] == int((~has).sum())
    true = {}
    for r, t in zip(w.cons_rank.tolist(), e_tot.tolist()):
        true[r] = true.get(r, 0) + t
    return got, true


def test_reference_readme_vector():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
    for case in ref["assign_exact"] + ref["assign_sets"]:
        members = sorted(case["subscriptions"])                     # ASCII ids: sorted() is String.compareTo order
        rank = {m: i for i, m in enumerate(members)}
        topics = list(case["lags"])
        po, co, pid, lag, cr = [0], [0], [], [], []
        for t in topics:
            for i, l in enumerate(case["lags"][t]):                  # partition i of the topic has lag l
                pid.append(i)
                lag.append(int(l))
            po.append(len(pid))
            cr += sorted(rank[m] for m in members if t in case["subscriptions"][m])
            co.append(len(cr))
        w = synth.Workload("ref", len(topics), np.array(po, np.int64), np.array(pid, np.int32), None, None, None,
                           np.array(lag, np.int64), np.array(co, np.int64), np.array(cr, np.int32), 0, 0)
        (parts, lags, unassigned), _ = _check(w, len(members), case["cite"])
        # and against the reference's own answer: who got how many
        for m in members:
            assert parts[rank[m]] == len(case["expected"][m]), (case["cite"], m)
        if "totals" in case:
            for m in members:
                assert lags[rank[m]] == int(case["totals"][m]), (case["cite"], m)   # one topic: its totals ARE the roll-up
        assert unassigned == 0


def test_ragged_batches_topics_without_consumers_and_idle_members():
    seen_unassigned = False
    for seed in range(6):
        w = synth.ragged(100 + seed, 60, 90, 12, negative=bool(seed % 2))
        m = 12 * 3 + 4                                              # ranks are drawn below 36: four members subscribe to nothing
        (parts, lags, unassigned), _ = _check(w, m, "ragged seed %d" % seed)
        assert not parts[36:].any() and not lags[36:].any()
        seen_unassigned |= unassigned > 0
    assert seen_unassigned


def test_full_range_lags_wrap_per_member():
    rng = np.random.default_rng(5)
    t, p, c = 40, 64, 4
    w = synth.make_uniform("wrap", 77, t, p, c, "zero", offsets=False)
    # 16 such lags per consumer and topic: a topic's totals stay below 2^61 (no wrap inside a topic, so the oracle's totals are
    # the true ones), 40 topics of them pass 2^63
    w.lag = rng.integers(1 << 56, 1 << 57, t * p).astype(np.int64)
    (parts, lags, unassigned), true = _check(w, c, "wrapping sums")
    assert max(true.values()) > (1 << 63) - 1, "the case must exercise the wrap"
    assert any(_fold(v) != v for v in true.values())
    np.testing.assert_array_equal(parts, np.full(c, t * p // c))
    w2 = synth.ragged(9, 50, 80, 6, dist="full", negative=True)
    _, true2 = _check(w2, 18, "full-range, negative")
    assert any(_fold(v) != v for v in true2.values())


def test_restatement_edge_cases():
    e32, e64 = np.empty(0, np.int32), np.empty(0, np.int64)
    parts, lags, unassigned = sharding.member_loads_numpy(e32, e32, e64, 3)
    assert parts.tolist() == [0, 0, 0] and lags.tolist() == [0, 0, 0] and unassigned == 0
    parts, lags, unassigned = sharding.member_loads_numpy(np.array([-1, -1], np.int32), e32, e64, 0)
    assert parts.size == 0 and lags.size == 0 and unassigned == 2
    for bad in ((np.array([3], np.int32), e32, e64), (np.array([-2], np.int32), e32, e64),
                (e32, np.array([-1], np.int32), np.array([1], np.int64)), (e32, np.array([3], np.int32), np.array([1], np.int64))):
        with pytest.raises(ValueError):
            sharding.member_loads_numpy(*bad, 3)


NEW_SYMBOLS = ("la_member_loads_device", "la_member_loads_device_on")


def test_header_binding_and_library_agree():
    from kafka_lag_based_assignor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(la_ctx \*ctx, " % name, header, re.M), name
        assert name in N.EXPORTED_SYMBOLS
    assert "#define LA_VERSION 500" in header
    lib = N.load()                                                   # loads without a GPU
    assert lib.la_version() == 500
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert callable(N.Context.member_loads_device)
    # the switch-over the tests run both sides of is the kernels' own constant
    kernels = open(os.path.join(CSRC, "la_kernels.h")).read()
    m = re.search(r"constexpr int32_t kLoadsLdsMaxMembers = (\d+);", kernels)
    assert m and int(m.group(1)) == N.LOADS_LDS_MAX_MEMBERS
    from kafka_lag_based_assignor_amd import build
    assert "la_loads.hip" in build.SOURCES


@pytest.fixture(scope="module")
def loads_isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = os.path.join(str(tmp_path_factory.mktemp("isa")), "la_loads.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                           os.path.join(CSRC, "la_loads.hip")], stderr=subprocess.DEVNULL)
    return open(dst).read()


def _instructions(text):
    return re.findall(r"^\s+([a-z][a-z0-9_]+)\b", text, re.M)


def test_isa_lds_bins_are_lds_atomics_and_the_flush_is_a_64_bit_global_add(loads_isa):
    ins = _instructions(loads_isa)
    assert any(i in ("ds_add_u32", "ds_add_rtn_u32") for i in ins), "32-bit LDS counts"
    assert any(i in ("ds_add_u64", "ds_add_rtn_u64") for i in ins), "64-bit LDS sums"
    assert any(i.startswith("global_atomic_add_x2") for i in ins), "64-bit global atomic add"
    loops = [i for i in ins if "cmpswap" in i or "cmpst" in i]
    assert not loops, "compare-and-swap loop in place of an atomic add: %s" % loops[:3]
    assert not [i for i in ins if i.startswith("flat_")], "a pointer the compiler could not place"
    assert any(i == "global_load_dwordx4" for i in ins), "16-byte loads"


def test_isa_no_kernel_of_the_unit_uses_scratch(loads_isa):
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", loads_isa)
    assert len(sizes) == 2, "member_loads_kernel<true> and <false>: %s" % sizes
    assert all(int(s) == 0 for s in sizes), sizes
    assert not [i for i in _instructions(loads_isa) if i.startswith("scratch_")]
