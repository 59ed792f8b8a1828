"""la_verify_assignment_device[_on] with LA_FLAG_VERIFY_LARGE on the GPU, through the C ABI: topics over the 4 096 x 4 096 limit of
one workgroup's LDS, verified by the global form (tables in device memory).  The yardstick is sharding.verify_assignment_numpy
with its limits raised, which tests/test_verify_large_cpu.py holds to the oracle at the same shapes and faults
(verify_large_cases.py): every case here is equal to it on zero / non-zero, on UNCHECKED and on the four summary words, and a
catalogue fault's class bit is among those set.  Every array of a call is a guarded device buffer, as in test_verify_gpu.py."""
import copy
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from oracle import oracle

import offset_cases
import verify_cases as V
import verify_large_cases as L
from gpu_helpers import SENTINEL, _grouped_expect, _workload, shifts_for
from test_verify_gpu import INPUTS, OUTPUTS, RESULTS, Run, _faulty, _stream

pytestmark = pytest.mark.gpu

FLAG = N.LA_FLAG_VERIFY_LARGE
CLEAN = [0, 0, -1, -1]


class LargeRun(Run):
    """test_verify_gpu.Run with LA_FLAG_VERIFY_LARGE (flags=0: without it); the expectation is the yardstick without a limit
    when the flag is set, with the limit of 4 096 when it is not."""

    def __init__(self, ctx, w, res, stream, flags=FLAG, **kw):
        self.flagged = bool(flags & FLAG)
        super().__init__(ctx, w, res, stream, flags=flags, **kw)

    def expect(self, res=None):
        res = self.res if res is None else res
        kw = {"lag": self.w.lag} if self.form == "lag" else {
            "begin": self.w.begin if self.form == "offsets" else None, "end": self.w.end, "committed": self.w.committed,
            "reset_latest": self.latest}
        res = (res[0], res[1], res[2] if self.totals else None)
        return L.yardstick(self.w, res, **kw) if self.flagged else V.yardstick(self.w, res, **kw)


# ---- shapes: these two fail without the feature / guard the opt-in ----------------------------------------------------------------
def test_every_large_shape_is_certified_with_the_flag(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = L.shape_batch()
    r = LargeRun(ctx, w, V.oracle_result(w), stream)
    ctx.sync(stream)
    got_v, got_s = r.check("the shape batch")
    assert not got_v.any(), "topics %s: %s" % (np.flatnonzero(got_v), got_v[got_v != 0])
    assert list(got_s) == CLEAN
    assert 1 < r.launches <= N.VERIFY_MAX_LAUNCHES


def test_without_the_flag_large_topics_read_unchecked_as_before(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = L.shape_batch()
    r = LargeRun(ctx, w, V.oracle_result(w), stream, flags=0)
    ctx.sync(stream)                                                 # data, not an error
    got_v, got_s = r.check("the shape batch, no flag")
    want_v, want_s = L.unflagged_pattern(w)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_s, want_s)
    assert r.launches == 1 and int(got_s[1]) == len(L.LARGE) == 12


def test_a_fault_in_every_topic_of_the_shape_batch(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = L.shape_batch()
    r = LargeRun(ctx, w, _faulty(w, V.oracle_result(w)), stream)
    ctx.sync(stream)
    got_v, got_s = r.check("a fault per topic")
    assert got_v.all() and list(got_s) == [w.n_topics, 0, 0, -1]


# ---- the catalogue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", L.CATALOGUE_SHAPES)
def test_every_fault_of_the_catalogue_in_a_large_topic(ctx, torch_dev, shape):
    stream = _stream(torch_dev[0])
    w = L.catalogue_batch(shape)
    exp = V.oracle_result(w)
    cases = [c for c in V.catalogue_cases(w, exp) if c[1] == 1]
    assert len(cases) >= 6
    runs = [LargeRun(ctx, w, res, stream) for _, _, res in cases]
    ctx.sync(stream)
    for (name, t, _), r in zip(cases, runs):
        got_v, got_s = r.check("%s at %s" % (name, shape))
        assert got_v[t] & V.CATALOGUE[name], "%s at %s: verdict %d lacks its class bit" % (name, shape, got_v[t])
        assert list(np.flatnonzero(got_v)) == [t] and list(got_s) == [1, 0, t, -1]      # the small topics on both sides stay certified


def test_large_topics_side_by_side_fail_each_in_its_own_way(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    shapes = [(30, 5), (5000, 37), (4100, 4097), (64, 8), (8193, 1), (5000, 0), (6000, 50), (12289, 4099), (10, 2)]
    w = L.batch(shapes, 31)
    exp = V.oracle_result(w)
    faults = {2: "swap owners inside a round, totals tie", 4: "repeated id", 5: "rank in a topic without consumers", 7: "total + 2^63",
              8: "swap neighbours, different lags"}
    res = exp
    for t, name in faults.items():
        res = V.mutate(name, w, res, t)
        assert res is not None, name
    clean, bad = LargeRun(ctx, w, exp, stream), LargeRun(ctx, w, res, stream)
    ctx.sync(stream)
    assert clean.launches == bad.launches
    assert not clean.check("side by side")[0].any()
    got_v, got_s = bad.check("side by side, faulty")
    assert list(np.flatnonzero(got_v)) == sorted(faults) and list(got_s) == [5, 0, 2, -1]
    for t, name in faults.items():
        assert got_v[t] & V.CATALOGUE[name], "%s in topic %d: verdict %d" % (name, t, got_v[t])


# ---- unverifiable input in a large topic -------------------------------------------------------------------------------------------
def test_duplicate_input_ids_and_swapped_ranks_in_large_topics_are_unchecked(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w0 = L.batch([(64, 8), (5000, 37), (30, 5), (300, 4097), (6000, 3)], 32)
    exp = V.oracle_result(w0)
    w = copy.copy(w0)
    w.partition_id, w.cons_rank = w0.partition_id.copy(), w0.cons_rank.copy()
    a = int(w.part_off[1])
    w.partition_id[a + 7] = w.partition_id[a + 4321]                 # topic 1: a duplicate input id
    k = int(w.cons_off[3])
    w.cons_rank[[k + 2000, k + 2001]] = w.cons_rank[[k + 2001, k + 2000]]      # topic 3: two ranks swapped
    r = LargeRun(ctx, w, exp, stream)
    ctx.sync(stream)                                                 # LA_OK: data
    got_v, got_s = r.check("duplicate ids, swapped ranks")
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, 0, V.UNCHECKED, 0])
    np.testing.assert_array_equal(got_s, [0, 2, -1, 1])


# ---- host and device offsets that disagree -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [(4500, 2), (45, 2)], ids=["beside a listed topic", "the host lists none"])
def test_host_offsets_that_split_a_large_topic_are_a_shape_error_and_the_topic_is_unchecked(ctx, torch_dev, last):
    stream = _stream(torch_dev[0])
    w = L.batch([(64, 8), (5000, 37), (0, 0), (30, 5), last], 33)
    exp = V.oracle_result(w)
    r = LargeRun(ctx, w, exp, stream, call=False)
    h_po = r.h_po.copy()
    h_po[2] = h_po[1] + 2500                                         # the host: topic 1 and topic 2 hold 2 500 partitions each
    r.batch.h_part_off = h_po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    r.verify(ctx, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    got_v, got_s = r.g["verdict"].values(), r.g["summary"].values()
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, 0, 0, 0])  # (the device's topic 2 is empty)
    np.testing.assert_array_equal(got_s, [0, 1, -1, 1])
    for name, g in r.g.items():
        g.check_guards(name) if name in OUTPUTS else g.check_unchanged(name)
    r = LargeRun(ctx, w, exp, stream)                                # the next call on the context is an ordinary one
    ctx.sync(stream)
    assert not r.check("after the shape error")[0].any()


def test_a_large_topic_of_the_host_list_with_other_device_offsets_is_unchecked(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = L.batch([(64, 8), (5000, 37), (200, 9), (30, 5)], 34)
    exp = V.oracle_result(w)
    r = LargeRun(ctx, w, exp, stream, call=False)
    h_po = r.h_po.copy()
    h_po[2] += 100                                                   # the host: topic 1 holds 5 100 partitions, topic 2 holds 100
    r.batch.h_part_off = h_po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    r.verify(ctx, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    got_v, got_s = r.g["verdict"].values(), r.g["summary"].values()
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, 0, 0])     # (topic 2 is within the limit: the LDS form reads the device's offsets)
    np.testing.assert_array_equal(got_s, [0, 1, -1, 1])
    for name, g in r.g.items():
        g.check_guards(name) if name in OUTPUTS else g.check_unchanged(name)


def test_the_flag_requires_host_offsets_that_ascend_inside_the_arrays(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = L.batch([(64, 8), (5000, 37), (30, 5)], 35)
    exp = V.oracle_result(w)
    r = LargeRun(ctx, w, exp, stream, call=False)
    i64p = ctypes.POINTER(ctypes.c_int64)
    ptr = lambda a: a.ctypes.data_as(i64p)                            # (a pointer read back from the struct is a view of its field)

    def refused():
        with pytest.raises(N.LagAssignError) as ei:
            r.verify(ctx, stream)
        assert ei.value.code == N.LA_EINVAL

    r.batch.h_part_off = None
    refused()
    r.batch.h_part_off, r.batch.h_cons_off = ptr(r.h_po), None
    refused()
    bad = r.h_po.copy()
    bad[1], bad[2] = bad[2], bad[1]                                  # descending
    r.batch.h_part_off, r.batch.h_cons_off = ptr(bad), ptr(r.h_co)
    refused()
    bad2 = r.h_po.copy()
    bad2[3] += 1                                                     # past n_partitions
    r.batch.h_part_off = ptr(bad2)
    refused()
    ctx.sync(stream)
    assert (r.g["verdict"].values() == SENTINEL).all() and (r.g["summary"].values() == SENTINEL).all()      # nothing was enqueued
    r.batch.h_part_off = None                                        # without the flag nobody looks at them
    r.batch.flags, r.flagged = 0, False
    r.verify(ctx, stream)
    ctx.sync(stream)
    np.testing.assert_array_equal(r.check("no flag, no host offsets")[0], [0, V.UNCHECKED, 0])
    r.batch.h_part_off, r.batch.flags, r.flagged = ptr(r.h_po), FLAG, True
    r.verify(ctx, stream)
    ctx.sync(stream)
    assert not r.check("after the refusals")[0].any()


# ---- values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lags", ["equal", "zero", "wrap", "negative"])
def test_lag_values_in_large_topics(ctx, torch_dev, lags):
    """(9000, 1): 9 000 rounds in 95 chunks of 95, the totals wrap inside the chunk scan; (5000, 37): a partial last round."""
    stream = _stream(torch_dev[0])
    w = L.batch([(9000, 1), (40, 6), (5000, 37)], 36, lags=lags, ids="full")
    exp = V.oracle_result(w)
    runs = [(True, LargeRun(ctx, w, exp, stream)), (False, LargeRun(ctx, w, _faulty(w, exp, 2), stream))]
    for name in ("swap neighbours, equal lags", "swap owners inside a round, totals tie", "swap owners inside a round", "total + 2^63"):
        m = V.mutate(name, w, exp, 2)
        if m is not None:
            runs.append((False, LargeRun(ctx, w, m, stream)))
    ctx.sync(stream)
    for clean, r in runs:
        got_v, _ = r.check(lags)
        assert got_v.any() != clean


def test_lags_from_offsets_in_both_reset_modes_in_a_large_topic(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = offset_cases.make_case(((100, 16), (5000, 37), (7, 0)), "full-range", "50%")
    runs = []
    for latest in (True, False):
        lag = offset_cases.java_lags(w.begin, w.end, w.committed, latest)
        exp = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
        runs.append((True, LargeRun(ctx, w, exp, stream, form="offsets", latest=latest)))
        runs.append((False, LargeRun(ctx, w, exp, stream, form="offsets", latest=not latest)))      # the other mode's lags
        if latest:
            runs.append((True, LargeRun(ctx, w, exp, stream, form="no begin", latest=True)))
    ctx.sync(stream)
    for clean, r in runs:
        got_v, _ = r.check("latest %s, %s" % (r.latest, r.form))
        assert got_v.any() != clean


# ---- behind the assign call ------------------------------------------------------------------------------------------------------
E2E = {
    "block": (lambda: L.batch([(10000, 128)], 41), 0),
    "large, bins in LDS": (lambda: L.batch([(20000, 300)], 42), 0),
    "large, bins in HBM": (lambda: L.batch([(10000, 8200)], 43), 0),
    "ragged": (lambda: L.batch([(256, 32)] * 6 + [(10000, 128), (1000, 60), (20000, 300), (0, 3), (5, 9)], 44), N.LA_FLAG_RAGGED),
}


@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end_behind_the_assign_call_on_one_stream(ctx, torch_dev, case):
    make, flags = E2E[case]
    w = make()
    exp = V.oracle_result(w)
    stream = _stream(torch_dev[0])
    r = LargeRun(ctx, w, None, stream, flags=flags | FLAG, call=False)
    ctx.assign_batch_device(r.batch, stream)
    r.verify(ctx, stream)                                            # no sync in between
    ctx.sync(stream)                                                 # the first wait
    assert r.launches <= N.VERIFY_MAX_LAUNCHES
    certified = (np.zeros(w.n_topics, np.int32), np.array(CLEAN))
    got_v, _ = r.check(case, exp=certified, results_written=True)
    assert not got_v.any()
    for name, e in zip(RESULTS, exp):                                # (it certified what the oracle computes)
        np.testing.assert_array_equal(r.g[name].values(), e, err_msg=name)
    # one word of the result flipped afterwards: not certified any more
    import torch
    t = w.n_topics - 1 if case != "ragged" else 8
    at = int(w.part_off[t]) + int(w.part_off[t + 1] - w.part_off[t]) // 2
    g = r.g["out_rank"]
    raw = g.raw[g.start + 4 * at:g.start + 4 * at + 4]
    word = raw.cpu().numpy().view(np.int32).copy()
    word[0] ^= 1
    raw.copy_(torch.from_numpy(word.view(np.uint8)).to(raw.device))
    torch.cuda.synchronize()
    r.verify(ctx, stream)
    ctx.sync(stream)
    got_v = r.g["verdict"].values()
    assert list(np.flatnonzero(got_v)) == [t] and not got_v[t] & V.UNCHECKED


# ---- launches, scratch, kept results ---------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_number_of_large_topics(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    one = L.batch([(64, 8), (5000, 37), (30, 5)], 51)
    five = L.batch([(64, 8)] + [(5000, 37), (4100, 4097), (9000, 2), (30, 5)] * 2 + [(20000, 3)], 52)
    none = L.batch([(64, 8), (4096, 4096), (30, 5)], 53)
    r1, r5 = LargeRun(ctx, one, V.oracle_result(one), stream), LargeRun(ctx, five, V.oracle_result(five), stream)
    n_flag, n_plain = LargeRun(ctx, none, V.oracle_result(none), stream), LargeRun(ctx, none, V.oracle_result(none), stream, flags=0)
    ctx.sync(stream)
    for r in (r1, r5, n_flag, n_plain):
        assert not r.check("launches")[0].any()
    assert r1.launches == r5.launches <= N.VERIFY_MAX_LAUNCHES
    assert n_flag.launches == n_plain.launches == 1


def test_results_kept_for_group_last_by_member_survive_the_flagged_call(torch_dev):
    torch, _ = torch_dev
    c = N.Context(0)
    try:
        w = _workload(17, 0.05)
        m = int(w.cons_rank.max()) + 1
        first, topic, pid, e_tot, _ = _grouped_expect(w, m)
        _, _, tot = c.assign_batch(w.part_off, w.partition_id, w.begin, w.end, w.committed, N.LA_RESET_EARLIEST, w.cons_off,
                                   w.cons_rank, keep_on_device=True)
        np.testing.assert_array_equal(tot, e_tot)
        other = L.batch([(64, 8), (70001, 600), (4100, 4097)], 54)   # unrelated device arrays, the global form's scratch grows
        stream = _stream(torch)
        r = LargeRun(c, other, V.oracle_result(other), stream)
        c.sync(stream)
        assert not r.check("unrelated arrays")[0].any()
        off, g_t, g_p = c.group_last_by_member(w.n_partitions, m)
        np.testing.assert_array_equal(off, first)
        np.testing.assert_array_equal(g_t, topic)
        np.testing.assert_array_equal(g_p, pid)
    finally:
        c.close()


# ---- buffer contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["aligned", "odd", "three", "mixed"])
def test_buffer_contract_with_two_large_topics(ctx, torch_dev, pattern):
    stream = _stream(torch_dev[0])
    shifts = shifts_for(pattern, INPUTS + RESULTS + OUTPUTS)
    w = L.two_large_batch()
    exp = V.oracle_result(w)
    hw = offset_cases.make_case(((100, 16), (4099, 5), (7, 0)), "full-range", "50%")
    h_exp = oracle.assign_flat(hw.part_off, hw.partition_id, offset_cases.java_lags(hw.begin, hw.end, hw.committed, False), hw.cons_off,
                               hw.cons_rank)
    runs = [LargeRun(ctx, w, exp, stream, shifts=shifts), LargeRun(ctx, w, _faulty(w, exp), stream, shifts=shifts),
            LargeRun(ctx, hw, h_exp, stream, form="offsets", latest=False, shifts=shifts)]
    ctx.sync(stream)
    assert not runs[0].check(pattern)[0].any()
    assert runs[1].check(pattern + ", faulty")[0].all()
    assert not runs[2].check(pattern + ", offsets")[0].any()


# ---- shards ------------------------------------------------------------------------------------------------------------------------
def test_on_shard_one_of_a_two_shard_context(torch_dev):
    c2 = N.Context([0, 0])
    try:
        stream = c2.shard_stream(1)
        w = L.catalogue_batch((5000, 37))
        exp = V.oracle_result(w)
        r = LargeRun(c2, w, exp, stream, shard=1)
        bad = LargeRun(c2, w, V.mutate("repeated id", w, exp, 1), stream, shard=1)
        c2.sync(stream, shard=1)
        assert 1 < r.launches <= N.VERIFY_MAX_LAUNCHES
        assert not r.check("shard 1")[0].any()
        assert bad.check("shard 1, faulty")[0][1] & V.IDS
    finally:
        c2.close()
