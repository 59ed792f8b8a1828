"""la_verify_assignment_device[_on] on the GPU, through the C ABI.  The yardstick is sharding.verify_assignment_numpy, which
tests/test_verify_cpu.py holds to the oracle at the same shapes and faults (verify_cases.py): every case here is equal to it on
zero / non-zero, on UNCHECKED and on the four summary words, and a catalogue fault's class bit is among those set.  Every array
of a call is a guarded device buffer: the inputs and the results under test must come back byte for byte, guard bands included."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from oracle import oracle

import offset_cases
import verify_cases as V
from gpu_helpers import SENTINEL, Guarded, _grouped_expect, _workload, shifts_for

pytestmark = pytest.mark.gpu

INPUTS = ("part_off", "partition_id", "begin", "end", "committed", "lag", "cons_off", "cons_rank")
RESULTS = ("out_pid", "out_rank", "out_total")
OUTPUTS = ("verdict", "summary")
I64P = ctypes.POINTER(ctypes.c_int64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One verify call on guarded device buffers.  form: "lag" (d_lag), "offsets" (begin / end / committed) or "no begin"
    (offsets, d_begin_off NULL).  res: the results under test (None: SENTINEL, for an assign call to fill)."""

    def __init__(self, ctx, w, res, stream, form="lag", latest=True, shifts=None, want=OUTPUTS, totals=True, shard=None, hint=None,
                 flags=0, algo=N.LA_ALGO_AUTO, call=True):
        shifts = shifts or {}
        self.w, self.res, self.form, self.latest, self.totals = w, res, form, latest, totals
        n, k, t = w.n_partitions, w.cons_rank.size, w.n_topics
        arrays = {"part_off": w.part_off, "partition_id": w.partition_id, "cons_off": w.cons_off, "cons_rank": w.cons_rank}
        if form == "lag":
            arrays["lag"] = w.lag
        else:
            arrays["end"], arrays["committed"] = w.end, w.committed
            if form == "offsets":
                arrays["begin"] = w.begin
        self.g = {name: Guarded("device", a.size, a.dtype, shifts.get(name, 0), a, name=name) for name, a in arrays.items()}
        for name, size, dtype, a in (("out_pid", n, np.int32, None if res is None else res[0]),
                                     ("out_rank", n, np.int32, None if res is None else res[1]),
                                     ("out_total", k, np.int64, None if res is None else res[2])):
            self.g[name] = Guarded("device", size, dtype, shifts.get(name, 0), a, name=name)
        self.g["verdict"] = Guarded("device", t, np.int32, shifts.get("verdict", 0), name="verdict")
        self.g["summary"] = Guarded("device", 4, np.int64, shifts.get("summary", 0), name="summary")
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, (N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST), algo, flags
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = hint or (w.max_partitions, w.max_consumers)
        ptr = lambda name: self.g[name].ptr if name in self.g else None
        b.d_part_off, b.d_partition_id, b.d_cons_off, b.d_cons_rank = ptr("part_off"), ptr("partition_id"), ptr("cons_off"), ptr("cons_rank")
        b.d_begin_off, b.d_end_off, b.d_committed_off, b.d_lag = ptr("begin"), ptr("end"), ptr("committed"), ptr("lag")
        b.d_out_partition, b.d_out_member_rank = ptr("out_pid"), ptr("out_rank")
        b.d_out_total_lag = ptr("out_total") if totals else None
        self.h_po, self.h_co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)      # kept alive
        b.h_part_off, b.h_cons_off = self.h_po.ctypes.data_as(I64P), self.h_co.ctypes.data_as(I64P)
        self.batch = b
        self.v_ptr = self.g["verdict"].ptr if "verdict" in want else 0
        self.s_ptr = self.g["summary"].ptr if "summary" in want else 0
        self.want = want
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        if call:
            self.verify(ctx, stream, shard)

    def verify(self, ctx, stream, shard=None):
        ctx.verify_assignment_device(self.batch, self.v_ptr, self.s_ptr, stream, shard=shard)
        self.launches = ctx.last_launches()

    def expect(self, res=None):
        res = self.res if res is None else res
        kw = {"lag": self.w.lag} if self.form == "lag" else {
            "begin": self.w.begin if self.form == "offsets" else None, "end": self.w.end, "committed": self.w.committed,
            "reset_latest": self.latest}
        return V.yardstick(self.w, (res[0], res[1], res[2] if self.totals else None), **kw)

    def check(self, what="", exp=None, results_written=False):
        """After the sync: verdicts and summary against the yardstick, untouched inputs and results, guard bands."""
        verdict, summary = self.expect() if exp is None else exp
        got_v, got_s = self.g["verdict"].values(), self.g["summary"].values()
        if "verdict" in self.want:
            np.testing.assert_array_equal(got_v != 0, verdict != 0, err_msg="zero / non-zero %s: device %s" % (what, got_v[:16]))
            np.testing.assert_array_equal(got_v & V.UNCHECKED, verdict & V.UNCHECKED, err_msg="UNCHECKED %s" % what)
            assert ((got_v & V.UNCHECKED) == 0).all() or (got_v[(got_v & V.UNCHECKED) != 0] == V.UNCHECKED).all()
            assert ((got_v & ~63) == 0).all(), "unknown verdict bits %s" % what
        else:
            assert (got_v == SENTINEL).all(), "the verdicts were not asked for %s" % what
        if "summary" in self.want:
            np.testing.assert_array_equal(got_s, summary, err_msg="summary %s" % what)
        else:
            assert (got_s == SENTINEL).all(), "the summary was not asked for %s" % what
        for name, g in self.g.items():
            if name in OUTPUTS or (results_written and name in RESULTS):
                g.check_guards(what)
            else:
                g.check_unchanged(what)
        return got_v, got_s


def _faulty(w, exp, every=1):
    """A fault in every `every`-th topic: a total off by one where there are consumers, a foreign id where there are only
    partitions."""
    res = tuple(a.copy() for a in exp)
    for t in range(0, w.n_topics, every):
        p, c = int(w.part_off[t + 1] - w.part_off[t]), int(w.cons_off[t + 1] - w.cons_off[t])
        m = V.mutate("total + 1" if c else "foreign id", w, res, t)
        if m is not None:
            res = m
    return res


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", V.SHAPE_P)
def test_shapes_certified_and_faulty(ctx, torch_dev, p):
    stream = _stream(torch_dev[0])
    w = V.batch(V.shapes_of(p), p)
    exp = V.oracle_result(w)
    r = Run(ctx, w, exp, stream)
    bad = Run(ctx, w, _faulty(w, exp), stream)
    ctx.sync(stream)
    assert r.launches == 1 and bad.launches == 1
    got_v, got_s = r.check("P = %d" % p)
    assert not got_v.any() and list(got_s) == [0, 0, -1, -1]
    got_v, _ = bad.check("P = %d, a fault per topic" % p)
    assert got_v.any() or p == 0


def test_full_and_partial_last_rounds(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.batch(V.ROUND_SHAPES, 1)
    exp = V.oracle_result(w)
    runs = [Run(ctx, w, exp, stream), Run(ctx, w, _faulty(w, exp, 2), stream)]
    for t in range(w.n_topics):                                      # the last picked consumer replaced, topic by topic
        m = V.mutate("partial last round: an unpicked consumer for the last picked", w, exp, t)
        if m is not None:
            runs.append(Run(ctx, w, m, stream))
    assert len(runs) > 8
    ctx.sync(stream)
    assert not runs[0].check("round shapes")[0].any()
    for r in runs[1:]:
        assert r.check("round shapes, faulty")[0].any()


def test_more_topics_than_workgroups_with_small_topics_behind_large_ones(ctx, torch_dev):
    """At the limit's LDS request one workgroup fits a CU, so the grid is the CU count; topics t, t + 256, t + 512, ... share a
    workgroup on a 256-CU device: a 4096-partition topic, then a 1-partition topic, then an empty one, then 65 x 64."""
    stream = _stream(torch_dev[0])
    g = 256
    shapes = [((V.LIMIT, V.LIMIT if t % 64 == 0 else 5) if t % 4 == 0 else (7, 3)) for t in range(g)]
    shapes += [(1, 2)] * g + [(0, 1)] * g + [(65, 64)] * g
    w = V.batch(shapes, 9)
    exp = V.oracle_result(w)
    hint = (V.LIMIT, V.LIMIT)
    clean = Run(ctx, w, exp, stream, hint=hint)
    res = exp
    for t in range(0, g, 8):                                         # every second large topic fails, each in its own way
        res = V.mutate(list(V.CATALOGUE)[(t // 8) % 9], w, res, t) or res
    for t in (g + 8, 2 * g + 16, 3 * g + 24, 4 * g - 1):             # ... and a few of the small ones behind them
        res = V.mutate("total + 2^63", w, res, t)
    bad = Run(ctx, w, res, stream, hint=hint)
    ctx.sync(stream)
    assert clean.launches == 1
    assert not clean.check("4 x 256 topics")[0].any()
    got_v, got_s = bad.check("4 x 256 topics, faults in large topics")
    assert got_s[0] >= 16 + 4 and got_s[2] == 0
    assert not got_v[g:g + 8].any() and got_v[g + 8] and not got_v[2 * g:2 * g + 16].any()


def test_topics_over_the_limit_are_unchecked_and_the_others_certified(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.batch([(64, 8), (V.LIMIT + 1, 8), (30, 5), (64, V.LIMIT + 1), (20, 3)], 4)
    r = Run(ctx, w, V.oracle_result(w), stream)
    ctx.sync(stream)                                                 # data, not an error
    got_v, got_s = r.check("over the limit")
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, 0, V.UNCHECKED, 0])
    np.testing.assert_array_equal(got_s, [0, 2, -1, 1])


# ---- values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lags", ["equal", "zero", "wrap", "negative"])
def test_lag_values_and_id_values(ctx, torch_dev, lags):
    stream = _stream(torch_dev[0])
    runs = []
    for ids in ("shuffled", "full", "4096", "2^20"):
        w = V.batch([(256, 32), (1000, 7), (5, 9), (300, 0), (0, 4), (65, 64), (700, 300)], 2, lags=lags, ids=ids)
        exp = V.oracle_result(w)
        runs += [(ids, True, Run(ctx, w, exp, stream)), (ids, False, Run(ctx, w, _faulty(w, exp, 2), stream))]
        for name in ("swap neighbours, equal lags", "swap owners inside a round, totals tie", "swap owners inside a round"):
            m = V.mutate(name, w, exp, 1)
            if m is not None:
                runs.append((ids, False, Run(ctx, w, m, stream)))
    ctx.sync(stream)
    for ids, clean, r in runs:
        got_v, _ = r.check("%s / %s" % (lags, ids))
        assert got_v.any() != clean


@pytest.mark.parametrize("regime", offset_cases.REGIMES)
def test_lags_from_hostile_offsets_in_both_reset_modes(ctx, torch_dev, regime):
    stream = _stream(torch_dev[0])
    shapes = ((256, 32), (100, 16), (1000, 7), (5, 0), (0, 3))
    w = offset_cases.make_case(shapes, regime, "50%")
    runs = []
    for latest in (True, False):
        lag = offset_cases.java_lags(w.begin, w.end, w.committed, latest)
        exp = oracle.assign_flat(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)
        runs.append((True, Run(ctx, w, exp, stream, form="offsets", latest=latest)))
        runs.append((False, Run(ctx, w, exp, stream, form="offsets", latest=not latest)))      # the other mode's lags: not its result
        if latest:
            runs.append((True, Run(ctx, w, exp, stream, form="no begin", latest=True)))
    ctx.sync(stream)
    for clean, r in runs:
        got_v, _ = r.check("%s, latest %s, %s" % (regime, r.latest, r.form))
        assert got_v.any() != clean


# ---- unverifiable input ----------------------------------------------------------------------------------------------------------
def test_duplicate_input_ids_and_unsorted_ranks_are_unchecked(ctx, torch_dev):
    import copy
    stream = _stream(torch_dev[0])
    w0 = V.batch([(64, 8), (50, 8), (30, 5), (40, 6), (300, 40)], 5)
    exp = V.oracle_result(w0)
    w = copy.copy(w0)
    w.partition_id, w.cons_rank = w0.partition_id.copy(), w0.cons_rank.copy()
    w.partition_id[64 + 7] = w.partition_id[64 + 20]                 # topic 1
    a = int(w.cons_off[3])
    w.cons_rank[[a + 1, a + 2]] = w.cons_rank[[a + 2, a + 1]]        # topic 3
    r = Run(ctx, w, exp, stream)
    w2 = copy.copy(w0)
    w2.cons_rank = w0.cons_rank.copy()
    w2.cons_rank[int(w.cons_off[4]) + 39] = w2.cons_rank[int(w.cons_off[4]) + 38]         # topic 4: its last two ranks are equal
    r2 = Run(ctx, w2, exp, stream)
    ctx.sync(stream)
    got_v, got_s = r.check("duplicate ids, unsorted ranks")
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, 0, V.UNCHECKED, 0])
    np.testing.assert_array_equal(got_s, [0, 2, -1, 1])
    np.testing.assert_array_equal(r2.check("equal ranks")[0], [0, 0, 0, 0, V.UNCHECKED])


# ---- the catalogue -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.CATALOGUE_SHAPES)
def test_every_fault_of_the_catalogue(ctx, torch_dev, shape):
    stream = _stream(torch_dev[0])
    w = V.catalogue_batch(shape)
    exp = V.oracle_result(w)
    cases = V.catalogue_cases(w, exp)
    runs = [Run(ctx, w, res, stream) for _, _, res in cases]
    ctx.sync(stream)
    for (name, t, _), r in zip(cases, runs):
        got_v, got_s = r.check("%s at %s" % (name, shape))
        assert got_v[t] & V.CATALOGUE[name], "%s at %s: verdict %d lacks its class bit" % (name, shape, got_v[t])
        assert list(np.flatnonzero(got_v)) == [t] and list(got_s) == [1, 0, t, -1]


def test_only_the_last_topic_is_faulty(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.batch([(100, 8)] * 700 + [(30, 5)], 8)
    exp = V.oracle_result(w)
    r = Run(ctx, w, V.mutate("swap neighbours, different lags", w, exp, 700), stream)
    ctx.sync(stream)
    got_v, got_s = r.check("last topic")
    assert list(got_s) == [1, 0, 700, -1] and got_v[700] & V.ORDER


# ---- behind the assign call ------------------------------------------------------------------------------------------------------
E2E = {
    "tile, packed": (lambda: V.batch([(256, 32)] * 40 + [(100, 7), (0, 3), (5, 9), (64, 0)], 11), N.LA_ALGO_AUTO, 0),
    "tile, wide": (lambda: V.batch([(256, 32)] * 40 + [(100, 7), (0, 3), (5, 9), (64, 0)], 12, lags="negative", ids="full"),
                   N.LA_ALGO_ROUNDS_WIDE, 0),
    "tile, ragged": (lambda: V.batch([(1000, 60), (3, 2), (256, 32), (0, 0), (17, 40), (700, 1)] * 5, 13), N.LA_ALGO_AUTO, N.LA_FLAG_RAGGED),
    "block": (lambda: V.batch([(3000, 200), (256, 32), (2100, 300), (0, 2)], 14), N.LA_ALGO_AUTO, 0),
    "argmin": (lambda: V.batch([(256, 32)] * 10 + [(1000, 7), (5, 9)], 15, lags="wrap"), N.LA_ALGO_ARGMIN, 0),
}


@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end_behind_the_assign_call_on_one_stream(ctx, torch_dev, case):
    make, algo, flags = E2E[case]
    w = make()
    exp = V.oracle_result(w)
    stream = _stream(torch_dev[0])
    r = Run(ctx, w, None, stream, algo=algo, flags=flags, call=False)
    ctx.assign_batch_device(r.batch, stream)
    r.verify(ctx, stream)                                            # no sync in between
    ctx.sync(stream)                                                 # the first wait
    assert r.launches == 1
    got_v, got_s = r.check(case, exp=(np.zeros(w.n_topics, np.int32), np.array([0, 0, -1, -1])), results_written=True)
    assert not got_v.any()
    for name, e in zip(RESULTS, exp):                                # (it certified what the oracle computes)
        np.testing.assert_array_equal(r.g[name].values(), e, err_msg=name)


# ---- shards, launches, kept results --------------------------------------------------------------------------------------------
def test_on_shard_one_of_a_two_shard_context(torch_dev):
    c2 = N.Context([0, 0])
    try:
        stream = c2.shard_stream(1)
        w = V.catalogue_batch((1000, 7))
        exp = V.oracle_result(w)
        r = Run(c2, w, exp, stream, shard=1)
        bad = Run(c2, w, V.mutate("repeated id", w, exp, 1), stream, shard=1)
        c2.sync(stream, shard=1)
        assert r.launches <= 1 and bad.launches <= 1
        assert not r.check("shard 1")[0].any()
        assert bad.check("shard 1, faulty")[0][1] & V.IDS
        with pytest.raises(N.LagAssignError) as ei:
            Run(c2, w, exp, stream, shard=2)
        assert ei.value.code == N.LA_EINVAL
    finally:
        c2.close()


def test_results_kept_for_group_last_by_member_survive_the_call(torch_dev):
    torch, _ = torch_dev
    c = N.Context(0)
    try:
        w = _workload(17, 0.05)
        m = int(w.cons_rank.max()) + 1
        first, topic, pid, e_tot, _ = _grouped_expect(w, m)
        _, _, tot = c.assign_batch(w.part_off, w.partition_id, w.begin, w.end, w.committed, N.LA_RESET_EARLIEST, w.cons_off,
                                   w.cons_rank, keep_on_device=True)
        np.testing.assert_array_equal(tot, e_tot)
        other = V.batch([(V.LIMIT, 300), (90, 7)], 18)               # unrelated device arrays, the largest LDS request
        stream = _stream(torch)
        r = Run(c, other, V.oracle_result(other), stream)
        c.sync(stream)
        assert r.launches == 1 and not r.check("unrelated arrays")[0].any()
        off, g_t, g_p = c.group_last_by_member(w.n_partitions, m)
        np.testing.assert_array_equal(off, first)
        np.testing.assert_array_equal(g_t, topic)
        np.testing.assert_array_equal(g_p, pid)
    finally:
        c.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.catalogue_batch((5, 9))
    exp = V.oracle_result(w)
    r = Run(ctx, w, exp, stream, call=False)

    def refused(batch, v, s):
        with pytest.raises(N.LagAssignError) as ei:
            ctx.verify_assignment_device(batch, v, s, stream)
        assert ei.value.code == N.LA_EINVAL

    refused(r.batch, 0, 0)                                           # both outputs NULL
    refused(None, r.v_ptr, r.s_ptr)
    for field in ("n_topics", "n_partitions", "n_consumers"):
        keep = getattr(r.batch, field)
        setattr(r.batch, field, -1)
        refused(r.batch, r.v_ptr, r.s_ptr)
        setattr(r.batch, field, keep)
    r.batch.flags = N.LA_FLAG_WIRE_OUT
    refused(r.batch, r.v_ptr, r.s_ptr)
    r.batch.flags = 0
    ctx.sync(stream)
    assert (r.g["verdict"].values() == SENTINEL).all() and (r.g["summary"].values() == SENTINEL).all()      # nothing was enqueued
    r.verify(ctx, stream)                                            # the same struct is an ordinary call afterwards
    ctx.sync(stream)
    assert not r.check("after the refusals")[0].any()


@pytest.mark.parametrize("want", [("verdict",), ("summary",)])
def test_either_output_may_be_left_out(ctx, torch_dev, want):
    stream = _stream(torch_dev[0])
    w = V.catalogue_batch((256, 32))
    r = Run(ctx, w, V.mutate("total + 1", w, V.oracle_result(w), 1), stream, want=want)
    ctx.sync(stream)
    r.check("only %s" % (want,))


def test_totals_are_optional(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.catalogue_batch((256, 32))
    res = V.mutate("total + 1", w, V.oracle_result(w), 1)
    with_totals, without = Run(ctx, w, res, stream), Run(ctx, w, res, stream, totals=False)
    ctx.sync(stream)
    assert with_totals.check("totals")[0][1] == V.TOTALS
    assert not without.check("no totals")[0].any()


def test_batches_without_topics_or_partitions(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    empty = V.batch([], 1)
    r0 = Run(ctx, empty, V.oracle_result(empty), stream)
    w = V.batch([(0, 3), (0, 0), (0, 2)], 7)
    r1 = Run(ctx, w, V.oracle_result(w), stream)
    e32 = np.empty(0, np.int32)
    r2 = Run(ctx, w, (e32, e32, np.array([0, 0, 0, 1, 0], np.int64)), stream)       # a total without a partition behind it
    ctx.sync(stream)
    assert r0.launches == 0 and r1.launches <= 1
    assert list(r0.check("T = 0")[1]) == [0, 0, -1, -1]
    assert list(r1.check("N = 0")[1]) == [0, 0, -1, -1]
    np.testing.assert_array_equal(r2.check("N = 0, a stray total")[0], [0, 0, V.TOTALS])


def test_offsets_that_leave_the_arrays_are_a_shape_error_and_nothing_is_read_through_them(ctx, torch_dev):
    import copy
    stream = _stream(torch_dev[0])
    w0 = V.batch([(64, 8), (50, 8), (30, 5), (40, 6)], 5)
    exp = V.oracle_result(w0)
    w = copy.copy(w0)
    w.part_off = w0.part_off.copy()
    w.part_off[2] = w0.n_partitions + (1 << 40)                      # topic 1 ends far outside, topic 2 starts there
    r = Run(ctx, w, exp, stream, call=False)
    r.batch.n_partitions = w0.n_partitions
    r.verify(ctx, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    got_v, got_s = r.g["verdict"].values(), r.g["summary"].values()
    np.testing.assert_array_equal(got_v, [0, V.UNCHECKED, V.UNCHECKED, 0])
    np.testing.assert_array_equal(got_s, [0, 2, -1, 1])
    for name, g in r.g.items():
        g.check_guards(name) if name in OUTPUTS else g.check_unchanged(name)
    r = Run(ctx, w0, exp, stream)                                    # the next call on the context is an ordinary one
    ctx.sync(stream)
    assert not r.check("after the shape error")[0].any()


def test_a_topic_over_a_hint_within_the_limit_is_a_shape_error_and_unchecked(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.batch([(64, 8), (300, 8), (30, 40), (40, 6)], 5)
    r = Run(ctx, w, V.oracle_result(w), stream, hint=(256, 32))
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    np.testing.assert_array_equal(r.g["verdict"].values(), [0, V.UNCHECKED, V.UNCHECKED, 0])
    r = Run(ctx, w, V.oracle_result(w), stream, hint=(0, -5))        # no usable hint: the limit's request
    ctx.sync(stream)
    assert not r.check("no hint")[0].any()


# ---- buffer contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["aligned", "odd", "three", "mixed"])
def test_buffer_contract_element_aligned_views_guards_and_untouched_inputs(ctx, torch_dev, pattern):
    stream = _stream(torch_dev[0])
    shifts = shifts_for(pattern, INPUTS + RESULTS + OUTPUTS)
    w = V.batch([(37, 3), (1, 1), (300, 40), (0, 2), (64, 64), (1025, 9), (5, 0)], 15)
    exp = V.oracle_result(w)
    hw = offset_cases.make_case(((256, 32), (100, 16), (7, 0)), "full-range", "50%")
    h_exp = oracle.assign_flat(hw.part_off, hw.partition_id, offset_cases.java_lags(hw.begin, hw.end, hw.committed, False), hw.cons_off,
                               hw.cons_rank)
    runs = [Run(ctx, w, exp, stream, shifts=shifts), Run(ctx, w, _faulty(w, exp), stream, shifts=shifts),
            Run(ctx, hw, h_exp, stream, form="offsets", latest=False, shifts=shifts)]
    ctx.sync(stream)
    assert not runs[0].check(pattern)[0].any()
    assert runs[1].check(pattern + ", faulty")[0].any()
    assert not runs[2].check(pattern + ", offsets")[0].any()
