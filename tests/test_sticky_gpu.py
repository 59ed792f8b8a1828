"""la_sticky_ties_device on the GPU, through the C ABI.  The yardstick is sharding.sticky_ties_numpy, which tests/test_sticky_cpu.py
holds to an independent model, to brute force and to the consequences the header states, at the same cases (sticky_cases.py):
every output here is equal to it bit for bit.  Every array of a call is a guarded device buffer at an element shift; outputs
hold SENTINEL before the call, inputs must come back byte for byte, guard bands included."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

import sticky_cases as S
from gpu_helpers import SENTINEL, Guarded, shifts_for

pytestmark = pytest.mark.gpu

OUTPUTS = ("sticky", "kept", "saved", "summary")
NAMES = ("part_off", "partition_id", "lag", "begin", "end", "committed", "out_pid", "out_rank", "prev") + OUTPUTS


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One sticky call on guarded device buffers.  form: "lag" (d_lag) or "offsets" (begin / end / committed).  want: the
    optional outputs that are not NULL.  override: arrays that replace the workload's on the device (hostile input)."""

    def __init__(self, ctx, w, res, prev, stream, form="lag", latest=True, shifts="mixed", want=("kept", "saved", "summary"), hint=None,
                 override=None, n_partitions=None, call=True):
        sh = shifts_for(shifts, NAMES)
        self.w, self.res, self.prev, self.want = w, res, prev, want
        n, t = w.n_partitions, w.n_topics
        arrays = {"part_off": w.part_off, "partition_id": w.partition_id, "out_pid": res[0], "out_rank": res[1], "prev": prev}
        if form == "lag":
            arrays["lag"] = w.lag
        else:
            arrays["begin"], arrays["end"], arrays["committed"] = w.begin, w.end, w.committed
        arrays.update(override or {})
        self.g = {name: Guarded("device", a.size, a.dtype, sh[name], a, name=name) for name, a in arrays.items()}
        for name, size, dtype in (("sticky", n, np.int32), ("kept", t, np.int64), ("saved", t, np.int64), ("summary", 4, np.int64)):
            self.g[name] = Guarded("device", size, dtype, sh[name], name=name)
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, (N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST), N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = (n if n_partitions is None else n_partitions), 0
        b.max_partitions_per_topic, b.max_consumers_per_topic = (w.max_partitions if hint is None else hint), 0
        ptr = lambda name: self.g[name].ptr if name in self.g else None
        b.d_part_off, b.d_partition_id = ptr("part_off"), ptr("partition_id")
        b.d_begin_off, b.d_end_off, b.d_committed_off, b.d_lag = ptr("begin"), ptr("end"), ptr("committed"), ptr("lag")
        b.d_out_partition, b.d_out_member_rank = ptr("out_pid"), ptr("out_rank")
        self.batch = b
        a = N.StickyArgs()
        a.d_prev_owner, a.d_sticky_partition = ptr("prev"), ptr("sticky")
        a.d_topic_kept = ptr("kept") if "kept" in want else None
        a.d_topic_saved = ptr("saved") if "saved" in want else None
        a.d_summary = ptr("summary") if "summary" in want else None
        self.args = a
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        if call:
            ctx.sticky_ties_device(self.batch, self.args, stream)
            self.launches = ctx.last_launches()

    def check(self, exp, what=""):
        """After the sync: every output against `exp` = (sticky, kept, saved, summary), bit for bit; an output that was not
        asked for still holds SENTINEL; untouched inputs, guard bands."""
        got = {name: self.g[name].values() for name in OUTPUTS}
        np.testing.assert_array_equal(got["sticky"], exp[0], err_msg="sticky order %s" % what)
        for name, e in zip(OUTPUTS[1:], exp[1:]):
            if name in self.want:
                np.testing.assert_array_equal(got[name], e, err_msg="%s %s" % (name, what))
            else:
                assert (got[name] == SENTINEL).all(), "%s was not asked for %s" % (name, what)
        for name, g in self.g.items():
            g.check_guards(what) if name in OUTPUTS else g.check_unchanged(what)
        return got


def _expect_sync_error(ctx, stream, code):
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == code, ei.value


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", S.SHAPE_P)
def test_shapes(ctx, torch_dev, p):
    stream = _stream(torch_dev[0])
    w = S.shape_case(p)
    res = S.target(w)
    runs = []
    for i, kind in enumerate(("mixed", "shifted", "own")):
        prev = S.draw_prev_owner(w, res, 3, kind)
        runs.append((Run(ctx, w, res, prev, stream, shifts=("mixed", "odd", "aligned")[i]), S.expect(w, res, prev), kind))
    ctx.sync(stream)
    for r, exp, kind in runs:
        assert r.launches <= 1
        r.check(exp, "P = %d, %s" % (p, kind))
    if p >= 63:
        assert (runs[1][1][0] != res[0]).any() and runs[1][1][3][1] > runs[1][1][3][0]      # the case moves partitions at all


def test_one_run_over_a_whole_topic_of_256_and_of_4096(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    rng = np.random.default_rng(4)
    w = S.workload([(np.zeros(256, np.int64), 32), (np.full(4096, -9, np.int64), 100), (S.caught_up_lags(4096, 0.01, rng), 7)], 4)
    res = S.target(w)
    runs = [(Run(ctx, w, res, prev, stream), S.expect(w, res, prev)) for prev in
            (S.draw_prev_owner(w, res, 5), S.draw_prev_owner(w, res, 5, "shifted"))]
    ctx.sync(stream)
    for r, exp in runs:
        assert r.launches == 1
        r.check(exp, "whole-topic runs")
    assert runs[1][1][2][1] > 3000                                  # the 4096-run: nearly everything saved


def test_runs_across_the_wavefront_and_small_form_edges_and_runs_of_two(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = S.straddle_case()
    res = S.target(w)
    runs = []
    for hint in (None, 4096):                                       # 256 threads (hint 300) and the limit's request
        for kind in ("mixed", "shifted"):
            prev = S.draw_prev_owner(w, res, 1, kind)
            runs.append((Run(ctx, w, res, prev, stream, hint=hint), S.expect(w, res, prev)))
    w64 = S.workload([(S.lags_of_runs([60, 8, 180, 8]), 7), (S.lags_of_runs([2] * 128), 5)], 6)      # P = 256: the 64-thread form
    res64 = S.target(w64)
    prev64 = S.draw_prev_owner(w64, res64, 2, "shifted")
    runs.append((Run(ctx, w64, res64, prev64, stream), S.expect(w64, res64, prev64)))
    ctx.sync(stream)
    for r, exp in runs:
        r.check(exp, "straddling runs")


def test_a_member_with_more_and_with_fewer_previous_partitions_than_places(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res, prev = S.uneven_case()
    r = Run(ctx, w, res, prev, stream)
    ctx.sync(stream)
    r.check(S.expect(w, res, prev), "uneven")


def test_a_topic_over_the_limit_next_to_small_ones_and_a_topic_without_consumers(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    rng = np.random.default_rng(3)
    w = S.workload([(S.mixed_lags(50, rng), 3), (np.zeros(S.LIMIT + 1, np.int64), 2), (np.zeros(30, np.int64), 3),
                    (np.zeros(40, np.int64), 0)], 10)
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 2, "shifted")
    prev[w.part_off[3]:] = 1                                        # previous owners where nobody owns anything today
    r = Run(ctx, w, res, prev, stream)
    ctx.sync(stream)
    exp = S.expect(w, res, prev)
    assert exp[3][3] == 1 and exp[2][1] == 0 and exp[2][2] > 0 and exp[1][3] == 0
    r.check(exp, "4097 partitions: passed through and counted")


def test_empty_batches(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    none = S.workload([], 1)
    empty = S.workload([(np.empty(0, np.int64), 2)] * 3, 1)
    res = (np.empty(0, np.int32), np.empty(0, np.int32))
    a = Run(ctx, none, res, np.empty(0, np.int32), stream)
    assert a.launches == 0
    b = Run(ctx, empty, res, np.empty(0, np.int32), stream)
    assert b.launches <= 1
    ctx.sync(stream)
    a.check((np.empty(0, np.int32), np.empty(0, np.int64), np.empty(0, np.int64), np.zeros(4, np.int64)), "T = 0")
    b.check((np.empty(0, np.int32), np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(4, np.int64)), "N = 0")


def test_300_mixed_topics_in_one_call_twice(ctx, torch_dev):
    """Persistent workgroups walk several topics each at the 64-thread request; the second call, on other previous owners, finds
    nothing of the first in LDS."""
    stream = _stream(torch_dev[0])
    w = S.mixed_300()
    res = S.target(w)
    runs = []
    for seed, kind in ((1, "mixed"), (2, "shifted")):
        prev = S.draw_prev_owner(w, res, seed, kind)
        runs.append((Run(ctx, w, res, prev, stream), S.expect(w, res, prev)))
    ctx.sync(stream)
    for r, exp in runs:
        assert r.launches == 1
        r.check(exp, "300 topics")


# ---- the forms of the call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latest", [True, False])
def test_the_offsets_form_is_the_lag_form(ctx, torch_dev, latest):
    stream = _stream(torch_dev[0])
    w = S.offsets_case(latest)
    assert (w.committed < 0).any() and np.unique(w.lag).size < 8
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 7, "shifted")
    by_lag = Run(ctx, w, res, prev, stream, form="lag", latest=latest)
    by_off = Run(ctx, w, res, prev, stream, form="offsets", latest=latest)
    ctx.sync(stream)
    exp = S.expect(w, res, prev)
    by_lag.check(exp, "d_lag")
    by_off.check(exp, "offsets, latest = %s" % latest)


def test_each_optional_output_null_in_turn(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = S.shape_case(65)
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 3)
    wants = [("saved", "summary"), ("kept", "summary"), ("kept", "saved"), ()]
    runs = [Run(ctx, w, res, prev, stream, want=want) for want in wants]
    ctx.sync(stream)
    exp = S.expect(w, res, prev)
    for r, want in zip(runs, wants):
        r.check(exp, "outputs %s" % (want,))


def test_what_the_entry_refuses(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = S.shape_case(2)
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 3)
    r = Run(ctx, w, res, prev, stream, call=False)

    def refused(change, undo):
        change()
        with pytest.raises(N.LagAssignError) as ei:
            ctx.sticky_ties_device(r.batch, r.args, stream)
        assert ei.value.code == N.LA_EINVAL
        undo()

    def setter(obj, field, value):
        old = getattr(obj, field)
        return (lambda: setattr(obj, field, value)), (lambda: setattr(obj, field, old))

    refused(*setter(r.batch, "flags", N.LA_FLAG_WIRE_OUT))
    refused(*setter(r.args, "d_sticky_partition", r.batch.d_out_partition))      # not in place
    refused(*setter(r.args, "d_sticky_partition", None))
    refused(*setter(r.args, "d_prev_owner", None))
    refused(*setter(r.args, "reserved", 1))
    refused(*setter(r.args, "struct_size", ctypes.sizeof(N.StickyArgs) - 8))
    refused(*setter(r.batch, "d_lag", None))
    r.args.struct_size = 0
    ctx.sticky_ties_device(r.batch, r.args, stream)                  # and as it was built it is accepted
    ctx.sync(stream)
    r.check(S.expect(w, res, prev), "after the refusals")


# ---- hostile input: bounds the kernel checks --------------------------------------------------------------------------------------
def _hostile_workload():
    rng = np.random.default_rng(8)
    w = S.workload([(S.mixed_lags(40, rng), 4), (np.zeros(65, np.int64), 5), (np.zeros(30, np.int64), 3)], 8)
    res = S.target(w)
    return w, res, S.draw_prev_owner(w, res, 1, "shifted")


def test_an_output_id_that_is_no_input_id(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res, prev = _hostile_workload()
    out = res[0].copy()
    out[int(w.part_off[1]) + 7] = 1 << 20
    r = Run(ctx, w, (out, res[1]), prev, stream)
    _expect_sync_error(ctx, stream, N.LA_EINVAL)
    exp = sharding.sticky_ties_numpy(w.part_off, w.partition_id, w.lag, out, res[1], prev, strict=False)
    assert exp[3][3] == 1 and (exp[0][105:] != out[105:]).any()
    r.check(exp, "a foreign output id: its topic passed through, the others re-matched")


def test_a_duplicated_input_id(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res, prev = _hostile_workload()
    ids = w.partition_id.copy()
    ids[int(w.part_off[1]) + 3] = ids[int(w.part_off[1]) + 2]
    r = Run(ctx, w, res, prev, stream, override={"partition_id": ids})
    _expect_sync_error(ctx, stream, N.LA_EINVAL)
    exp = sharding.sticky_ties_numpy(w.part_off, ids, w.lag, res[0], res[1], prev, strict=False)
    assert exp[3][3] == 1
    r.check(exp, "a duplicated input id: its topic passed through")
    ok = Run(ctx, w, res, prev, stream)                              # the next call on the context is an ordinary one
    ctx.sync(stream)
    ok.check(S.expect(w, res, prev), "after the error")


def test_a_topic_over_its_hint_is_a_shape_error_and_passed_through(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res, prev = _hostile_workload()
    r = Run(ctx, w, res, prev, stream, hint=64)
    _expect_sync_error(ctx, stream, N.LA_ESHAPE)
    exp = S.expect(w, res, prev, max_partitions=64)
    assert exp[3][3] == 1
    r.check(exp, "hint 64, a topic of 65")
    for hint in (0, -5, 1 << 40):                                   # no usable hint: the limit's request
        r = Run(ctx, w, res, prev, stream, hint=hint)
        ctx.sync(stream)
        r.check(S.expect(w, res, prev), "hint %d" % hint)


def test_offsets_that_leave_the_arrays_are_a_shape_error_and_nothing_is_written(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res, prev = _hostile_workload()
    po = w.part_off.copy()
    po[2] = w.n_partitions + (1 << 40)                               # topic 1 ends far outside, topic 2 starts there
    r = Run(ctx, w, res, prev, stream, override={"part_off": po})
    _expect_sync_error(ctx, stream, N.LA_ESHAPE)
    good = S.expect(w, res, prev)
    sticky = np.full(w.n_partitions, SENTINEL, np.int32)
    sticky[:40] = good[0][:40]
    kept, saved = np.full(3, SENTINEL, np.int64), np.full(3, SENTINEL, np.int64)
    kept[0], saved[0] = good[1][0], good[2][0]
    before0 = int(((prev[:40] >= 0) & (prev[:40] == res[1][:40])).sum())
    r.check((sticky, kept, saved, np.array([before0, good[1][0], 1 if (good[0][:40] != res[0][:40]).any() else 0, 0], np.int64)),
            "offsets outside [0, N]")


# ---- with the calls around it --------------------------------------------------------------------------------------------------
def test_assign_adjust_sticky_round_on_one_stream(ctx, torch_dev):
    """assign, la_cooperative_adjust_device (for d_prev_owner), sticky, la_cooperative_round_device on the sticky order: no sync
    in between.  The round's withheld count is the numpy pipeline's, and at most what it is without the sticky step; the sticky
    order verifies as 0 or LA_VERDICT_ORDER, and the member loads are those of the reference's order."""
    torch = torch_dev[0]
    stream = _stream(torch)
    w, res, _, first = S.caught_up(8, 256, 32, 0.05, 41)
    n, t, k = w.n_partitions, w.n_topics, w.cons_rank.size
    m = int(w.cons_rank.max()) + 1
    owned_off, owned_topic, owned_pid = sharding.group_by_member_numpy(w.part_off, first[0], first[1], m)
    g = {name: Guarded("device", a.size, a.dtype, i % 3, a, name=name) for i, (name, a) in enumerate(
        (("part_off", w.part_off), ("partition_id", w.partition_id), ("lag", w.lag), ("cons_off", w.cons_off), ("cons_rank", w.cons_rank),
         ("owned_off", owned_off), ("owned_topic", owned_topic), ("owned_pid", owned_pid)))}
    for i, (name, size, dtype) in enumerate((("out_pid", n, np.int32), ("out_rank", n, np.int32), ("out_total", k, np.int64),
                                             ("prev", n, np.int32), ("adjust_summary", 6, np.int64), ("sticky", n, np.int32),
                                             ("kept", t, np.int64), ("saved", t, np.int64), ("summary", 4, np.int64),
                                             ("round_summary", 6, np.int64), ("member_off", m + 1, np.int64), ("g_topic", n, np.int32),
                                             ("g_pid", n, np.int32), ("verdict", t, np.int32), ("v_summary", 4, np.int64),
                                             ("m_parts", m, np.int64), ("m_lag", m, np.int64), ("unassigned", 1, np.int64))):
        g[name] = Guarded("device", size, dtype, (i + 1) % 3, name=name)
    torch.cuda.synchronize()
    p = lambda name: g[name].ptr
    b = N.DeviceBatch()
    b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
    b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = n, k, w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id, b.d_lag, b.d_cons_off, b.d_cons_rank = p("part_off"), p("partition_id"), p("lag"), p("cons_off"), p("cons_rank")
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = p("out_pid"), p("out_rank"), p("out_total")

    def coop(out_partition, summary):
        a = N.CoopArgs()
        a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, m, owned_pid.size
        a.d_part_off, a.d_out_partition, a.d_out_member_rank = p("part_off"), p(out_partition), p("out_rank")
        a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = p("owned_off"), p("owned_topic"), p("owned_pid")
        a.d_summary = p(summary)
        return a

    ctx.assign_batch_device(b, stream)
    adjust = coop("out_pid", "adjust_summary")
    adjust.d_prev_owner = p("prev")
    ctx.cooperative_adjust_device(adjust, stream)
    s = N.StickyArgs()
    s.d_prev_owner, s.d_sticky_partition, s.d_topic_kept, s.d_topic_saved, s.d_summary = p("prev"), p("sticky"), p("kept"), p("saved"), p("summary")
    ctx.sticky_ties_device(b, s, stream)
    rnd = N.CoopRoundArgs()
    rnd.adjust = coop("sticky", "round_summary")
    rnd.member_off, rnd.grouped_topic, rnd.grouped_partition = p("member_off"), p("g_topic"), p("g_pid")
    ctx.cooperative_round_device(rnd, stream)
    vb = N.DeviceBatch.from_buffer_copy(b)
    vb.d_out_partition = p("sticky")
    ctx.verify_assignment_device(vb, p("verdict"), p("v_summary"), stream)
    ctx.member_loads_device(n, p("out_rank"), k, p("cons_rank"), p("out_total"), m, p("m_parts"), p("m_lag"), p("unassigned"), stream)
    ctx.sync(stream)

    got = {name: x.values() for name, x in g.items()}
    for name, e in zip(("out_pid", "out_rank", "out_total"), res):
        np.testing.assert_array_equal(got[name], e, err_msg=name)
    plain = sharding.cooperative_round_numpy(w.part_off, res[0], res[1], m, owned_off, owned_topic, owned_pid)
    np.testing.assert_array_equal(got["prev"], plain[0])
    np.testing.assert_array_equal(got["adjust_summary"], plain[7])
    exp = S.expect(w, res, plain[0])
    for name, e in zip(OUTPUTS, exp):
        np.testing.assert_array_equal(got[name], e, err_msg=name)
    sticky_round = sharding.cooperative_round_numpy(w.part_off, exp[0], res[1], m, owned_off, owned_topic, owned_pid)
    np.testing.assert_array_equal(got["round_summary"], sticky_round[7])
    for name, e in zip(("member_off", "g_topic", "g_pid"), sticky_round[8:]):
        np.testing.assert_array_equal(got[name], e, err_msg=name)
    assert got["round_summary"][2] == sticky_round[7][2] <= plain[7][2]
    assert got["round_summary"][0] == exp[3][1] and plain[7][0] == exp[3][0]      # the round keeps what the sticky call said
    assert exp[3][1] > exp[3][0]                                    # the case has something to save
    v_exp, v_sum = sharding.verify_assignment_numpy(w.part_off, w.partition_id, w.cons_off, w.cons_rank, exp[0], res[1], res[2], lag=w.lag)
    np.testing.assert_array_equal(got["verdict"], v_exp)
    assert set(got["verdict"].tolist()) <= {0, N.LA_VERDICT_ORDER} and N.LA_VERDICT_ORDER in got["verdict"]
    np.testing.assert_array_equal(got["v_summary"], v_sum)
    parts, lag, unassigned = sharding.member_loads_numpy(res[1], w.cons_rank, res[2], m)
    np.testing.assert_array_equal(got["m_parts"], parts)
    np.testing.assert_array_equal(got["m_lag"], lag)
    assert int(got["unassigned"][0]) == unassigned
    for name in ("part_off", "partition_id", "lag", "cons_off", "cons_rank", "owned_off", "owned_topic", "owned_pid"):
        g[name].check_unchanged(name)
    for name, x in g.items():
        x.check_guards(name)
