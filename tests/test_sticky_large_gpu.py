"""la_sticky_ties_device with LA_FLAG_STICKY_LARGE on the GPU, through the C ABI: topics of more than 4096 partitions are
re-matched by the global form (csrc/la_sticky_large.hip).  The yardstick is sharding.sticky_ties_numpy without a limit, which
tests/test_sticky_large_cpu.py holds to the independent model at the same cases (sticky_large_cases.py): every output here equals
it bit for bit.  Every array of a call is a guarded device buffer at an element shift; outputs hold SENTINEL before the call,
inputs must come back byte for byte, guard bands included.  Behind them the flag through la_cooperative_round_sticky_device,
LA_COOP_STICKY_LARGE through la_assign_batch_cooperative_sticky, and the host mirror's lag.assignor.sticky.ties.large."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

import coop_sticky_cases as K
import sticky_cases as S
import sticky_large_cases as SL
from gpu_helpers import SENTINEL, Guarded, shifts_for

pytestmark = pytest.mark.gpu

FLAG = N.LA_FLAG_STICKY_LARGE
OUTPUTS = ("sticky", "kept", "saved", "summary")
NAMES = ("part_off", "partition_id", "lag", "begin", "end", "committed", "out_pid", "out_rank", "prev") + OUTPUTS
MAX_LAUNCHES = 1 + N.STICKY_GLOBAL_LAUNCHES
_i64p = ctypes.POINTER(ctypes.c_int64)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Run:
    """One sticky call on guarded device buffers.  flags: the batch's (FLAG or 0); h_po: the host offsets handed over with the
    flag (default: the workload's; False: none).  form: "lag" (d_lag) or "offsets"; want: the optional outputs that are not NULL;
    override: arrays that replace the workload's on the device (hostile input)."""

    def __init__(self, ctx, w, res, prev, stream, flags=FLAG, h_po=None, form="lag", latest=True, shifts="mixed",
                 want=("kept", "saved", "summary"), hint=None, override=None, call=True):
        sh = shifts_for(shifts, NAMES)
        self.w, self.want = w, want
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
        b.n_topics, b.reset_mode, b.algo, b.flags = t, (N.LA_RESET_LATEST if latest else N.LA_RESET_EARLIEST), N.LA_ALGO_AUTO, flags
        b.n_partitions, b.n_consumers = n, 0
        b.max_partitions_per_topic, b.max_consumers_per_topic = (w.max_partitions if hint is None else hint), 0
        ptr = lambda name: self.g[name].ptr if name in self.g else None
        b.d_part_off, b.d_partition_id = ptr("part_off"), ptr("partition_id")
        b.d_begin_off, b.d_end_off, b.d_committed_off, b.d_lag = ptr("begin"), ptr("end"), ptr("committed"), ptr("lag")
        b.d_out_partition, b.d_out_member_rank = ptr("out_pid"), ptr("out_rank")
        self.h_po = None if h_po is False else np.ascontiguousarray(w.part_off if h_po is None else h_po, np.int64).copy()
        self.h_po_before = None if self.h_po is None else self.h_po.copy()
        if self.h_po is not None:
            b.h_part_off = self.h_po.ctypes.data_as(_i64p)
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

    def check_contract(self, what=""):
        for name, g in self.g.items():
            g.check_guards(what) if name in OUTPUTS else g.check_unchanged(what)
        if self.h_po is not None:
            np.testing.assert_array_equal(self.h_po, self.h_po_before, err_msg="the host offsets %s" % what)

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
        self.check_contract(what)
        return got


def _expect_sync_error(ctx, stream, code):
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == code, ei.value


# ---- fails without the feature ---------------------------------------------------------------------------------------------------
def test_a_topic_of_4097_is_re_matched_not_passed_through(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    name = "shape %d" % SL.SHAPE_P[0]
    w, res = SL.case(name)
    prev = SL.prev_of(name, "shifted")
    r = Run(ctx, w, res, prev, stream)
    ctx.sync(stream)
    exp = SL.expected(name, "shifted")
    got = r.check(exp, "4097, flagged")
    assert got["summary"][3] == 0 and (got["sticky"] != res[0]).any() and got["saved"][0] > 0
    assert 1 < r.launches <= MAX_LAUNCHES


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", SL.SHAPE_P)
def test_shapes(ctx, torch_dev, p):
    stream = _stream(torch_dev[0])
    name = "shape %d" % p
    w, res = SL.case(name)
    runs = []
    for i, kind in enumerate(SL.KINDS):
        prev = SL.prev_of(name, kind)
        runs.append((Run(ctx, w, res, prev, stream, shifts=("mixed", "odd", "aligned")[i]), SL.expected(name, kind), kind,
                     Run(ctx, w, res, prev, stream, flags=0, h_po=False), S.expect(w, res, prev)))
    ctx.sync(stream)
    for r, exp, kind, plain, plain_exp in runs:
        assert r.launches <= MAX_LAUNCHES and plain.launches == 1
        r.check(exp, "P = %d, %s" % (p, kind))
        plain.check(plain_exp, "P = %d, %s, unflagged" % (p, kind))
        assert plain_exp[3][3] == 1 and exp[3][3] == 0
    assert runs[1][1][3][1] > runs[1][1][3][0]                      # the shifted owners: the case saves something


@pytest.mark.parametrize("name,kind", [("neighbours", "shifted"), ("neighbours", "mixed"), ("one run", "mixed"), ("one run", "shifted"),
                                       ("no ties", "shifted"), ("extremes", "mixed"), ("extremes", "shifted"),
                                       ("caught up", "shifted"), ("straddle", "skewed"), ("straddle", "mixed"), ("two large", "mixed")])
def test_runs_and_lags(ctx, torch_dev, name, kind):
    """Two adjacent large topics that are all lag 0 (two runs, not one) | one run over 12 289 | no ties at all | runs at
    INT64_MIN / INT64_MAX and negative lags | caught up at 1 % | runs and groups across the sort's tile edges, |S| > |W| and
    |W| > |S|, leftovers in several runs."""
    stream = _stream(torch_dev[0])
    w, res = SL.case(name)
    prev = SL.prev_of(name, kind)
    r = Run(ctx, w, res, prev, stream)
    plain = Run(ctx, w, res, prev, stream, flags=0, h_po=False, shifts="odd")
    ctx.sync(stream)
    exp = SL.expected(name, kind)
    got = r.check(exp, "%s, %s" % (name, kind))
    plain.check(S.expect(w, res, prev), "%s, %s, unflagged" % (name, kind))
    assert r.launches <= MAX_LAUNCHES and got["summary"][3] == 0
    if name == "no ties":
        np.testing.assert_array_equal(got["sticky"], res[0])
        assert got["summary"][2] == 0
    if name == "neighbours" and kind == "shifted":
        assert (got["saved"] > 0).all()


def test_large_topics_between_small_ones_an_empty_one_and_one_of_exactly_4096(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res = SL.case("mixed batch")
    runs = []
    for kind in ("mixed", "shifted"):
        prev = SL.prev_of("mixed batch", kind)
        runs.append((Run(ctx, w, res, prev, stream), SL.expected("mixed batch", kind), Run(ctx, w, res, prev, stream, flags=0, h_po=False),
                     S.expect(w, res, prev)))
    ctx.sync(stream)
    a, z = int(w.part_off[3]), int(w.part_off[4])
    assert z - a == SL.LIMIT
    for r, exp, plain, plain_exp in runs:
        got = r.check(exp, "mixed batch")
        unflagged = plain.check(plain_exp, "mixed batch, unflagged")
        assert plain_exp[3][3] == 3 and exp[3][3] == 0
        np.testing.assert_array_equal(got["sticky"][a:z], unflagged["sticky"][a:z])      # the 4096 topic: the LDS kernel's either way
        assert (got["kept"][3], got["saved"][3]) == (unflagged["kept"][3], unflagged["saved"][3])
    # the hint: whatever it says, the large topics are re-matched; a small topic over it is still a shape error
    r = Run(ctx, w, res, SL.prev_of("mixed batch"), stream, hint=0)
    ctx.sync(stream)
    r.check(SL.expected("mixed batch"), "hint 0")


def test_the_lag_from_offsets_on_a_large_topic(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = SL.offsets_case(latest=False)
    assert (w.committed < 0).any() and np.unique(w.lag).size < 12 and SL.big_topics(w) == [1]
    res = S.target(w)
    prev = S.draw_prev_owner(w, res, 7, "shifted")
    by_lag = Run(ctx, w, res, prev, stream, form="lag", latest=False)
    by_off = Run(ctx, w, res, prev, stream, form="offsets", latest=False)
    ctx.sync(stream)
    exp = SL.expect(w, res, prev)
    assert exp[3][3] == 0 and exp[2][1] > 0
    by_lag.check(exp, "d_lag")
    by_off.check(exp, "offsets, EARLIEST")


def test_each_optional_output_null_in_turn(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res = SL.case("two large")
    prev = SL.prev_of("two large")
    wants = [("saved", "summary"), ("kept", "summary"), ("kept", "saved"), ()]
    runs = [Run(ctx, w, res, prev, stream, want=want) for want in wants]
    ctx.sync(stream)
    for r, want in zip(runs, wants):
        r.check(SL.expected("two large"), "outputs %s" % (want,))


# ---- launches ------------------------------------------------------------------------------------------------------------------------
def test_the_launch_count_does_not_depend_on_the_number_of_large_topics(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    runs = []
    for name in ("one large", "three large"):
        w, res = SL.case(name)
        runs.append((Run(ctx, w, res, SL.prev_of(name), stream), SL.expected(name), name))
    ctx.sync(stream)
    for r, exp, name in runs:
        r.check(exp, name)
        assert 1 < r.launches <= MAX_LAUNCHES
    assert runs[0][0].launches == runs[1][0].launches


def test_a_flagged_call_without_a_large_topic_is_the_unflagged_call(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res = SL.case("small only")
    prev = SL.prev_of("small only", "shifted")
    flagged = Run(ctx, w, res, prev, stream)
    plain = Run(ctx, w, res, prev, stream, flags=0, h_po=False)
    ctx.sync(stream)
    exp = S.expect(w, res, prev)
    flagged.check(exp, "flagged, no large topic")
    plain.check(exp, "unflagged")
    assert flagged.launches == plain.launches == 1


# ---- what the entry refuses --------------------------------------------------------------------------------------------------------
def test_the_flag_without_usable_host_offsets_is_einval_at_the_call(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w, res = SL.case("two large")
    prev = SL.prev_of("two large")
    descending = w.part_off.copy()
    descending[1], descending[2] = descending[2], descending[1]
    outside = w.part_off.copy()
    outside[-1] += 1
    for h_po in (False, descending, outside):
        r = Run(ctx, w, res, prev, stream, h_po=h_po, call=False)
        with pytest.raises(N.LagAssignError) as ei:
            ctx.sticky_ties_device(r.batch, r.args, stream)
        assert ei.value.code == N.LA_EINVAL
        ctx.sync(stream)
        for name in OUTPUTS:
            assert (r.g[name].values() == SENTINEL).all(), "%s was written by a refused call" % name
    ok = Run(ctx, w, res, prev, stream, flags=0, h_po=descending)     # without the flag nobody looks at them
    ctx.sync(stream)
    ok.check(S.expect(w, res, prev), "unflagged, descending host offsets")


# ---- hostile input -------------------------------------------------------------------------------------------------------------------
def _passed_through(w, res, prev, bad_topic, ids=None):
    """The unlimited yardstick with `bad_topic` passed through exactly and counted."""
    exp = sharding.sticky_ties_numpy(w.part_off, w.partition_id if ids is None else ids, w.lag, res[0], res[1], prev,
                                     max_partitions=SL.ANY, strict=False)
    a, z = int(w.part_off[bad_topic]), int(w.part_off[bad_topic + 1])
    np.testing.assert_array_equal(exp[0][a:z], res[0][a:z])
    assert exp[3][3] == 1 and exp[2][bad_topic] == 0
    return exp


@pytest.mark.parametrize("what", ["duplicate input id", "foreign output id", "repeated output id"])
def test_a_bad_large_topic_is_passed_through_and_the_other_is_exact(ctx, torch_dev, what):
    stream = _stream(torch_dev[0])
    w, res = SL.case("two large")
    prev = SL.prev_of("two large", "shifted")
    a = int(w.part_off[2])
    ids, out = w.partition_id.copy(), res[0].copy()
    if what == "duplicate input id":
        ids[a + 4100] = ids[a + 7]
    elif what == "foreign output id":
        out[a + 4100] = 1 << 20
    else:
        out[a + 4100] = out[a + 7]
    r = Run(ctx, w, (out, res[1]), prev, stream, override={"partition_id": ids})
    _expect_sync_error(ctx, stream, N.LA_EINVAL)
    exp = _passed_through(w, (out, res[1]), prev, 2, ids)
    assert exp[2][0] > 0
    r.check(exp, what)
    ok = Run(ctx, w, res, prev, stream)                              # the next call on the context is an ordinary one
    ctx.sync(stream)
    ok.check(SL.expected("two large", "shifted"), "after the error")


@pytest.mark.parametrize("what", ["boundary later", "boundary earlier", "large on the device only"])
def test_device_offsets_that_differ_from_the_hosts_are_a_shape_error(ctx, torch_dev, what):
    """(The shifted boundary lies between two large topics: a small topic cut differently would hold foreign ids as well, and
    la_sync reports LA_EINVAL before LA_ESHAPE.)"""
    stream = _stream(torch_dev[0])
    name = "two large" if what == "large on the device only" else "neighbours"
    w, res = SL.case(name)
    prev = SL.prev_of(name)
    po, h_po = w.part_off.copy(), w.part_off.copy()
    if what == "boundary later":
        po[1] += 5                                                   # the first topic ends, the second starts, later on the device
    elif what == "boundary earlier":
        po[1] -= 3
    else:
        h_po[1] = SL.LIMIT                                           # by the host's offsets topic 0 is within the limit
    r = Run(ctx, w, res, prev, stream, h_po=h_po, override={"part_off": po})
    _expect_sync_error(ctx, stream, N.LA_ESHAPE)
    r.check_contract(what)
    ok = Run(ctx, w, res, prev, stream)                              # the next call on the context is an ordinary one
    ctx.sync(stream)
    ok.check(SL.expected(name), "after the error")


# ---- the chain and the host call -----------------------------------------------------------------------------------------------------
def test_the_flag_reaches_the_sticky_step_of_the_cooperative_round(ctx, torch_dev):
    import test_coop_sticky_gpu as TC
    stream = _stream(torch_dev[0])
    k = K.drawn(61, [SL.LIMIT + 1, 40], 5, K.caught_up)
    c = k.coop
    h_po = np.ascontiguousarray(c.part_off, np.int64).copy()

    def flag(r):
        r.batch.flags = FLAG
        r.batch.h_part_off = h_po.ctypes.data_as(_i64p)

    flagged = TC.Call(ctx, k, stream, edit=flag)
    plain = TC.Call(ctx, k, stream)
    ctx.sync(stream)
    args = (c.part_off, k.partition_id, k.lag, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
    exp = sharding.cooperative_round_sticky_numpy(*args, max_partitions=sharding.STICKY_ANY_SIZE)
    assert exp[3][3] == 0 and exp[2][0] > 0
    flagged.check(exp, "flagged chain")
    plain.check(k.expect(), "unflagged chain")
    assert flagged.launches > plain.launches

    def no_offsets(r):
        r.batch.flags = FLAG

    with pytest.raises(N.LagAssignError) as ei:
        TC.Call(ctx, k, stream, edit=no_offsets)
    assert ei.value.code == N.LA_EINVAL
    ctx.sync(stream)


def test_the_host_call_with_large(ctx, torch_dev):
    h = K.HostCase(71, [SL.LIMIT + 1, 30, 5000], 6)
    call = lambda **kw: ctx.assign_batch_cooperative_sticky(h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, *h.owned, **kw, **h.inputs("sparse"))
    got = call(large=True)
    exp = sharding.assign_cooperative_sticky_numpy(h.part_off, h.pid, h.lag_of("sparse"), h.cons_off, h.cons_rank, h.m, *h.owned,
                                                   assign=oracle.assign_flat, max_partitions=sharding.STICKY_ANY_SIZE)
    import test_coop_sticky_gpu as TC
    TC.host_same(got, exp, "large")
    assert got.sticky_summary[3] == 0 and got.topic_saved[0] > 0
    plain = call()
    TC.host_same(plain, h.expect("sparse"), "without large")
    assert plain.sticky_summary[3] == 2 and got.coop.summary[2] < plain.coop.summary[2], "the large topics withhold less re-matched"
    # every other call keeps rejecting the bit
    a = N.AssignCoopArgs()
    a.struct_size, a.flags = ctypes.sizeof(N.AssignCoopArgs), N.LA_COOP_STICKY_LARGE
    assert N.load().la_assign_batch_cooperative(ctx._h, ctypes.byref(a)) == N.LA_EINVAL


def test_the_mirror_with_both_keys_on_passes_no_topic_through():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    import test_coop_sticky_gpu as TC
    metadata = {"events": list(range(5000)), "small": list(range(9))}
    tps = [(t, p) for t, ps in metadata.items() for p in ps]

    def source(lagging):
        lag = {tp: (1000 + 7 * i if tp in lagging else 0) for i, tp in enumerate(tps)}
        return TC.Offsets({tp: 0 for tp in tps}, {tp: 500 + lag[tp] for tp in tps}, {tp: 500 for tp in tps})

    subs = {"app-1": ["events", "small"], "app-2": ["events", "small"], "app-3": ["events"]}
    conf = {"group.id": "g", "auto.offset.reset": "earliest", "lag.assignor.sticky.ties": "true"}
    sticky, large, only_large = LagBasedPartitionAssignor(), LagBasedPartitionAssignor(), LagBasedPartitionAssignor()
    sticky.configure(conf)
    large.configure(dict(conf, **{"lag.assignor.sticky.ties.large": "true"}))
    only_large.configure({"group.id": "g", "auto.offset.reset": "earliest", "lag.assignor.sticky.ties.large": "true"})
    before, now = source({("events", 3), ("events", 4000), ("small", 1)}), source({("events", 17), ("events", 2500), ("small", 6)})
    owned = {m: [tuple(tp) for tp in x] for m, x in sticky.assign(metadata, subs, before).items()}
    sticky.assign_cooperative(metadata, subs, owned, now)
    c_sticky = sticky.last_cooperative_round()
    large.assign_cooperative(metadata, subs, owned, now)
    c_large = large.last_cooperative_round()
    only_large.assign_cooperative(metadata, subs, owned, now)
    c_only = only_large.last_cooperative_round()
    assert c_sticky["sticky_topics_passed_through"] == 1 and c_large["sticky_topics_passed_through"] == 0
    assert c_large["sticky_kept_after"] > c_sticky["sticky_kept_after"] and c_large["withheld"] < c_sticky["withheld"]
    assert c_large["sticky_kept_before"] == c_sticky["sticky_kept_before"]
    assert (c_only["sticky_kept_before"], c_only["sticky_kept_after"], c_only["sticky_topics_passed_through"]) == (0, 0, 0)
