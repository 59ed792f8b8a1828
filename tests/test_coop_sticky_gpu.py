"""la_cooperative_round_sticky_device on the GPU, through the C ABI.  The yardstick is sharding.cooperative_round_sticky_numpy,
which tests/test_coop_sticky_cpu.py holds to a dictionary model at the same cases (coop_sticky_cases.py).  Every case runs three
times on the same inputs -- as it comes, with LA_COOP_FORCE_TABLE, and as the chain of the three EXISTING device calls the new
call is defined by -- and all three must equal the yardstick bit for bit on every output.  Every array of a call is a guarded
device buffer at an element shift of its own; outputs hold SENTINEL before the call, inputs must come back byte for byte.
Behind them la_assign_batch_cooperative_sticky on host arrays (against sharding.assign_cooperative_sticky_numpy over the reference
oracle's assign_flat) and the host mirror with lag.assignor.sticky.ties on and off."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N

import coop_cases as C
import coop_sticky_cases as K
from gpu_helpers import SENTINEL, Guarded, shifts_for

pytestmark = pytest.mark.gpu

INPUTS = ("part_off", "partition_id", "lag", "begin", "end", "committed", "pid", "rank", "owned_off", "owned_topic", "owned_pid")
FIELD = {"prev_owner": "d_prev_owner", "coop_rank": "d_coop_member_rank", "kept": "d_member_kept", "fresh": "d_member_fresh",
         "pending": "d_member_pending", "release": "d_member_release", "topic_withheld": "d_topic_withheld", "summary": "d_summary"}
REQUIRED = ("sticky", "member_off", "grouped_partition")
OPTIONAL = tuple(k for k in K.ALL if k not in REQUIRED)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def sizes_of(c):
    return {"sticky": c.n, "topic_kept": c.t, "topic_saved": c.t, "sticky_summary": 4, "prev_owner": c.n, "coop_rank": c.n, "kept": c.m,
            "fresh": c.m, "pending": c.m, "release": c.m, "topic_withheld": c.t, "summary": 6, "member_off": c.m + 1,
            "grouped_topic": c.n, "grouped_partition": c.n}


def dtype_of(name):
    return np.int32 if name in ("sticky", "prev_owner", "coop_rank", "grouped_topic", "grouped_partition") else np.int64


class Call:
    """One sticky round on guarded device buffers.  how: "call" (la_cooperative_round_sticky_device) or "chain" (the three
    existing device calls, the previous owners of the target in a buffer of the test's own).  form: "lag" (d_lag) or "offsets"."""

    def __init__(self, ctx, k, stream, flags=0, how="call", want=K.ALL, shifts="mixed", form=None, null_owned=False, edit=None):
        c = k.coop
        self.k, self.want = k, tuple(want) + tuple(x for x in REQUIRED if x not in want)
        sh = shifts_for(shifts, INPUTS + K.ALL + ("tmp_prev",))
        form = form or ("offsets" if k.offsets is not None else "lag")
        arrays = {"part_off": c.part_off, "partition_id": k.partition_id, "pid": c.pid, "rank": c.rank}
        if form == "lag":
            arrays["lag"] = k.lag
        else:
            arrays["begin"], arrays["end"], arrays["committed"] = k.offsets
        if not null_owned:
            arrays.update(owned_off=c.owned_off, owned_topic=c.owned_topic, owned_pid=c.owned_pid)
        self.g = {name: Guarded("device", a.size, a.dtype, sh[name], a, name=name) for name, a in arrays.items()}
        self.inputs = tuple(arrays)
        sz = sizes_of(c)
        for name in K.ALL:
            self.g[name] = Guarded("device", sz[name], dtype_of(name), sh[name], name=name)
        ptr = lambda name: self.g[name].ptr if name in self.g else None
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = c.t, (N.LA_RESET_LATEST if k.latest else N.LA_RESET_EARLIEST), N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = c.n, 0, k.hint, 0
        b.d_part_off, b.d_partition_id = ptr("part_off"), ptr("partition_id")
        b.d_begin_off, b.d_end_off, b.d_committed_off, b.d_lag = ptr("begin"), ptr("end"), ptr("committed"), ptr("lag")
        b.d_out_partition, b.d_out_member_rank = ptr("pid"), ptr("rank")
        self.batch = b
        want_ptr = lambda name: ptr(name) if name in self.want else None
        a = N.CoopStickyArgs()
        a.flags = flags
        r = a.round
        adj = r.adjust
        adj.n_members, adj.n_owned = c.m, (0 if null_owned else c.n_owned)
        adj.d_owned_member_off, adj.d_owned_topic, adj.d_owned_partition = ptr("owned_off"), ptr("owned_topic"), ptr("owned_pid")
        for name, field in FIELD.items():
            setattr(adj, field, want_ptr(name))
        r.member_off, r.grouped_topic, r.grouped_partition = ptr("member_off"), want_ptr("grouped_topic"), ptr("grouped_partition")
        a.d_sticky_partition, a.d_topic_kept, a.d_topic_saved = ptr("sticky"), want_ptr("topic_kept"), want_ptr("topic_saved")
        a.d_sticky_summary = want_ptr("sticky_summary")
        self.args = a
        if edit:
            edit(self)
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        if how == "call":
            ctx.cooperative_round_sticky_device(self.batch, self.args, stream)
            self.launches = ctx.last_launches()
            return
        assert how == "chain", how
        self.g["tmp_prev"] = Guarded("device", c.n, np.int32, sh["tmp_prev"], name="tmp_prev")
        first = N.CoopArgs()
        first.n_topics, first.n_partitions, first.n_members, first.n_owned = c.t, c.n, c.m, adj.n_owned
        first.d_part_off, first.d_out_partition, first.d_out_member_rank = ptr("part_off"), ptr("pid"), ptr("rank")
        first.d_owned_member_off, first.d_owned_topic, first.d_owned_partition = ptr("owned_off"), ptr("owned_topic"), ptr("owned_pid")
        first.d_prev_owner = ptr("tmp_prev")
        ctx.cooperative_adjust_device(first, stream)
        self.launches = ctx.last_launches()
        s = N.StickyArgs()
        s.d_prev_owner, s.d_sticky_partition = ptr("tmp_prev"), ptr("sticky")
        s.d_topic_kept, s.d_topic_saved, s.d_summary = a.d_topic_kept, a.d_topic_saved, a.d_sticky_summary
        ctx.sticky_ties_device(self.batch, s, stream)
        self.launches += ctx.last_launches()
        third = N.CoopRoundArgs()
        third.flags = flags
        ctypes.memmove(ctypes.byref(third.adjust), ctypes.byref(adj), ctypes.sizeof(N.CoopArgs))
        t = third.adjust
        t.n_topics, t.n_partitions = c.t, c.n
        t.d_part_off, t.d_out_partition, t.d_out_member_rank = ptr("part_off"), ptr("sticky"), ptr("rank")
        third.member_off, third.grouped_topic, third.grouped_partition = r.member_off, r.grouped_topic, r.grouped_partition
        ctx.cooperative_round_device(third, stream)
        self.launches += ctx.last_launches()

    def outputs(self):
        return [self.g[name].values() for name in K.ALL]

    def check_contract(self, what=""):
        for name in self.inputs:
            self.g[name].check_unchanged(what)
        for name in K.ALL:
            self.g[name].check_guards(what)

    def check(self, exp, what=""):
        """Wanted outputs equal the yardstick, the others still hold SENTINEL, nothing outside the arrays was written, the
        inputs are byte for byte what they were."""
        for name, g, e in zip(K.ALL, self.outputs(), exp):
            if name in self.want:
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))
            else:
                assert (np.asarray(g) == SENTINEL).all(), "%s was not asked for %s" % (name, what)
        self.check_contract(what)


def three(ctx, torch, k, what="", **kw):
    """The case as it comes, with LA_COOP_FORCE_TABLE and as the chain of the existing calls: all equal the yardstick."""
    stream = _stream(torch)
    exp = k.expect()
    plain = Call(ctx, k, stream, 0, **kw)
    forced = Call(ctx, k, stream, N.LA_COOP_FORCE_TABLE, **kw)
    chain = Call(ctx, k, stream, 0, how="chain", **kw)
    ctx.sync(stream)
    plain.check(exp, what + " (as it comes)")
    forced.check(exp, what + " (table forced)")
    chain.check(exp, what + " (the chain of the three calls)")
    assert (plain.launches == 1) == k.small, "one launch exactly within the limits %s: %d" % (what, plain.launches)
    if not k.small:
        assert plain.launches == forced.launches == chain.launches > 1, "the general form is the chain %s" % what
    else:
        assert forced.launches > 1
    return exp, plain, forced, chain


def _expect_sync_error(ctx, stream, code):
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == code, ei.value


# ---- every case of the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CLEAN)
def test_case(ctx, torch_dev, name):
    k = K.case(name)
    exp, plain, forced, _ = three(ctx, torch_dev[0], k, name)
    if name == "topic of 4097":
        assert forced.launches > 3 and exp[3][3] == 1


def test_nothing_owned_with_null_owned_pointers(ctx, torch_dev):
    k = K.case("nothing owned")
    exp, plain, _, _ = three(ctx, torch_dev[0], k, "NULL owned pointers", null_owned=True)
    np.testing.assert_array_equal(plain.outputs()[0], k.coop.pid)    # sticky equals the target


def test_a_topic_over_the_hint_is_la_eshape_and_passed_through(ctx, torch_dev):
    """The kernel of the one-workgroup form finds the topic itself (the host does not know the topics' sizes of a device call):
    one launch, LA_ESHAPE from la_sync, the topic passed through exactly as la_sticky_ties_device passes it."""
    k = K.case("topic over the hint")
    stream = _stream(torch_dev[0])
    exp = k.expect()
    for flags, how in ((0, "call"), (N.LA_COOP_FORCE_TABLE, "call"), (0, "chain")):
        r = Call(ctx, k, stream, flags, how=how)
        _expect_sync_error(ctx, stream, N.LA_ESHAPE)
        r.check(exp, "over the hint, flags %d, %s" % (flags, how))
        if how == "call":
            assert (r.launches == 1) == (flags == 0)
    three(ctx, torch_dev[0], K.case("one partition"), "the next clean call")


@pytest.mark.parametrize("form", ["lag", "offsets"])
def test_the_offsets_form_is_the_lag_form(ctx, torch_dev, form):
    for name in ("offsets, latest", "offsets, earliest"):
        three(ctx, torch_dev[0], K.case(name), "%s by %s" % (name, form), form=form)


# ---- optional outputs ----------------------------------------------------------------------------------------------------------------
def test_every_optional_output_may_be_null_alone_and_all_at_once(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    k = K.case("stale, unmapped, head and tail claims")
    exp = k.expect()
    wants = [()] + [tuple(x for x in OPTIONAL if x != name) for name in OPTIONAL]
    runs = [(w, f, Call(ctx, k, stream, f, want=w)) for w in wants for f in (0, N.LA_COOP_FORCE_TABLE)]
    ctx.sync(stream)
    for w, f, r in runs:
        assert (r.launches == 1) == (f == 0)
        r.check(exp, "outputs %s, flags %d" % (w, f))
    assert (exp[0] != k.coop.pid).any() and (exp[5] == -1).any()


# ---- buffer contract -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", ["aligned", "odd", "three"])
@pytest.mark.parametrize("name", ["at the limit of N", "previous owner owns nothing in the run"])
def test_guard_bands_offset_views_and_untouched_inputs(ctx, torch_dev, name, shifts):
    three(ctx, torch_dev[0], K.case(name), "%s, %s" % (name, shifts), shifts=shifts)


# ---- errors la_sync reports --------------------------------------------------------------------------------------------------------------
def broken(k, bad):
    b = k.copy()
    b.coop = C.break_case(k.coop, bad)
    return b


# (part offsets that end short of N where the last topic has ONE partition: the topic is empty then and its ids cannot disagree,
#  so LA_ESHAPE is all there is to report; offsets that cut through topics make ids foreign as well, and LA_EINVAL comes first)
@pytest.mark.parametrize("bad,code,name", [("duplicate claim, two members", N.LA_EINVAL, "mixed lags"),
                                           ("target rank M", N.LA_EINVAL, "mixed lags"),
                                           ("owned topic T", N.LA_EINVAL, "mixed lags"),
                                           ("part_off ends short of N", N.LA_ESHAPE, "at the limit of M"),
                                           ("descending owned offsets", N.LA_ESHAPE, "mixed lags")])
@pytest.mark.parametrize("flags", [0, N.LA_COOP_FORCE_TABLE])
def test_an_error_of_the_round_is_reported_and_nothing_leaves_the_arrays(ctx, torch_dev, bad, code, name, flags):
    stream = _stream(torch_dev[0])
    k = K.case(name)
    assert name != "at the limit of M" or np.diff(k.coop.part_off)[-1] == 1
    r = Call(ctx, broken(k, bad), stream, flags)
    _expect_sync_error(ctx, stream, code)
    r.check_contract(bad)
    clean = Call(ctx, k, stream, flags)
    ctx.sync(stream)
    clean.check(k.expect(), "the next clean call after %s" % bad)


@pytest.mark.parametrize("bad", ["duplicate input id", "foreign output id"])
def test_a_bad_topic_is_la_einval_and_passed_through_the_others_exact(ctx, torch_dev, bad):
    stream = _stream(torch_dev[0])
    k = K.case("mixed lags")
    b, t = K.break_input(k, bad)
    exp = b.expect()
    a, z = int(b.coop.part_off[t]), int(b.coop.part_off[t + 1])
    np.testing.assert_array_equal(exp[0][a:z], b.coop.pid[a:z])
    assert exp[3][3] == 1 and exp[3][2] >= 2
    for flags, how in ((0, "call"), (N.LA_COOP_FORCE_TABLE, "call"), (0, "chain")):
        r = Call(ctx, b, stream, flags, how=how)
        _expect_sync_error(ctx, stream, N.LA_EINVAL)
        r.check(exp, "%s, flags %d, %s" % (bad, flags, how))
    clean = Call(ctx, k, stream)
    ctx.sync(stream)
    clean.check(k.expect(), "the next clean call after %s" % bad)


# ---- errors of the call itself -----------------------------------------------------------------------------------------------------------
def test_what_the_call_itself_refuses(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    k = K.case("previous owner owns nothing in the run")

    def size_minus_8(r): r.args.struct_size = ctypes.sizeof(N.CoopStickyArgs) - 8
    def flags_2(r): r.args.flags = 2
    def reserved(r): r.args.round.adjust.reserved = 1
    def wire_out(r): r.batch.flags = N.LA_FLAG_WIRE_OUT
    def in_place(r): r.args.d_sticky_partition = r.batch.d_out_partition
    def over_input(r): r.args.d_sticky_partition = r.batch.d_partition_id
    def no_member_off(r): r.args.round.member_off = None
    def no_sticky(r): r.args.d_sticky_partition = None
    def no_grouped(r): r.args.round.grouped_partition = None

    for edit in (size_minus_8, flags_2, reserved, wire_out, in_place, over_input, no_member_off, no_sticky, no_grouped):
        with pytest.raises(N.LagAssignError) as ei:
            Call(ctx, k, stream, edit=edit)
        assert ei.value.code == N.LA_EINVAL, edit.__name__
    with pytest.raises(N.LagAssignError) as ei:
        ctx.cooperative_round_sticky_device(None, N.CoopStickyArgs(), stream)
    assert ei.value.code == N.LA_EINVAL
    ok = Call(ctx, k, stream)                                         # nothing was enqueued by any of them
    ctx.sync(stream)
    ok.check(k.expect(), "after the refused calls")
    assert ok.launches == 1


def test_the_target_fields_of_round_are_not_looked_at(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    k = K.case("mixed lags")

    def poison(r):
        adj = r.args.round.adjust
        adj.struct_size, adj.n_topics, adj.n_partitions = 3, -5, 1 << 40
        adj.d_part_off, adj.d_out_partition, adj.d_out_member_rank = 8, 16, 24
        r.args.round.struct_size, r.args.round.flags = 1, 2

    r = Call(ctx, k, stream, edit=poison)
    ctx.sync(stream)
    r.check(k.expect(), "poisoned target fields")


# ---- la_assign_batch_cooperative_sticky: the host call --------------------------------------------------------------------------------
HOST_FIELDS = ("sticky_partition", "topic_kept", "topic_saved", "sticky_summary")


def host_buffers(h):
    """Caller-owned outputs holding SENTINEL -> (AssignSticky, every array of it by name)."""
    n, m, t = h.n, h.m, h.t
    i32 = lambda s: np.full(s, SENTINEL, np.int32)
    i64 = lambda s: np.full(s, SENTINEL, np.int64)
    coop = N.AssignCoop(i32(n), i32(n), i64(h.k), i32(n), i32(n), i64(m), i64(m), i64(m), i64(m), i64(t), i64(6), i64(m + 1), i32(n), i32(n))
    out = N.AssignSticky(coop, i32(n), i64(t), i64(t), i64(4))
    arrays = dict(zip(N.AssignCoop._fields, coop))
    arrays.update(zip(HOST_FIELDS, out[1:]))
    return out, arrays


def host_call(ctx, h, mode, force=False, out=None, owned=None):
    off, topic, pid = owned if owned is not None else h.owned
    return ctx.assign_batch_cooperative_sticky(h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, off, topic, pid, force_table=force,
                                               out=out, **h.inputs(mode))


def host_same(got, exp, what=""):
    """exp: the eighteen outputs of assign_cooperative_sticky_numpy (target, sticky outputs, round outputs)."""
    for name, g, e in zip(("out_partition", "out_member_rank", "totals"), got.coop[:3], exp[:3]):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))
    for name, g, e in zip(HOST_FIELDS, got[1:], exp[3:7]):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))
    for name, g, e in zip(N.AssignCoop._fields[3:], got.coop[3:], exp[7:]):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))


@pytest.mark.parametrize("mode", K.HOST_MODES)
@pytest.mark.parametrize("name", K.HOST_NAMES)
def test_host_call(ctx, torch_dev, name, mode):
    h = K.host_case(name)
    exp = h.expect(mode)
    inputs = [h.part_off, h.pid, h.cons_off, h.cons_rank, h.lag, h.begin, h.end, h.committed] + list(h.owned)
    before = [x.copy() for x in inputs]
    launches = []
    for force in (False, True):
        got = host_call(ctx, h, mode, force)
        launches.append(ctx.last_launches())
        host_same(got, exp, "%s, %s, force %s" % (name, mode, force))
    assert launches[1] > launches[0] or name == "one over the limit", "the round is one launch within the limits, unforced"
    for a, b in zip(inputs, before):
        np.testing.assert_array_equal(a, b)
    # the target is la_assign_batch_cooperative's for the same inputs
    plain = ctx.assign_batch_cooperative(h.part_off, h.pid, h.cons_off, h.cons_rank, h.m, *h.owned, **h.inputs(mode))
    for k in range(3):
        np.testing.assert_array_equal(got.coop[k], plain[k], err_msg=N.AssignCoop._fields[k])
    if name != "tiny":
        assert got.coop.summary[2] < plain.summary[2], "the caught-up group withholds less on the sticky order"


def test_host_call_leaves_the_outputs_untouched_on_an_error_and_consumes_the_hint(ctx, torch_dev):
    h = K.host_case("at the limit")
    off, topic, pid = (x.copy() for x in h.owned)
    live = np.flatnonzero((np.arange(topic.size) >= off[0]) & (np.arange(topic.size) < off[-1]))
    topic[live[-1]], pid[live[-1]] = topic[live[0]], pid[live[0]]    # one partition claimed by the first and by the last member
    for force in (False, True):
        out, arrays = host_buffers(h)
        with pytest.raises(N.LagAssignError) as ei:
            host_call(ctx, h, "sparse", force, out=out, owned=(off, topic, pid))
        assert ei.value.code == N.LA_EINVAL
        for name, a in arrays.items():
            assert (a == SENTINEL).all(), "%s was written by a call that failed" % name
    for bad in ("reserved", "flags", "size"):
        a = N.AssignStickyArgs()
        a.struct_size = ctypes.sizeof(N.AssignStickyArgs) - (8 if bad == "size" else 0)
        a.reserved = 1 if bad == "reserved" else 0
        a.coop.flags = 2 if bad == "flags" else 0
        assert N.load().la_assign_batch_cooperative_sticky(ctx._h, ctypes.byref(a)) == N.LA_EINVAL, bad
    out, _ = host_buffers(h)
    host_same(host_call(ctx, h, "sparse", out=out), h.expect("sparse"), "caller-owned buffers, after the failed calls")
    # a pending hint is taken by the call, exact with it, and spent by it -- also by a call that fails (launches as unhinted after)
    small = K.HostCase(53, [40, 9, 25], 4)
    small.lag = small.lag % 1000                                     # (bounds under which every tile packs)
    exp = small.expect("lag")
    bounds = N.offset_bounds(None, None, None, small.pid, lag=small.lag)
    assert bounds is not None
    host_same(host_call(ctx, small, "lag"), exp, "unhinted")
    unhinted = ctx.last_launches()
    ctx.hint_next_call(bounds)
    host_same(host_call(ctx, small, "lag"), exp, "hinted")
    assert ctx.last_launches() <= unhinted
    host_same(host_call(ctx, small, "lag"), exp, "the hint was spent")
    assert ctx.last_launches() == unhinted
    ctx.hint_next_call(bounds)
    with pytest.raises(N.LagAssignError):
        host_call(ctx, small, "lag", owned=([0, 1, 2, 2, 2], [0, 0], [small.pid[0], small.pid[0]]))
    host_same(host_call(ctx, small, "lag"), exp, "after a failed hinted call")
    assert ctx.last_launches() == unhinted


# ---- the host mirror --------------------------------------------------------------------------------------------------------------------
class Offsets:
    def __init__(self, begin, end, committed):
        self.begin, self.end, self.com = begin, end, committed

    def beginning_offsets(self, tps):
        return {tp: self.begin[tp] for tp in tps}

    def end_offsets(self, tps):
        return {tp: self.end[tp] for tp in tps}

    def committed(self, tps):
        return {tp: self.com.get(tp) for tp in tps}


def mirror_group(lagging):
    """Two topics of a group that has caught up: every lag 0 but for the partitions in `lagging`."""
    metadata = {"orders": list(range(24)), "payments": list(range(9))}
    tps = [(t, p) for t, ps in metadata.items() for p in ps]
    lag = {tp: (1000 + 7 * i if tp in lagging else 0) for i, tp in enumerate(tps)}
    return metadata, lag, Offsets({tp: 0 for tp in tps}, {tp: 500 + lag[tp] for tp in tps}, {tp: 500 for tp in tps})


def test_host_mirror_with_the_key_on_withholds_less_and_reports_the_sticky_numbers():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor, _host
    subs = {"app-1": ["orders", "payments"], "app-2": ["orders", "payments"], "app-3": ["orders"]}
    metadata, _, src_before = mirror_group({("orders", 3), ("payments", 1)})
    _, lag, src = mirror_group({("orders", 17), ("payments", 6)})
    off_a, on_a, default_a = LagBasedPartitionAssignor(), LagBasedPartitionAssignor(), LagBasedPartitionAssignor()
    off_a.configure({"group.id": "g", "auto.offset.reset": "earliest", "lag.assignor.sticky.ties": "false"})
    on_a.configure({"group.id": "g", "auto.offset.reset": "earliest", "lag.assignor.sticky.ties": "true"})
    default_a.configure({"group.id": "g", "auto.offset.reset": "earliest"})
    owned = {m: [tuple(tp) for tp in tps] for m, tps in off_a.assign(metadata, subs, src_before).items()}
    target = off_a.assign(metadata, subs, src)
    loads = off_a.last_member_loads()
    # key off, and no key: today's call
    got_off = off_a.assign_cooperative(metadata, subs, owned, src)
    c_off = off_a.last_cooperative_round()
    assert default_a.assign_cooperative(metadata, subs, owned, src) == got_off
    assert default_a.last_cooperative_round() == c_off
    assert (c_off["sticky_kept_before"], c_off["sticky_kept_after"], c_off["sticky_topics_passed_through"]) == (0, 0, 0)
    assert c_off["withheld"] > 0, "the plain order withholds something"
    # key on
    got_on = on_a.assign_cooperative(metadata, subs, owned, src)
    c_on = on_a.last_cooperative_round()
    assert c_on["withheld"] < c_off["withheld"]
    assert on_a.last_member_loads() == loads, "the target accessors describe the target"
    # the numpy model: the target in the reference's order per topic (lag descending, id ascending), the owned arrays of the mirror
    h = _host()
    members, topics = list(subs), list(metadata)
    rank = dict(zip(members, h.rank_members(members)))
    owner_now = {tuple(tp): rank[m] for m, tps in target.items() for tp in tps}
    flat = [(t, p) for t in topics for p in sorted(metadata[t], key=lambda p: (-lag[(t, p)], p))]
    part_off = np.concatenate([[0], np.cumsum([len(metadata[t]) for t in topics])])
    off, o_topic, o_pid = h.cooperative_owned_arrays(members, topics, [list(owned.get(m, ())) for m in members])
    pid_in = [p for t in topics for p in metadata[t]]
    exp = sharding_model(part_off, pid_in, [lag[(t, p)] for t in topics for p in metadata[t]], [p for _, p in flat],
                         [owner_now.get(tp, -1) for tp in flat], len(members), off, o_topic, o_pid)
    assert (c_on["sticky_kept_before"], c_on["sticky_kept_after"], c_on["sticky_topics_passed_through"]) == \
        (int(exp[3][0]), int(exp[3][1]), int(exp[3][3]))
    assert c_on["sticky_kept_before"] == c_off["kept"] and c_on["sticky_kept_after"] == c_on["kept"]
    summary = exp[4 + 7].tolist()
    assert [c_on["kept"], c_on["fresh"], c_on["withheld"], c_on["dropped"], c_on["stale"], int(c_on["followup"])] == summary
    member_off, g_topic, g_pid = exp[-3:]
    for m in members:                                                # (inside a topic in the order of the sticky assignment)
        a, z = int(member_off[rank[m]]), int(member_off[rank[m] + 1])
        model = [(topics[int(t)], int(p)) for t, p in zip(g_topic[a:z], g_pid[a:z])]
        for topic in topics:
            assert [tuple(tp) for tp in got_on[m] if tuple(tp)[0] == topic] == [tp for tp in model if tp[0] == topic], (m, topic)


def sharding_model(*args):
    from kafka_lag_based_assignor_amd import sharding
    return sharding.cooperative_round_sticky_numpy(*args)
