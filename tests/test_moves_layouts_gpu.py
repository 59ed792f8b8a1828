"""la_assignment_moves_device[_on] with a layout per assignment (d_prev_part_off) on the GPU: topics that gained or lost
partitions, new topics, emptied topics.  The yardstick is sharding.assignment_moves_layouts_numpy (tests/test_moves_layouts_cpu.py
holds it against a naive dict join), applied to the ORACLE's two assignments where the test runs the assign calls and to synthetic
assignments (tests/moves_layouts_cases.py) elsewhere.  Every comparison is bit for bit; every array is a Guarded buffer at an
element shift of its own, and outputs hold SENTINEL before a call."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

from gpu_helpers import SENTINEL, Guarded, _grouped_expect, _workload, shifts_for
from moves_layouts_cases import I32, NAMES as OUTPUTS, LCase, build, same

pytestmark = pytest.mark.gpu

L = N.MOVES_LDS_MAX_PARTITIONS          # up to here (both sides) a pair is joined in LDS, beyond it in a table in device memory
B = N.MOVES_LDS_MAX_MEMBERS             # up to here gained / lost are LDS bins, beyond it global atomics
INPUTS = ("part_off", "cur_pid", "cur_rank", "prev_part_off", "prev_pid", "prev_rank", "rank_map", "prev_topic")
HOST = ("part_off", "prev_part_off", "prev_topic")
FIELD = {"prev_owner": "d_prev_owner", "topic_moved": "d_topic_moved", "topic_added": "d_topic_added",
         "topic_removed": "d_topic_removed", "gained": "d_member_gained", "lost": "d_member_lost", "moved": "d_moved",
         "added": "d_added", "removed": "d_removed"}
ONE_LAYOUT = ("prev_owner", "topic_moved", "gained", "lost", "moved")
MIXED = shifts_for("mixed", INPUTS + OUTPUTS)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _host_ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


class Run:
    """One call.  host: which host copies are passed (those of `host_from`, default: the case's own); one_layout:
    d_prev_part_off stays NULL (the previous arrays then follow today's layout); struct_size: what the args claim (default: the
    binding's); trailing: the byte that fills the struct behind its first 128 bytes."""

    def __init__(self, ctx, case, stream, shifts=MIXED, want=OUTPUTS, host=HOST, shard=0, hint=None, one_layout=False,
                 struct_size=None, trailing=None, host_from=None):
        self.case, self.want = case, want
        n_of = {"part_off": case.t + 1, "cur_pid": case.n, "cur_rank": case.n, "prev_part_off": case.t_prev + 1,
                "prev_pid": case.n_prev, "prev_rank": case.n_prev, "prev_owner": case.n, "topic_moved": case.t,
                "topic_added": case.t, "topic_removed": case.t, "gained": case.m, "lost": case.m, "moved": 1, "added": 1, "removed": 1}
        self.g = {}
        for k in INPUTS:
            v = getattr(case, k)
            if v is not None:
                self.g[k] = Guarded("device", v.size, v.dtype, shifts.get(k, 0), v, name=k)
        for k in OUTPUTS:
            self.g[k] = Guarded("device", n_of[k], np.int32 if k == "prev_owner" else np.int64, shifts.get(k, 0), name=k)
        a = N.MovesArgs()
        if trailing is not None:                                     # whatever lies behind the one-layout struct
            ctypes.memset(ctypes.addressof(a) + 128, trailing, ctypes.sizeof(a) - 128)
        a.n_topics, a.n_partitions = case.t, case.n
        a.max_partitions_per_topic = case.hint if hint is None else hint
        a.d_part_off = self.g["part_off"].ptr
        self.keep = keep = {k: getattr(host_from or case, k) for k in HOST}          # kept alive
        if "part_off" in host:
            a.h_part_off = _host_ptr(keep["part_off"], ctypes.c_int64)
        a.d_out_partition, a.d_out_member_rank = self.g["cur_pid"].ptr, self.g["cur_rank"].ptr
        a.d_prev_partition, a.d_prev_member_rank = self.g["prev_pid"].ptr, self.g["prev_rank"].ptr
        a.n_members = case.m
        if case.rank_map is not None:
            a.n_prev_members, a.d_prev_rank_map = case.rank_map.size, self.g["rank_map"].ptr
        if not one_layout:
            a.n_prev_topics, a.n_prev_partitions = case.t_prev, case.n_prev
            a.d_prev_part_off = self.g["prev_part_off"].ptr
            if "prev_part_off" in host:
                a.h_prev_part_off = _host_ptr(keep["prev_part_off"], ctypes.c_int64)
            if case.prev_topic is not None:
                a.d_prev_topic = self.g["prev_topic"].ptr
                if "prev_topic" in host:
                    a.h_prev_topic = _host_ptr(keep["prev_topic"], ctypes.c_int32)
        for k in want:
            if not (one_layout and trailing is not None and k not in ONE_LAYOUT):
                setattr(a, FIELD[k], self.g[k].ptr)
        if struct_size is not None:
            a.struct_size = struct_size
        self.args = a
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        ctx.assignment_moves_device(a, stream, shard=shard)
        self.launches = ctx.last_launches()

    def outputs(self):
        v = [self.g[k].values() for k in OUTPUTS]
        return tuple(v[:6]) + tuple(int(x[0]) for x in v[6:])

    def check_contract(self, what=""):
        for k in INPUTS:
            if k in self.g:
                self.g[k].check_unchanged(what)
        for k in OUTPUTS:
            self.g[k].check_guards(what)

    def check(self, exp=None, what=""):
        """Wanted outputs equal the restatement, the others still hold SENTINEL, nothing outside the arrays was written."""
        exp = self.case.expect() if exp is None else exp
        for k, g, e in zip(OUTPUTS, self.outputs(), exp):
            if k in self.want:
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
            else:
                assert (np.asarray(g) == SENTINEL).all(), "%s was not asked for %s" % (k, what)
        self.check_contract(what)


# ---- pairs (P_prev, P): the LDS form -----------------------------------------------------------------------------------------
LDS_PAIRS = [(0, 5), (5, 0), (0, 0), (1, 1), (63, 64), (64, 65), (255, 257), (256, 256), (300, 300, "disjoint"), (17, 17, "half"),
             (3, 4000), (4000, 3), (L, L - 1), (L - 1, L), (L, L)]


@pytest.mark.parametrize("m", [5, B, B + 1])
def test_pairs_within_the_lds_limit_are_one_launch(ctx, torch_dev, m):
    stream = _stream(torch_dev[0])
    c = build(m, LDS_PAIRS, m)
    exp = c.expect()
    assert exp[6] > 0 and exp[7] > 4000 and exp[8] > 4000 and exp[2][0] == 5 and exp[3][1] == 5 and exp[2][7] == 0 and exp[2][8] == 300
    for host in (HOST, ()):
        r = Run(ctx, c, stream, host=host)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(exp, "LDS pairs, M = %d, host copies %s" % (m, host))


# ---- the global form ---------------------------------------------------------------------------------------------------------
GLOBAL_PAIRS = {
    "at the limit": [(L + 1, L), (L, L + 1), (9000, 5000), (0, 5000), (5000, 0)],
    "step edges": [(5 * 1024 - 1, 5 * 1024 + 1), (5 * 1024 + 1, 5 * 1024 - 1, "half"), (5 * 1024, 6 * 1024, "disjoint")],
    "beside small topics": [(L + 1, 100), (50, 60), (300, 9000), (0, 0), (5000, 5000, "half"), (10, 0), (0, 7), (L, L)],
    "large only": [(2 * L, 2 * L + 5, "half")],
}


@pytest.mark.parametrize("m", [8, B + 1])
@pytest.mark.parametrize("pairs", list(GLOBAL_PAIRS))
def test_pairs_beyond_the_lds_limit_go_through_the_table_in_device_memory(ctx, torch_dev, pairs, m):
    stream = _stream(torch_dev[0])
    c = build(3, GLOBAL_PAIRS[pairs], m, ids="full")
    exp = c.expect()
    assert exp[7] > 0 and exp[8] > 0
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    assert 2 <= r.launches <= 4
    r.check(exp, pairs)
    r = Run(ctx, c, stream)                                          # the table is cleared per call
    ctx.sync(stream)
    r.check(exp, pairs + ", second call")
    r = Run(ctx, c, stream, hint=L)                                  # within the limit the same call is a shape error
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE and r.launches == 1
    r.check_contract(pairs + ", hint at the limit")


# ---- topic maps ------------------------------------------------------------------------------------------------------------
MAP_PAIRS = {"lds": [(40, 56), (None, 30), (56, 40), (25, 0), (0, 25), (None, 0), (64, 64), (300, 200, "half")],
             "global": [(40, 56), (None, L + 3), (L + 9, 40), (None, 30), (25, 0), (5000, 5200)]}


@pytest.mark.parametrize("form", list(MAP_PAIRS))
def test_topic_maps_permuted_with_new_topics_and_unreferenced_previous_topics(ctx, torch_dev, form):
    stream = _stream(torch_dev[0])
    c = build(5, MAP_PAIRS[form], 21, topic_map="permute", extra_prev=(33, 0, 700 if form == "lds" else L + 50))
    assert c.t_prev != c.t and (c.prev_topic < 0).sum() == 2 and not (np.diff(c.prev_topic[c.prev_topic >= 0]) > 0).all()
    r = Run(ctx, c, stream)                                          # (the unreferenced topics hold duplicates and ranks out of
    ctx.sync(stream)                                                 #  range: looking at them would be LA_EINVAL)
    r.check(what="permuted map, " + form)
    assert r.launches == (1 if form == "lds" else 4)
    pairs = [p for p in MAP_PAIRS[form] if p[0] is not None]
    a, b = build(6, pairs, 21), build(6, pairs, 21, topic_map="same")
    ra, rb = Run(ctx, a, stream), Run(ctx, b, stream)
    ctx.sync(stream)
    ra.check(what="no map, " + form)
    rb.check(what="identity map, " + form)
    same(rb.outputs(), ra.outputs(), "identity map against NULL")


# ---- ids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["full", "4096", "2^20"])
def test_any_int32_is_an_id(ctx, torch_dev, ids):
    stream = _stream(torch_dev[0])
    pairs = [(300, 280, "half"), (4, 9), (1, 1500), (1500, 1), (200, 200, "disjoint")]
    if ids != "2^20":                                                # (beyond 4 096 ids of that stride leave int32)
        pairs.append((L + 1, L + 2, "half"))
    c = build(7, pairs, 40, ids=ids)
    if ids == "full":
        assert {I32.min, -1, 0, I32.max} <= set(c.cur_pid[:280].tolist()) | set(c.prev_pid[:300].tolist())
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    r.check(what=ids)


# ---- equal layouts, struct_size --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[200, 31, 300, 0, 77, L], [L + 7, 50, 0]], ids=["lds", "global"])
def test_equal_layouts_equal_the_one_layout_call(ctx, torch_dev, sizes):
    stream = _stream(torch_dev[0])
    c = build(8, [(p, p) for p in sizes], 33, ids="full")
    one = Run(ctx, c, stream, one_layout=True, want=ONE_LAYOUT)
    two = Run(ctx, c, stream)
    # a caller built against the one-layout header: 128 bytes, and whatever lies behind them is not read
    old = Run(ctx, c, stream, one_layout=True, want=OUTPUTS, struct_size=128, trailing=0xFF)
    ctx.sync(stream)
    exp = c.expect()
    two.check(exp, "two equal layouts")
    assert exp[7] == exp[8] == 0 and not exp[2].any() and not exp[3].any()
    want = sharding.assignment_moves_numpy(c.part_off, c.cur_pid, c.cur_rank, c.prev_pid, c.prev_rank, c.m)
    for r, what in ((one, "d_prev_part_off NULL"), (old, "struct_size 128")):
        got = r.outputs()
        same((got[0], got[1], got[4], got[5], got[6]), want, what)
        same((got[0], got[1], got[4], got[5], got[6]), (exp[0], exp[1], exp[4], exp[5], exp[6]), what + " against two layouts")
        assert all((np.asarray(got[i]) == SENTINEL).all() for i in (2, 3, 7, 8)), "the one-layout form writes five outputs"
        r.check_contract(what)
        assert r.launches == two.launches - (0 if sizes[0] <= L else 1)
    for size in (129, 127, ctypes.sizeof(N.MovesArgs) - 1, -1):
        with pytest.raises(N.LagAssignError) as ei:
            Run(ctx, c, stream, struct_size=size)
        assert ei.value.code == N.LA_EINVAL and ctx.last_launches() == 0, size
    r = Run(ctx, c, stream, struct_size=ctypes.sizeof(N.MovesArgs) + 64)      # a later header's struct: what this library knows of it
    ctx.sync(stream)
    r.check(exp, "a larger struct_size")


# ---- optional outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [[(200, 231), (31, 0), (300, 150, "half"), (0, 0), (0, 77)], [(L + 1, L + 40, "half"), (50, 20)]],
                         ids=["lds", "global"])
def test_every_output_is_optional(ctx, torch_dev, pairs):
    stream = _stream(torch_dev[0])
    c = build(9, pairs, 33)
    exp = c.expect()
    wants = [(k,) for k in OUTPUTS] + [tuple(x for x in OUTPUTS if x != k) for k in OUTPUTS]
    runs = [Run(ctx, c, stream, want=w) for w in wants]
    ctx.sync(stream)
    for w, r in zip(wants, runs):
        r.check(exp, "outputs %s" % (w,))
    with pytest.raises(N.LagAssignError) as ei:
        Run(ctx, c, stream, want=())
    assert ei.value.code == N.LA_EINVAL and ctx.last_launches() == 0
    ctx.sync(stream)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def _broken(c, bad, t=1):
    """A copy of `c` with one entry of topic `t` (or its map entry) broken.  The topic's first current id has a previous entry."""
    b = c.copy()
    i, (j, nq) = int(c.part_off[t]), c.segment_of(t)
    assert nq > 3 and c.part_off[t + 1] - i > 3
    shared = np.intersect1d(c.cur_pid[i:int(c.part_off[t + 1])], c.prev_pid[j:j + nq])
    if bad == "duplicate id, previous":
        b.prev_pid[j + 1] = b.prev_pid[j + 2]
    elif bad == "duplicate id, current":
        at = i + np.flatnonzero(c.cur_pid[i:int(c.part_off[t + 1])] != shared[0])[0]
        b.cur_pid[at] = shared[0]
    elif bad == "current rank M":
        b.cur_rank[i + 1] = c.m
    elif bad == "current rank -2":
        b.cur_rank[i + 1] = -2
    elif bad == "previous rank M":
        b.prev_rank[j + 1] = c.m if c.rank_map is None else c.rank_map.size
    elif bad == "previous rank -2":
        b.prev_rank[j + 1] = -2
    elif bad == "map entry M":
        b.prev_rank[j + 1] = max(int(b.prev_rank[j + 1]), 0)
        b.rank_map[int(b.prev_rank[j + 1])] = c.m
    elif bad == "topic map entry T_prev":
        b.prev_topic[t] = c.t_prev
    elif bad == "topic map entry -2":
        b.prev_topic[t] = -2
    else:
        raise ValueError(bad)
    return b


ERRORS = ["duplicate id, previous", "duplicate id, current", "current rank M", "current rank -2", "previous rank M",
          "previous rank -2", "map entry M", "topic map entry T_prev", "topic map entry -2"]


@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("bad", ERRORS)
def test_broken_input_is_reported_and_never_stored_through(ctx, torch_dev, bad, form):
    """In the global form the host copies stay valid (a bad host copy is refused at the call, test_shape_errors_...): what is
    broken is what the device reads."""
    stream = _stream(torch_dev[0])
    m = 9 if form == "lds" else B + 1
    rank_map = np.random.default_rng(1).permutation(m).astype(np.int32) if bad == "map entry M" else None
    pairs = [(20, 25), (30, 40, "half"), (22, 20)] if form == "lds" else [(20, 25), (L + 30, L + 40, "half"), (22, 20)]
    c = build(12, pairs, m, rank_map=rank_map, topic_map="same", hint=None if form == "lds" else L + 100)
    b = _broken(c, bad)
    with pytest.raises(ValueError):
        b.expect()                                                   # the restatement refuses the same input
    r = Run(ctx, b, stream, host_from=c)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_EINVAL and "la_assignment_moves_device" in str(ei.value)
    r.check_contract(bad)
    r = Run(ctx, c, stream)                                          # the next call on the same context is an ordinary one
    ctx.sync(stream)
    r.check(what="after " + bad)


ADDED_DUPS = {"lds": [(20, 25), (0, 40), (None, 300), (30, 50, "half")],
              "global": [(20, 25), (0, L + 40), (None, L + 300), (L + 30, L + 50, "half")]}


@pytest.mark.parametrize("form", list(ADDED_DUPS))
@pytest.mark.parametrize("t", [1, 2, 3], ids=["P_prev = 0", "new topic", "grown topic"])
def test_a_duplicate_among_the_added_ids_is_reported(ctx, torch_dev, form, t):
    """Two current entries with one id that has NO previous entry: neither finds a mark, they have to find each other -- side by
    side (one wavefront) and at the two ends of the segment (in the global form: different workgroups)."""
    stream = _stream(torch_dev[0])
    c = build(13, ADDED_DUPS[form], 9 if form == "lds" else B + 1, topic_map="permute")
    lo, hi = int(c.part_off[t]), int(c.part_off[t + 1])
    q0, nq = c.segment_of(t)
    assert (c.prev_topic[t] < 0) == (t == 2) and nq == (0 if t < 3 else ADDED_DUPS[form][3][0])
    added = lo + np.flatnonzero(~np.isin(c.cur_pid[lo:hi], c.prev_pid[q0:q0 + nq]))
    assert added.size >= 20
    for what, (i, j) in (("neighbours", (added[0], added[1])), ("far apart", (added[0], added[-1]))):
        b = c.copy()
        b.cur_pid[i] = b.cur_pid[j]
        with pytest.raises(ValueError):
            b.expect()
        r = Run(ctx, b, stream)
        with pytest.raises(N.LagAssignError) as ei:
            ctx.sync(stream)
        assert ei.value.code == N.LA_EINVAL and "la_assignment_moves_device" in str(ei.value), what
        r.check_contract(what)
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    r.check(what="after the duplicates")


def _without_topic(c, t):
    """`c` as if topic t held nothing on either side: what the call computes when it skips the topic."""
    lo, hi = int(c.part_off[t]), int(c.part_off[t + 1])
    keep = np.r_[0:lo, hi:c.n]
    po = c.part_off.copy()
    po[t + 1:] -= hi - lo
    pt = (np.arange(c.t) if c.prev_topic is None else c.prev_topic).copy()
    pt[t] = -1
    return LCase(po, c.cur_pid[keep], c.cur_rank[keep], c.prev_part_off, c.prev_pid, c.prev_rank, c.m, c.rank_map, pt), keep


@pytest.mark.parametrize("side", ["current", "previous"])
def test_a_pair_over_a_hint_within_the_limit_is_a_shape_error_and_is_left_alone(ctx, torch_dev, side):
    stream = _stream(torch_dev[0])
    big = (60, 120) if side == "current" else (120, 60)
    c = build(14, [(50, 70), big, (60, 30), (0, 0)], 12, hint=100)
    r = Run(ctx, c, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    r.check_contract("a pair over the hint")
    got = r.outputs()
    lo, hi = int(c.part_off[1]), int(c.part_off[2])
    assert (got[0][lo:hi] == SENTINEL).all() and got[1][1] == got[2][1] == got[3][1] == SENTINEL      # nothing is written for it
    rest, keep = _without_topic(c, 1)
    exp = rest.expect()
    np.testing.assert_array_equal(got[0][keep], exp[0])
    for i in (1, 2, 3):
        np.testing.assert_array_equal(got[i][[0, 2, 3]], exp[i][[0, 2, 3]])
    same(got[4:], exp[4:], "the other topics")
    r = Run(ctx, c, stream, hint=L + 1)                              # a larger hint: every pair is done by its real size
    ctx.sync(stream)
    r.check(what="large hint, small pairs")
    assert r.launches == 1


def test_host_copies_are_required_and_validated_beyond_the_limit(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = build(15, [(50, 70), (None, 20), (60, 30)], 12, topic_map="permute", extra_prev=(5,))

    def refused(what, **kw):
        with pytest.raises(N.LagAssignError) as ei:
            Run(ctx, kw.pop("case", c), stream, hint=L + 1, **kw)
        assert ei.value.code == N.LA_EINVAL, what
        assert ctx.last_launches() == 0, what                        # nothing was enqueued

    for k in HOST:
        refused("no host copy of " + k, host=tuple(x for x in HOST if x != k))
    for k, i, v in (("part_off", 1, 200), ("part_off", c.t, c.n + 1), ("part_off", 0, 1), ("prev_part_off", 1, -1),
                    ("prev_part_off", c.t_prev, c.n_prev - 1), ("prev_topic", 0, c.t_prev), ("prev_topic", 2, -2)):
        b = c.copy()
        getattr(b, k)[i] = v
        b.n, b.n_prev = c.n, c.n_prev
        refused("host %s[%d] = %d" % (k, i, v), case=b)
    r = Run(ctx, c, stream, host=())                                 # within the limit no host copy is looked at
    ctx.sync(stream)
    r.check(what="no host copies, hint within the limit")
    no_map = build(16, [(50, 70), (60, 30)], 12)
    r = Run(ctx, no_map, stream)
    ctx.sync(stream)
    for field, v in (("n_prev_topics", 3), ("reserved", 1), ("n_prev_topics", -1), ("n_prev_partitions", -1)):
        was = getattr(r.args, field)                                 # without a map both layouts hold the same topics; sizes >= 0
        setattr(r.args, field, v)
        with pytest.raises(N.LagAssignError) as ei:
            ctx.assignment_moves_device(r.args, stream)
        assert ei.value.code == N.LA_EINVAL and ctx.last_launches() == 0, field
        setattr(r.args, field, was)
    junk = np.full(no_map.t, 99, np.int32)                           # without d_prev_topic its host copy is not looked at
    r.args.h_prev_topic, r.args.max_partitions_per_topic = _host_ptr(junk, ctypes.c_int32), L + 1
    ctx.assignment_moves_device(r.args, stream)
    ctx.sync(stream)
    r.check(what="h_prev_topic without d_prev_topic")


# ---- empty sides -----------------------------------------------------------------------------------------------------------
def test_empty_sides_zero_the_outputs(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    e, z1, z5 = np.empty(0, np.int32), np.zeros(1, np.int64), np.zeros(5, np.int64)
    for what, c, launches in (("T = 0", LCase(z1, e, e, z1, e, e, 6), 0),
                              ("N = 0 and N_prev = 0", LCase(z5, e, e, z5, e, e, 6), 0),
                              ("T = 0 over a previous layout", LCase(z1, e, e, [0, 2], [1, 1], [9, 9], 6, prev_topic=e), 0),
                              ("N = 0: everything removed", build(1, [(40, 0), (0, 0), (7, 0)], 6), 1),
                              ("N_prev = 0: everything added", build(2, [(0, 40), (0, 0), (0, 7)], 6), 1),
                              ("every topic new", build(3, [(None, 40), (None, 0)], 6, topic_map="permute"), 1)):
        r = Run(ctx, c, stream)
        ctx.sync(stream)
        assert r.launches == launches, what
        r.check(what=what)
        got = r.outputs()
        assert got[6] == 0 and got[7] == c.n and got[8] == (c.n_prev if c.t else 0), what


# ---- behind two assign calls on one stream -----------------------------------------------------------------------------------
def _two_rebalances():
    """A ragged workload, then the same topics with some grown by new partitions, one emptied, one new topic in their midst and a
    third of the members gone with new ones joined -> (previous workload, today's, rank map, M, topic map)."""
    rng = np.random.default_rng(31)
    w1 = synth.ragged(21, 120, 300, 40)
    m_prev = int(w1.cons_rank.max()) + 1
    rank_map = np.full(m_prev, -1, np.int32)
    stay = np.array([r for r in range(m_prev) if r % 3 != 1])
    rank_map[stay] = np.arange(stay.size, dtype=np.int32) * 2 + 1           # ascending: a topic's ranks keep their order
    m = 2 * stay.size + 1
    names1 = ["topic-%d" % t for t in range(w1.n_topics)]
    pids, ranks, names = [], [], []
    for t in range(w1.n_topics):
        if t == 60:
            names.append("brand-new")
            pids.append(np.arange(90, dtype=np.int32))
            ranks.append(np.array([0, 2, 4, 7], np.int32))
        ids = w1.partition_id[int(w1.part_off[t]):int(w1.part_off[t + 1])]
        if t % 7 == 3:                                                       # grown by 16 partitions
            ids = np.concatenate([ids, int(ids.max(initial=-1)) + 1 + np.arange(16, dtype=np.int32)])
        elif t == 11:                                                        # emptied
            ids = ids[:0]
        kept = rank_map[w1.cons_rank[int(w1.cons_off[t]):int(w1.cons_off[t + 1])]]
        names.append(names1[t])
        pids.append(ids.astype(np.int32))
        ranks.append(np.unique(np.concatenate([kept[kept >= 0], [2 * (t % stay.size)]])).astype(np.int32))      # ... and one joined
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    n = int(off(pids)[-1])
    lag = rng.integers(0, 1 << 40, n).astype(np.int64)
    w2 = synth.Workload("today", len(names), off(pids), np.concatenate(pids), np.zeros(n, np.int64), lag.copy(), np.zeros(n, np.int64),
                        lag, off(ranks), np.concatenate(ranks), max(len(x) for x in pids), max(len(x) for x in ranks))
    return w1, w2, rank_map, m, sharding.prev_topic_map(names1, names)


def test_end_to_end_behind_two_assign_calls_on_one_stream(ctx, torch_dev):
    torch, dev = torch_dev
    w1, w2, rank_map, m, prev_topic = _two_rebalances()
    assert prev_topic[60] == -1 and prev_topic[61] == 60 and w2.n_topics == w1.n_topics + 1
    sides = []
    for w in (w1, w2):
        pid, rank, _ = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
        sides.append((pid, rank))
    c = LCase(w2.part_off, sides[1][0], sides[1][1], w1.part_off, sides[0][0], sides[0][1], m, rank_map, prev_topic)
    exp = c.expect()
    assert exp[6] > 0 and exp[7] >= 90 + 16 * 17 and exp[8] == w1.part_off[12] - w1.part_off[11] > 0 and exp[2][60] == 90
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep, batches, res = [], [], []
    for w in (w1, w2):
        d = {k: up(getattr(w, k)) for k in ("part_off", "partition_id", "lag", "cons_off", "cons_rank")}
        out = [torch.full((w.n_partitions,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
        po, co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = w.n_topics, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = w.n_partitions, w.cons_rank.size
        b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
        b.d_part_off, b.d_partition_id, b.d_lag = d["part_off"].data_ptr(), d["partition_id"].data_ptr(), d["lag"].data_ptr()
        b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out[0].data_ptr(), out[1].data_ptr(), None
        b.h_part_off, b.h_cons_off = _host_ptr(po, ctypes.c_int64), _host_ptr(co, ctypes.c_int64)
        keep.append((d, po, co))
        batches.append(b)
        res.append(out)
    d_map, d_topic = up(rank_map), up(prev_topic)
    outs = {k: torch.full((n,), SENTINEL, dtype=torch.int32 if k == "prev_owner" else torch.int64, device=dev)
            for k, n in zip(OUTPUTS, (c.n, c.t, c.t, c.t, m, m, 1, 1, 1))}
    a = N.MovesArgs()
    a.n_topics, a.n_partitions, a.max_partitions_per_topic = c.t, c.n, max(w1.max_partitions, w2.max_partitions)
    a.d_part_off, a.d_out_partition, a.d_out_member_rank = batches[1].d_part_off, res[1][0].data_ptr(), res[1][1].data_ptr()
    a.d_prev_part_off, a.d_prev_partition, a.d_prev_member_rank = batches[0].d_part_off, res[0][0].data_ptr(), res[0][1].data_ptr()
    a.n_prev_topics, a.n_prev_partitions = c.t_prev, c.n_prev
    a.n_members, a.n_prev_members, a.d_prev_rank_map, a.d_prev_topic = m, rank_map.size, d_map.data_ptr(), d_topic.data_ptr()
    for k in OUTPUTS:
        setattr(a, FIELD[k], outs[k].data_ptr())
    torch.cuda.synchronize()                                         # the uploads ran on torch's stream
    stream = _stream(torch)
    for b in batches:                                                # previous, today, the join: enqueued end to end
        ctx.assign_batch_device(b, stream)
    ctx.assignment_moves_device(a, stream)
    launches = ctx.last_launches()
    ctx.sync(stream)                                                 # the first wait
    got = [outs[k].cpu().numpy() for k in OUTPUTS]
    same(tuple(got[:6]) + tuple(int(x[0]) for x in got[6:]), exp, "behind two assign calls")
    np.testing.assert_array_equal(res[1][0].cpu().numpy(), c.cur_pid)            # (the join read what the oracle says it read)
    np.testing.assert_array_equal(res[0][1].cpu().numpy(), c.prev_rank)
    assert launches == 1


# ---- shards, kept results --------------------------------------------------------------------------------------------------
def test_on_shard_one_of_a_two_shard_context(torch_dev):
    c2 = N.Context([0, 0])
    try:
        stream = c2.shard_stream(1)
        torch_dev[0].cuda.synchronize()
        c = build(16, [(100, 116), (L + 1, L + 17), (7, 0), (None, 12)], 20, topic_map="permute", extra_prev=(9,))
        r = Run(c2, c, stream, shard=1)
        c2.sync(stream, shard=1)
        r.check(what="shard 1")
        Run(c2, _broken(c, "duplicate id, previous", t=0), stream, shard=1)          # the error belongs to the shard that ran the call
        c2.sync(c2.shard_stream(0), shard=0)
        with pytest.raises(N.LagAssignError) as ei:
            c2.sync(stream, shard=1)
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
        case = build(18, [(2 * L + 1, 2 * L + 17), (90, 80), (L + 5, 3)], 77)          # unrelated arrays; the table is allocated here
        stream = _stream(torch)
        r = Run(c, case, stream)
        c.sync(stream)
        assert r.launches == 4
        r.check(what="unrelated arrays")
        off, g_t, g_p = c.group_last_by_member(w.n_partitions, m)
        np.testing.assert_array_equal(off, first)
        np.testing.assert_array_equal(g_t, topic)
        np.testing.assert_array_equal(g_p, pid)
    finally:
        c.close()
