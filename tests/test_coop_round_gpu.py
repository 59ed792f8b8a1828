"""la_cooperative_round_device and la_cooperative_round on the GPU: the eight outputs of la_cooperative_adjust_device plus every
member's list of the adjusted assignment, in one call.  The yardstick is sharding.cooperative_round_numpy
(tests/test_coop_round_cpu.py holds it against a dictionary model and a plain grouping).  Every device case runs twice -- as it
comes, and with LA_COOP_FORCE_TABLE -- and the two runs must agree on every output.  Every comparison is bit for bit; outputs hold
SENTINEL before a call, every array sits between guard bands at an element shift of its own."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

from coop_cases import I32, OUTPUTS, CoopCase, break_case, claims_from, owned_arrays, synthetic, topics_of
from gpu_helpers import SENTINEL, Guarded, _grouped_expect, _workload, shifts_for

pytestmark = pytest.mark.gpu

LE, LO, LM, LT = N.COOP_SMALL_ENTRIES, N.COOP_SMALL_OWNED, N.COOP_SMALL_MEMBERS, N.COOP_SMALL_TOPICS
INPUTS = ("part_off", "pid", "rank", "owned_off", "owned_topic", "owned_pid")
LISTS = ("member_off", "grouped_topic", "grouped_partition")
ALL = OUTPUTS + LISTS
FIELD = {"prev_owner": "d_prev_owner", "coop_rank": "d_coop_member_rank", "kept": "d_member_kept", "fresh": "d_member_fresh",
         "pending": "d_member_pending", "release": "d_member_release", "topic_withheld": "d_topic_withheld", "summary": "d_summary"}


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def expect(c):
    return sharding.cooperative_round_numpy(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)


def sizes_of(c):
    return {"prev_owner": c.n, "coop_rank": c.n, "kept": c.m, "fresh": c.m, "pending": c.m, "release": c.m, "topic_withheld": c.t,
            "summary": 6, "member_off": c.m + 1, "grouped_topic": c.n, "grouped_partition": c.n}


def dtype_of(k):
    return np.int32 if k in ("prev_owner", "coop_rank", "grouped_topic", "grouped_partition") else np.int64


def args_of(case, ptr, want, flags=0, null_owned=False):
    """la_coop_round_args over the addresses ptr[name]; member_off and grouped_partition always, the rest where wanted."""
    r = N.CoopRoundArgs()
    r.struct_size, r.flags = ctypes.sizeof(N.CoopRoundArgs), flags
    a = r.adjust
    a.struct_size = ctypes.sizeof(N.CoopArgs)
    a.n_topics, a.n_partitions, a.n_members, a.n_owned = case.t, case.n, case.m, case.n_owned
    a.d_part_off, a.d_out_partition, a.d_out_member_rank = ptr["part_off"], ptr["pid"], ptr["rank"]
    if not null_owned:
        a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = ptr["owned_off"], ptr["owned_topic"], ptr["owned_pid"]
    for k in OUTPUTS:
        if k in want:
            setattr(a, FIELD[k], ptr[k])
    r.member_off, r.grouped_partition = ptr["member_off"], ptr["grouped_partition"]
    if "grouped_topic" in want:
        r.grouped_topic = ptr["grouped_topic"]
    return r


class Round:
    """One call of la_cooperative_round_device: every array a Guarded device buffer (4 KiB guard bands, element shift per array)."""

    def __init__(self, ctx, case, stream, flags=0, shifts=None, want=ALL, null_owned=False):
        shifts = shifts if shifts is not None else shifts_for("mixed", INPUTS + ALL)
        self.case, self.want = case, tuple(want) + tuple(k for k in ("member_off", "grouped_partition") if k not in want)
        sz = sizes_of(case)
        self.g = {}
        for k in INPUTS:
            v = getattr(case, k)
            self.g[k] = Guarded("device", v.size, v.dtype, shifts.get(k, 0), v, name=k)
        for k in ALL:
            self.g[k] = Guarded("device", sz[k], dtype_of(k), shifts.get(k, 0), name=k)
        self.args = args_of(case, {k: g.ptr for k, g in self.g.items()}, self.want, flags, null_owned)
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        ctx.cooperative_round_device(self.args, stream)
        self.launches = ctx.last_launches()

    def outputs(self):
        return [self.g[k].values() for k in ALL]

    def check_contract(self, what=""):
        for k in INPUTS:
            self.g[k].check_unchanged(what)
        for k in ALL:
            self.g[k].check_guards(what)

    def check(self, exp, what=""):
        """Wanted outputs equal the restatement, the others still hold SENTINEL, nothing outside the arrays was written."""
        for k, g, e in zip(ALL, self.outputs(), exp):
            if k in self.want:
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
            else:
                assert (np.asarray(g) == SENTINEL).all(), "%s was not asked for %s" % (k, what)
        self.check_contract(what)


def both(ctx, torch, c, what="", small=None, **kw):
    """The case as it comes and with LA_COOP_FORCE_TABLE: both equal the restatement (hence each other).  small: whether the plain
    run must be the one-workgroup form (None: by the limits)."""
    stream = _stream(torch)
    exp = expect(c)
    plain = Round(ctx, c, stream, 0, **kw)
    forced = Round(ctx, c, stream, N.LA_COOP_FORCE_TABLE, **kw)
    ctx.sync(stream)
    plain.check(exp, what + " (as it comes)")
    forced.check(exp, what + " (table forced)")
    for k, a, b in zip(ALL, plain.outputs(), forced.outputs()):
        np.testing.assert_array_equal(a, b, err_msg="%s differs between the forms %s" % (k, what))
    within = c.n <= LE and c.n_owned <= LO and c.m <= LM and c.t <= LT
    assert within == (small if small is not None else within), (c.n, c.n_owned, c.m, c.t)
    if within:
        assert plain.launches == 1, "one launch within the limits %s" % what
    else:
        assert plain.launches > 1, what
    return exp, plain, forced


def split(n, parts=4):
    """n entries over five topics, the second empty, the fifth (it has no consumers in a synthetic case) not."""
    base = [n // parts] * parts
    base[0] += n - sum(base)
    return [base[0], 0] + base[1:] if n >= parts else [n]


# ---- smallest shapes -------------------------------------------------------------------------------------------------------------
def test_one_topic_one_partition_one_member(ctx, torch_dev):
    exp, plain, _ = both(ctx, torch_dev[0], synthetic(1, [1], 1, owned_frac=1.0), "T = P = M = 1")
    assert exp[7].tolist() == [1, 0, 0, 0, 0, 0] and exp[8].tolist() == [0, 1]


def test_nothing_owned_with_null_owned_pointers(ctx, torch_dev):
    c = synthetic(2, [40, 0, 7, 64, 30], 6, owned_frac=0.0)
    assert c.n_owned == 0
    for null_owned in (True, False):
        exp, plain, _ = both(ctx, torch_dev[0], c, "n_owned = 0, NULL %s" % null_owned, null_owned=null_owned)
        np.testing.assert_array_equal(plain.outputs()[1], c.rank)
        assert exp[7].tolist() == [0, int((c.rank >= 0).sum()), 0, 0, 0, 0]


def test_no_entries_but_owned_ones_all_stale_and_no_topics(ctx, torch_dev):
    e = np.empty(0, np.int32)
    for part_off in (np.zeros(5, np.int64), np.zeros(1, np.int64)):              # N == 0 with topics, and T == 0
        t = part_off.size - 1
        claims = [(0, -1, 4), (2, -1, 4)] + ([(1, 2, 9), (3, 0, 0)] if t else [])
        c = CoopCase(part_off, e, e, 4, *owned_arrays(4, claims, 1, 1))
        exp, plain, _ = both(ctx, torch_dev[0], c, "T = %d, N = 0" % t)
        assert exp[7].tolist() == [0, 0, 0, 0, len(claims), 0] and not exp[8].any()
        both(ctx, torch_dev[0], CoopCase(part_off, e, e, 4, *owned_arrays(4, [])), "T = %d, nothing at all" % t, null_owned=True)


def test_every_output_is_optional_and_the_lists_need_no_coop_rank(ctx, torch_dev):
    torch = torch_dev[0]
    stream = _stream(torch)
    c = synthetic(3, [200, 31, 300, 0, 77], 5, n_stale=10, n_unmapped=3, head=2, tail=2)
    exp = expect(c)
    optional = OUTPUTS + ("grouped_topic",)
    wants = [()] + [(k,) for k in optional] + [tuple(x for x in optional if x != k) for k in optional]
    runs = [(w, f, Round(ctx, c, stream, f, want=w)) for w in wants for f in (0, N.LA_COOP_FORCE_TABLE)]
    ctx.sync(stream)
    for w, f, r in runs:
        assert (r.launches == 1) == (f == 0)
        r.check(exp, "outputs %s, flags %d" % (w, f))
    assert (exp[1] == -1).any() and (exp[1] != c.rank).any(), "the lists without coop_rank are not those of the target"


# ---- chunk and stride edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_chunks_of_64_entries_and_the_workgroup_stride(ctx, torch_dev, n):
    c = synthetic(10 + n, split(n), 40, ids="full", n_stale=9, n_unmapped=3, head=3, tail=2)
    c.rank[c.rank == 5] = 6                                          # (the owned lists do not depend on the target's ranks)
    assert c.n == n and c.n_owned <= LO
    exp, _, _ = both(ctx, torch_dev[0], c, "N = %d" % n, small=True)
    lists = np.diff(exp[8])
    assert (lists == 0).any() and (lists > 0).any(), "members that receive nothing"
    assert (c.rank[c.part_off[4]:] == -1).all() and c.part_off[5] > c.part_off[4], "a topic without consumers"
    assert exp[8][0] > 0 and c.owned_off[0] == 3 and c.n_owned - c.owned_off[-1] == 2


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def test_hostile_ids_unmapped_topics_and_all_five_states(ctx, torch_dev):
    c = synthetic(20, [12] + np.random.default_rng(20).integers(0, 41, 59).tolist(), 7, ids="full", n_stale=30, n_unmapped=9, head=2, tail=3)
    assert c.part_off[1] >= 3 and {0, -1, I32.min} <= set(c.pid[: int(c.part_off[1])].tolist()), "(topic 0, id 0) is an entry"
    assert (c.owned_topic[c.owned_off[0]:c.owned_off[-1]] == -1).any()
    # (topic 0, id 0) is claimed: its key must not read as an empty slot
    at = int(np.flatnonzero(c.pid[: int(c.part_off[1])] == 0)[0])
    claims = [(int(r), int(t), int(i)) for r in range(c.m) for t, i in
              zip(c.owned_topic[c.owned_off[r]:c.owned_off[r + 1]], c.owned_pid[c.owned_off[r]:c.owned_off[r + 1]])
              if (t, i) != (0, 0)] + [(3, 0, 0)]
    c = CoopCase(c.part_off, c.pid, c.rank, c.m, *owned_arrays(c.m, claims, 2, 3, 21))
    exp, _, _ = both(ctx, torch_dev[0], c, "full ids", small=True)
    assert exp[0][at] == 3
    idle = int(((c.rank == -1) & (exp[0] == -1)).sum())
    assert (exp[7][:5] > 0).all() and idle > 0, "kept, fresh, withheld, dropped, stale and idle all occur"


@pytest.mark.parametrize("extra", [0, 1], ids=["n_owned = 2^9", "n_owned = 2^9 + 1"])
def test_table_sizing_at_a_power_of_two(ctx, torch_dev, extra):
    c = synthetic(22, [200, 300, 12], 7, ids="full", owned_frac=1.0, n_stale=extra)
    assert c.n_owned == 512 + extra and c.owned_off[0] == 0 and c.owned_off[-1] == c.n_owned
    exp, _, _ = both(ctx, torch_dev[0], c, "every slot of the owned arrays is a live claim", small=True)
    assert exp[7][4] == extra


def test_ids_that_are_multiples_of_2_pow_20_over_many_topics(ctx, torch_dev):
    rng = np.random.default_rng(23)
    t, p, m = 80, 24, 9
    part_off = np.arange(t + 1, dtype=np.int64) * p
    pid = np.concatenate([(rng.permutation(p).astype(np.int64) - p // 2) << 20 for _ in range(t)]).astype(np.int32)
    rank = rng.integers(-1, m, t * p).astype(np.int32)
    claims = claims_from(24, part_off, pid, m, owned_frac=0.9, n_stale=100)
    c = CoopCase(part_off, pid, rank, m, *owned_arrays(m, claims, 0, 0, 25))
    assert c.n == 1920 and 1024 < c.n_owned <= LO and (c.pid.astype(np.int64) % (1 << 20) == 0).all()
    exp, _, _ = both(ctx, torch_dev[0], c, "equal low key bits", small=True)
    assert (exp[7][:3] > 0).all() and exp[7][4] >= 100


# ---- limits ----------------------------------------------------------------------------------------------------------------------
def limit_case(which, over):
    if which == "N":
        return synthetic(30, split(LE + over, 8), 5, owned_frac=0.5, head=1)
    if which == "n_owned":
        c = synthetic(31, [700, 0, 800], 6, ids="negative", owned_frac=1.0, n_stale=LO + over - 1500)
        assert c.n_owned == LO + over
        return c
    if which == "M":
        return synthetic(32, [300, 0, 299, 1], LM + over, owned_frac=0.7, n_unmapped=3, tail=2)
    assert which == "T"
    sizes = [(1 if t % 3 == 0 else 0) for t in range(LT + over)]     # two empty topics behind every topic of one partition
    sizes[-1] = 0
    return synthetic(33, sizes, 4, owned_frac=0.8, n_stale=7)


@pytest.mark.parametrize("over", [0, 1], ids=["at the limit", "one above"])
@pytest.mark.parametrize("which", ["N", "n_owned", "M", "T"])
def test_each_limit_and_one_above_it(ctx, torch_dev, which, over):
    c = limit_case(which, over)
    assert {"N": c.n, "n_owned": c.n_owned, "M": c.m, "T": c.t}[which] == {"N": LE, "n_owned": LO, "M": LM, "T": LT}[which] + over
    exp, plain, forced = both(ctx, torch_dev[0], c, "%s = limit + %d" % (which, over), small=(over == 0))
    assert forced.launches > 1
    if which == "M":
        assert exp[2][c.m - 1] + exp[3][c.m - 1] + exp[4][c.m - 1] > 0, "the last member's counters"


# ---- hostile input ---------------------------------------------------------------------------------------------------------------
BROKEN = {"duplicate claim, one member": N.LA_EINVAL, "duplicate claim, two members": N.LA_EINVAL, "owned topic T": N.LA_EINVAL,
          "owned topic -2": N.LA_EINVAL, "target rank M": N.LA_EINVAL, "target rank -2": N.LA_EINVAL,
          "descending owned offsets": N.LA_ESHAPE, "owned offset beyond n_owned": N.LA_ESHAPE, "negative owned offset": N.LA_ESHAPE,
          "part_off descends": N.LA_ESHAPE, "part_off ends short of N": N.LA_ESHAPE}
# (an owned offset that leaves the slices makes the call look at the entries next to them: those two cases carry no poison there)
BARE = ("owned offset beyond n_owned", "negative owned offset")


@pytest.mark.parametrize("bad", list(BROKEN))
def test_broken_input_is_reported_alike_by_both_forms_and_never_stored_through(ctx, torch_dev, bad):
    torch = torch_dev[0]
    stream = _stream(torch)
    poison = 0 if bad in BARE else 2
    c = synthetic(11, [20, 30, 20], 5, owned_frac=1.0, n_unmapped=2, head=poison, tail=poison)
    b = break_case(c, bad)
    with pytest.raises(ValueError):
        expect(b)                                                    # the restatement refuses the same input
    # what la_cooperative_adjust_device says of it
    g = {k: Guarded("device", getattr(b, k).size, getattr(b, k).dtype, 0, getattr(b, k), name=k) for k in INPUTS}
    g["summary"] = Guarded("device", 6, np.int64, 0, name="summary")
    a = args_of(b, {**{k: v.ptr for k, v in g.items()}, "member_off": None, "grouped_partition": None}, ("summary",)).adjust
    torch.cuda.synchronize()
    ctx.cooperative_adjust_device(a, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == BROKEN[bad]
    for flags in (0, N.LA_COOP_FORCE_TABLE):
        r = Round(ctx, b, stream, flags)
        assert (r.launches == 1) == (flags == 0)
        with pytest.raises(N.LagAssignError) as ei:
            ctx.sync(stream)
        assert ei.value.code == BROKEN[bad], "flags %d" % flags
        r.check_contract("%s, flags %d" % (bad, flags))
    both(ctx, torch, c, "after " + bad)                              # the next calls on the same context are ordinary ones


# ---- chained on the device -------------------------------------------------------------------------------------------------------
def test_three_rounds_chained_on_one_stream_one_launch_each(ctx, torch_dev):
    """The first rebalance (nobody owns anything) and its lists; rebalance B -- other ranks, the last member gone, one topic
    without consumers -- against A's lists as they lie on the device; the convergence round against B's lists.  One stream,
    one sync."""
    torch, dev = torch_dev
    rng = np.random.default_rng(40)
    m, mb = 7, 6
    sizes = rng.integers(1, 120, 20).tolist()
    ca = synthetic(40, sizes, m, owned_frac=0.0)
    t, n = ca.t, ca.n
    assert n <= LE and (ca.rank == m - 1).any()
    topic = topics_of(ca.part_off)
    t_lost = next(x for x in range(t) if sizes[x] > 20 and (ca.rank[topic == x] >= 0).any())
    b_rank = np.where((topic % 5 == 4) | (topic == t_lost), -1, rng.integers(0, mb, n)).astype(np.int32)

    made = []

    def dev_buf(size, dtype, values=None):
        made.append(Guarded("device", size, dtype, (0, 1, 3)[len(made) % 3], values, name="buffer %d" % len(made)))
        return made[-1]

    up = lambda x: dev_buf(x.size, x.dtype, x)
    i32 = lambda: dev_buf(n, np.int32)
    i64 = lambda k: dev_buf(k, np.int64)
    d = dict(part_off=up(ca.part_off), pid=up(ca.pid), a_rank=up(ca.rank), b_rank=up(b_rank))
    inputs = list(made)
    lists = {k: (i64((m if k == "a" else mb) + 1), i32(), i32()) for k in "abc"}
    summ = {k: i64(6) for k in "abc"}
    coop_b, release_b = i32(), i64(mb)

    def call(rank, members, owned, out, summary, n_owned, coop=None, release=None):
        r = N.CoopRoundArgs()
        a = r.adjust
        a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, members, n_owned
        a.d_part_off, a.d_out_partition, a.d_out_member_rank = d["part_off"].ptr, d["pid"].ptr, rank.ptr
        if owned is not None:
            a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = (x.ptr for x in owned)
        a.d_summary = summary.ptr
        a.d_coop_member_rank = coop.ptr if coop is not None else None
        a.d_member_release = release.ptr if release is not None else None
        r.member_off, r.grouped_topic, r.grouped_partition = (x.ptr for x in out)
        ctx.cooperative_round_device(r, s)
        return ctx.last_launches()

    torch.cuda.synchronize()                                         # the uploads ran on torch's stream
    s = _stream(torch)
    launches = [call(d["a_rank"], m, None, lists["a"], summ["a"], 0),
                # A's lists as they lie there: the first M offsets are those of the members that stayed, the one that left owns the tail
                call(d["b_rank"], mb, lists["a"], lists["b"], summ["b"], n, coop_b, release_b),
                call(d["b_rank"], mb, lists["b"], lists["c"], summ["c"], n)]
    ctx.sync(s)                                                      # the first wait
    assert launches == [1, 1, 1]

    host = lambda x: x.values()
    for g in made:
        g.check_unchanged("chained") if g in inputs else g.check_guards("chained")
    ea = sharding.cooperative_round_numpy(ca.part_off, ca.pid, ca.rank, m, None, None, None)
    eb = sharding.cooperative_round_numpy(ca.part_off, ca.pid, b_rank, mb, ea[8][:m], ea[9], ea[10])
    ec = sharding.cooperative_round_numpy(ca.part_off, ca.pid, b_rank, mb, eb[8], eb[9], eb[10])
    for k, e in zip("abc", (ea, eb, ec)):
        for got, want in zip(lists[k], e[8:]):
            np.testing.assert_array_equal(host(got), want, err_msg="lists of round " + k)
        np.testing.assert_array_equal(host(summ[k]), e[7], err_msg="summary of round " + k)
    np.testing.assert_array_equal(host(coop_b), eb[1])
    np.testing.assert_array_equal(host(release_b), eb[5])
    assert (eb[7][:4] > 0).all() and eb[7][4] == 0 and eb[7][5] == 1
    assert eb[6][t_lost] == 0 and (eb[1][topic == t_lost] == -1).all()
    s3 = host(summ["c"])
    assert s3[2] == 0 and s3[3] == 0 and s3[4] == 0 and s3[5] == 0, "the second round withholds nothing and asks for no follow-up"
    live = b_rank >= 0
    np.testing.assert_array_equal(ec[1][live], b_rank[live])


# ---- contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["aligned", "odd", "three"])
def test_buffer_contract_at_every_element_shift(ctx, torch_dev, pattern):
    c = synthetic(50, [37, 1, 300, 0, 64, 700], 7, ids="full", n_stale=25, n_unmapped=6, head=3, tail=5)
    both(ctx, torch_dev[0], c, pattern, shifts=shifts_for(pattern, INPUTS + ALL))


def test_results_kept_for_group_last_by_member_survive_a_one_workgroup_round(torch_dev):
    torch, _ = torch_dev
    c = N.Context(0)
    try:
        w = _workload(17, 0.05)
        m = int(w.cons_rank.max()) + 1
        first, topic, pid, e_tot, _ = _grouped_expect(w, m)
        _, _, tot = c.assign_batch(w.part_off, w.partition_id, w.begin, w.end, w.committed, N.LA_RESET_EARLIEST, w.cons_off,
                                   w.cons_rank, keep_on_device=True)
        np.testing.assert_array_equal(tot, e_tot)
        stream = _stream(torch)
        case = synthetic(18, [600, 1000], 8, n_stale=100)            # unrelated device arrays
        r = Round(c, case, stream)
        c.sync(stream)
        assert r.launches == 1
        r.check(expect(case), "unrelated arrays")
        off, g_t, g_p = c.group_last_by_member(w.n_partitions, m)
        np.testing.assert_array_equal(off, first)
        np.testing.assert_array_equal(g_t, topic)
        np.testing.assert_array_equal(g_p, pid)
    finally:
        c.close()


def test_the_entry_refuses_bad_arguments_enqueues_nothing_and_leaves_the_current_device_alone(ctx, torch_dev):
    torch = torch_dev[0]
    lib, stream = N.load(), ctypes.c_void_p(_stream(torch))
    c = synthetic(60, [90, 0, 45], 6, n_stale=4)
    exp = expect(c)
    r = Round(ctx, c, _stream(torch))
    ctx.sync(_stream(torch))
    before = torch.cuda.current_device()
    size = ctypes.sizeof(N.CoopRoundArgs)

    def variant(**kw):
        v = N.CoopRoundArgs()
        ctypes.memmove(ctypes.byref(v), ctypes.byref(r.args), size)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    for dev_call in (True, False):
        fn = (lambda h, a: lib.la_cooperative_round_device(h, a, stream)) if dev_call else lib.la_cooperative_round
        assert fn(None, ctypes.byref(r.args)) == N.LA_EINVAL
        assert fn(ctx._h, None) == N.LA_EINVAL
        for v in (variant(struct_size=size - 8), variant(flags=2), variant(flags=N.LA_COOP_FORCE_TABLE | 4), variant(member_off=None),
                  variant(grouped_partition=None)):
            assert fn(ctx._h, ctypes.byref(v)) == N.LA_EINVAL
            assert ctx.last_launches() == 0
    assert torch.cuda.current_device() == before
    ctx.sync(_stream(torch))                                         # nothing was enqueued, nothing is pending
    r.check(exp, "after the refused calls")


# ---- la_cooperative_round: host buffers --------------------------------------------------------------------------------------------
HOST_SIZES = {"one entry": lambda: synthetic(70, [1], 1, owned_frac=1.0),
              "300 ragged entries": lambda: synthetic(71, np.random.default_rng(71).integers(0, 9, 75).tolist(), 7, ids="full",
                                                      n_stale=30, n_unmapped=9, head=2, tail=3),
              "over the limits": lambda: synthetic(72, [1000, 0, 900, 700], 11, ids="negative", n_stale=50, n_unmapped=5, head=1, tail=1)}


@pytest.mark.parametrize("name", list(HOST_SIZES))
def test_host_entry_on_pageable_offset_views(ctx, torch_dev, name):
    lib = N.load()
    c = HOST_SIZES[name]()
    if name == "over the limits":
        assert c.n > LE
    exp = expect(c)
    results = []
    for flags in (0, N.LA_COOP_FORCE_TABLE):
        shifts = shifts_for("mixed", INPUTS + ALL)
        g = {k: Guarded("numpy", getattr(c, k).size, getattr(c, k).dtype, shifts[k], getattr(c, k), name=k) for k in INPUTS}
        g.update({k: Guarded("numpy", sizes_of(c)[k], dtype_of(k), shifts[k], name=k) for k in ALL})
        a = args_of(c, {k: v.ptr for k, v in g.items()}, ALL, flags)
        assert lib.la_cooperative_round(ctx._h, ctypes.byref(a)) == N.LA_OK, ctx._lib.la_last_error(ctx._h)
        assert (ctx.last_launches() == 1) == (flags == 0 and name != "over the limits")
        for k, e in zip(ALL, exp):
            np.testing.assert_array_equal(g[k].array, e, err_msg="%s, %s, flags %d" % (k, name, flags))
            g[k].check_guards(name)
        for k in INPUTS:
            g[k].check_unchanged(name)
        results.append([g[k].array.copy() for k in ALL])
    for k, x, y in zip(ALL, *results):
        np.testing.assert_array_equal(x, y, err_msg=k)
    # the binding: numpy in, a named tuple out
    for force in (False, True):
        got = ctx.cooperative_round(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid, force_table=force)
        assert got._fields[8:] == LISTS and len(got) == len(exp)
        for k, x, e in zip(ALL, got, exp):
            np.testing.assert_array_equal(x, e, err_msg="%s, %s, force_table %s" % (k, name, force))


def test_host_entry_first_rebalance_and_optional_outputs(ctx, torch_dev):
    c = synthetic(73, [40, 0, 7, 64], 6, owned_frac=0.0)
    exp = expect(c)
    got = ctx.cooperative_round(c.part_off, c.pid, c.rank, c.m, None, None, None)
    for k, x, e in zip(ALL, got, exp):
        np.testing.assert_array_equal(x, e, err_msg=k)
    lib = N.load()
    c = HOST_SIZES["300 ragged entries"]()
    exp = expect(c)
    for flags in (0, N.LA_COOP_FORCE_TABLE):
        g = {k: Guarded("numpy", getattr(c, k).size, getattr(c, k).dtype, 1, getattr(c, k), name=k) for k in INPUTS}
        g.update({k: Guarded("numpy", sizes_of(c)[k], dtype_of(k), 3, name=k) for k in ALL})
        a = args_of(c, {k: v.ptr for k, v in g.items()}, ("release",), flags)      # the lists without coop_rank or topics
        assert lib.la_cooperative_round(ctx._h, ctypes.byref(a)) == N.LA_OK
        for k, e in zip(ALL, exp):
            if k in ("release", "member_off", "grouped_partition"):
                np.testing.assert_array_equal(g[k].array, e, err_msg=k)
            else:
                assert (g[k].array == SENTINEL).all(), k
            g[k].check_guards()


@pytest.mark.parametrize("bad", ["duplicate claim, two members", "target rank M", "descending owned offsets", "part_off descends"])
def test_host_entry_returns_the_error_itself(ctx, torch_dev, bad):
    c = synthetic(11, [20, 30, 20], 5, owned_frac=1.0, n_unmapped=2, head=2, tail=2)
    b = break_case(c, bad)
    for force in (False, True):
        with pytest.raises(N.LagAssignError) as ei:
            ctx.cooperative_round(b.part_off, b.pid, b.rank, b.m, b.owned_off, b.owned_topic, b.owned_pid, force_table=force)
        assert ei.value.code == BROKEN[bad]
        ctx.sync(ctx.stream)                                         # the call took its error with it
        got = ctx.cooperative_round(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid, force_table=force)
        for k, x, e in zip(ALL, got, expect(c)):
            np.testing.assert_array_equal(x, e, err_msg="%s after %s" % (k, bad))


def test_on_a_two_shard_context_both_calls_run_on_shard_zero(torch_dev):
    c2 = N.Context([0, 0])
    try:
        c = synthetic(61, [90, 0, 300, 45, 7], 6, ids="full", n_stale=40, n_unmapped=8, head=2, tail=2)
        exp = expect(c)
        got = c2.cooperative_round(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
        for k, x, e in zip(ALL, got, exp):
            np.testing.assert_array_equal(x, e, err_msg=k)
        stream = c2.shard_stream(0)
        torch_dev[0].cuda.synchronize()
        r = Round(c2, c, stream)
        c2.sync(stream, shard=0)
        r.check(exp, "shard 0 of two")
        Round(c2, break_case(c, "target rank M"), stream)            # the error belongs to shard 0
        c2.sync(c2.shard_stream(1), shard=1)
        with pytest.raises(N.LagAssignError) as ei:
            c2.sync(stream, shard=0)
        assert ei.value.code == N.LA_EINVAL
    finally:
        c2.close()
