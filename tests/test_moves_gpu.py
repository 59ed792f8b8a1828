"""la_assignment_moves_device[_on] on the GPU: the previous owner of every entry of an assignment, moved entries per topic, gained
and lost per member, the moved total.  The yardstick is sharding.assignment_moves_numpy (tests/test_moves_cpu.py holds that
restatement against a naive dict join), applied to the ORACLE's two assignments where the test runs the assign calls, and to
synthetic assignments over a valid id layout elsewhere.  Every comparison is bit for bit; outputs hold SENTINEL before a call."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

from gpu_helpers import SENTINEL, Guarded, _batch_of, _grouped_expect, _workload, shifts_for

pytestmark = pytest.mark.gpu

L = N.MOVES_LDS_MAX_PARTITIONS          # up to here a topic is joined in LDS, beyond it in a table in device memory
B = N.MOVES_LDS_MAX_MEMBERS             # up to here gained / lost are LDS bins, beyond it global atomics
I32 = np.iinfo(np.int32)
OUTPUTS = ("prev_owner", "topic_moved", "gained", "lost", "moved")
INPUTS = ("part_off", "cur_pid", "cur_rank", "prev_pid", "prev_rank", "rank_map")


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Two assignments over one layout, on the host."""

    def __init__(self, part_off, cur_pid, cur_rank, prev_pid, prev_rank, m, rank_map=None, hint=None):
        self.part_off = np.ascontiguousarray(part_off, np.int64)
        self.cur_pid, self.cur_rank = np.ascontiguousarray(cur_pid, np.int32), np.ascontiguousarray(cur_rank, np.int32)
        self.prev_pid, self.prev_rank = np.ascontiguousarray(prev_pid, np.int32), np.ascontiguousarray(prev_rank, np.int32)
        self.m = int(m)
        self.rank_map = None if rank_map is None else np.ascontiguousarray(rank_map, np.int32)
        self.t, self.n = self.part_off.size - 1, int(self.part_off[-1])
        sizes = np.diff(self.part_off)
        self.hint = int(sizes.max() if sizes.size else 0) if hint is None else int(hint)

    def expect(self):
        return sharding.assignment_moves_numpy(self.part_off, self.cur_pid, self.cur_rank, self.prev_pid, self.prev_rank, self.m,
                                               self.rank_map)

    def sizes(self):
        return {"part_off": self.t + 1, "cur_pid": self.n, "cur_rank": self.n, "prev_pid": self.n, "prev_rank": self.n,
                "rank_map": 0 if self.rank_map is None else self.rank_map.size,
                "prev_owner": self.n, "topic_moved": self.t, "gained": self.m, "lost": self.m, "moved": 1}


def _ids(rng, kind, p, first):
    if kind == "shuffled":
        return rng.permutation(p)
    if kind == "full":                                              # any int32, the corners in the first topic
        ids = set([I32.min, -1, 0, I32.max][: p] if first else [])
        while len(ids) < p:
            ids.update(rng.integers(I32.min, I32.max, p - len(ids), endpoint=True).tolist())
        return rng.permutation(np.array(sorted(ids), np.int64))
    step = {"4096": 4096, "2^20": 1 << 20}[kind]                     # strided: long probe chains under a masking hash
    return rng.permutation(p) * step


def synthetic(seed, sizes, m, ids="shuffled", m_prev=None, rank_map=None, hint=None):
    """Distinct ids per topic, each side in an order of its own, uniformly random ranks (-1 included; one topic in four had no
    consumers before, one in five has none now)."""
    rng = np.random.default_rng(seed)
    part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cur_pid, prev_pid, cur_rank, prev_rank = [], [], [], []
    for t, p in enumerate(sizes):
        base = _ids(rng, ids, p, t == 0)
        cur_pid.append(base[rng.permutation(p)])
        prev_pid.append(base[rng.permutation(p)])
        cur_rank.append(np.full(p, -1) if t % 5 == 4 else rng.integers(-1, m, p))
        prev_rank.append(np.full(p, -1) if t % 4 == 3 else rng.integers(-1, m_prev or m, p))
    cat = lambda xs: np.concatenate(xs + [np.empty(0, np.int64)])
    c = Case(part_off, cat(cur_pid), cat(cur_rank), cat(prev_pid), cat(prev_rank), m, rank_map, hint)
    if c.n > 3:
        c.cur_rank[:2] = m - 1                                      # the last bin is used
        c.prev_rank[-2:] = (m_prev or m) - 1
    return c


def from_oracle(w, seed):
    """The oracle's assignment of `w` (previous) and of the same layout with every lag redrawn (current)."""
    rng = np.random.default_rng(seed)
    prev_pid, prev_rank, _ = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    lag2 = rng.integers(0, 1 << 40, w.n_partitions).astype(np.int64)
    cur_pid, cur_rank, _ = oracle.assign_flat(w.part_off, w.partition_id, lag2, w.cons_off, w.cons_rank)
    m = (int(w.cons_rank.max()) + 1 if w.cons_rank.size else 0) + 3
    return Case(w.part_off, cur_pid, cur_rank, prev_pid, prev_rank, m), lag2


class Run:
    """One call: every array a Guarded device buffer (4 KiB guard bands, element shift per array)."""

    def __init__(self, ctx, case, stream, shifts=None, want=OUTPUTS, use_h=True, shard=0, hint=None):
        shifts = shifts or {}
        sz = case.sizes()
        self.case, self.want = case, want
        self.g = {}
        for k in INPUTS:
            v = getattr(case, k)
            if v is None:
                continue
            self.g[k] = Guarded("device", sz[k], v.dtype, shifts.get(k, 0), v, name=k)
        for k in OUTPUTS:
            self.g[k] = Guarded("device", sz[k], np.int32 if k == "prev_owner" else np.int64, shifts.get(k, 0), name=k)
        a = N.MovesArgs()
        a.n_topics, a.n_partitions = case.t, case.n
        a.max_partitions_per_topic = case.hint if hint is None else hint
        a.d_part_off = self.g["part_off"].ptr
        self.h_part_off = case.part_off                              # kept alive
        a.h_part_off = self.h_part_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if use_h else None
        a.d_out_partition, a.d_out_member_rank = self.g["cur_pid"].ptr, self.g["cur_rank"].ptr
        a.d_prev_partition, a.d_prev_member_rank = self.g["prev_pid"].ptr, self.g["prev_rank"].ptr
        a.n_members = case.m
        if case.rank_map is not None:
            a.n_prev_members, a.d_prev_rank_map = case.rank_map.size, self.g["rank_map"].ptr
        for k in want:
            setattr(a, "d_" + {"gained": "member_gained", "lost": "member_lost"}.get(k, k), self.g[k].ptr)
        self.args = a
        import torch
        torch.cuda.synchronize()                                     # the uploads ran on torch's stream; `stream` may be another
        ctx.assignment_moves_device(a, stream, shard=shard)
        self.launches = ctx.last_launches()

    def outputs(self):
        v = [self.g[k].values() for k in OUTPUTS]
        return v[0], v[1], v[2], v[3], int(v[4][0])

    def check_contract(self, what=""):
        for k in INPUTS:
            if k in self.g:
                self.g[k].check_unchanged(what)
        for k in OUTPUTS:
            self.g[k].check_guards(what)

    def check(self, exp=None, what=""):
        """Wanted outputs equal the restatement, the others still hold SENTINEL, nothing outside the arrays was written."""
        exp = self.case.expect() if exp is None else exp
        got = self.outputs()
        for k, g, e in zip(OUTPUTS, got, exp):
            if k in self.want:
                np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))
            else:
                assert (np.asarray(g) == SENTINEL).all(), "%s was not asked for %s" % (k, what)
        self.check_contract(what)


def _same_moves(got, exp, what=""):
    for k, g, e in zip(OUTPUTS, got, exp):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, what))


# ---- behind two assign calls on one stream -----------------------------------------------------------------------------------
E2E = {
    "ragged": lambda: synth.ragged(21, 400, 300, 40),
    "topics without consumers": lambda: _batch_of([(100, 0), (50, 4), (0, 3), (900, 0), (256, 32), (7, 0)], 5),
    "N = 0": lambda: _batch_of([(0, 3), (0, 2), (0, 0)], 6),
}


@pytest.mark.parametrize("case", list(E2E))
def test_end_to_end_behind_two_assign_calls_on_one_stream(ctx, torch_dev, case):
    torch, _ = torch_dev
    w = E2E[case]()
    c, lag2 = from_oracle(w, 3)
    exp = c.expect()
    dev = torch.device("cuda", 0)

    def up(a):
        a = np.ascontiguousarray(a)
        t = torch.zeros(max(a.size, 1), dtype=getattr(torch, a.dtype.name), device=dev)
        if a.size:
            t[: a.size] = torch.from_numpy(a)
        return t

    d = {k: up(getattr(w, k)) for k in ("part_off", "partition_id", "lag", "cons_off", "cons_rank")}
    d["lag2"] = up(lag2)
    n, k, t, m = w.n_partitions, w.cons_rank.size, w.n_topics, c.m
    res = {name: torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device=dev) for name in ("prev_pid", "prev_rank", "cur_pid", "cur_rank", "owner")}
    outs = {"topic_moved": torch.full((max(t, 1),), SENTINEL, dtype=torch.int64, device=dev),
            "gained": torch.full((m,), SENTINEL, dtype=torch.int64, device=dev),
            "lost": torch.full((m,), SENTINEL, dtype=torch.int64, device=dev),
            "moved": torch.full((1,), SENTINEL, dtype=torch.int64, device=dev)}
    po, co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)
    h_po = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    batches = []
    for lag, pid, rank in ((d["lag"], res["prev_pid"], res["prev_rank"]), (d["lag2"], res["cur_pid"], res["cur_rank"])):
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = t, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
        b.d_part_off, b.d_partition_id, b.d_lag = d["part_off"].data_ptr(), d["partition_id"].data_ptr(), lag.data_ptr()
        b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = pid.data_ptr(), rank.data_ptr(), None
        b.h_part_off, b.h_cons_off = h_po, co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        batches.append(b)
    a = N.MovesArgs()
    a.n_topics, a.n_partitions, a.max_partitions_per_topic = t, n, w.max_partitions
    a.d_part_off, a.h_part_off = d["part_off"].data_ptr(), h_po
    a.d_out_partition, a.d_out_member_rank = res["cur_pid"].data_ptr(), res["cur_rank"].data_ptr()
    a.d_prev_partition, a.d_prev_member_rank = res["prev_pid"].data_ptr(), res["prev_rank"].data_ptr()
    a.n_members = m
    a.d_prev_owner, a.d_topic_moved = res["owner"].data_ptr(), outs["topic_moved"].data_ptr()
    a.d_member_gained, a.d_member_lost, a.d_moved = outs["gained"].data_ptr(), outs["lost"].data_ptr(), outs["moved"].data_ptr()
    torch.cuda.synchronize()                                         # the uploads ran on torch's stream
    stream = _stream(torch)
    for b in batches:                                                # previous, current, the join: enqueued end to end
        ctx.assign_batch_device(b, stream)
    ctx.assignment_moves_device(a, stream)
    launches = ctx.last_launches()
    ctx.sync(stream)                                                 # the first wait
    got = (res["owner"].cpu().numpy()[:n], outs["topic_moved"].cpu().numpy()[:t], outs["gained"].cpu().numpy(),
           outs["lost"].cpu().numpy(), int(outs["moved"].cpu().numpy()[0]))
    _same_moves(got, exp, case)
    np.testing.assert_array_equal(res["cur_pid"].cpu().numpy()[:n], c.cur_pid)          # (the join read what the oracle says it read)
    np.testing.assert_array_equal(res["prev_rank"].cpu().numpy()[:n], c.prev_rank)
    assert launches == (1 if n else 0)
    if n:
        assert exp[4] > 0, "redrawn lags move something"


# ---- ids -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["shuffled", "full", "4096", "2^20"])
def test_any_int32_is_an_id(ctx, torch_dev, ids):
    rng = np.random.default_rng(4)
    sizes = rng.integers(1, 301, 64).tolist()
    sizes[0], sizes[1] = 300, 4
    c = synthetic(11, sizes, 40, ids=ids)
    if ids == "full":
        assert {I32.min, -1, 0, I32.max} <= set(c.cur_pid[:300].tolist())
    stream = _stream(torch_dev[0])
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    assert r.launches == 1
    r.check(what=ids)


# ---- topic sizes: both forms and the switch between them --------------------------------------------------------------------
def test_topic_sizes_up_to_the_lds_limit_are_one_launch(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = synthetic(2, [1, 2, 63, 64, 65, L - 1, L], 24, hint=L)
    for use_h in (False, True):
        r = Run(ctx, c, stream, use_h=use_h)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(what="sizes up to L, h_part_off %s" % use_h)


@pytest.mark.parametrize("m", [8, B + 1])
@pytest.mark.parametrize("sizes", [[L + 1], [L + 1, 300, 2 * L + 7, 0], [0, 2 * L, L + 1]], ids=["L+1", "mixed", "large only"])
def test_topics_beyond_the_lds_limit_go_through_the_table_in_device_memory(ctx, torch_dev, sizes, m):
    stream = _stream(torch_dev[0])
    c = synthetic(3, sizes, m, ids="full")
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    assert 2 <= r.launches <= 3
    r.check(what="sizes %s" % sizes)
    r = Run(ctx, c, stream)                                          # the table is cleared per call
    ctx.sync(stream)
    r.check(what="sizes %s, second call" % sizes)


def test_mixed_batch_of_oracle_assignments(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c, _ = from_oracle(_batch_of([(L + 1, 5), (300, 10), (2 * L + 7, 3), (0, 2)], 8), 5)
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    assert r.launches == 3
    r.check(what="mixed oracle batch")
    assert r.outputs()[4] > 0


# ---- member counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 64, B - 1, B, B + 1, 100000])
def test_member_counts_on_both_sides_of_the_bin_limit(ctx, torch_dev, m):
    stream = _stream(torch_dev[0])
    rng = np.random.default_rng(m)
    c = synthetic(m, rng.integers(1, 301, 60).tolist() + [2000], m)
    exp = c.expect()
    assert exp[4] > 0 or m == 1
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    assert r.launches == 1
    r.check(exp, "M = %d" % m)


# ---- rank map --------------------------------------------------------------------------------------------------------------
def test_identity_map_equals_no_map(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = synthetic(6, [200, 31, 300, 5, 77], 50)
    r0 = Run(ctx, c, stream)
    c.rank_map = np.arange(50, dtype=np.int32)
    r1 = Run(ctx, c, stream)
    ctx.sync(stream)
    r1.check(what="identity map")
    _same_moves(r1.outputs(), r0.outputs(), "identity map against NULL")


@pytest.mark.parametrize("sizes", [[200, 31, 300, 5, 77, 0, 128], [L + 9, 40]], ids=["lds", "global"])
def test_rank_map_with_members_gone_and_new_ranks_interleaved(ctx, torch_dev, sizes):
    stream = _stream(torch_dev[0])
    m_prev = 60
    rank_map = np.full(m_prev, -1, np.int32)
    stay = [r for r in range(m_prev) if r % 3 != 1]                  # a third of the members left
    rank_map[stay] = np.arange(len(stay), dtype=np.int32) * 2 + 1   # today's even ranks are members that joined
    m = 2 * len(stay) + 1
    c = synthetic(7, sizes, m, m_prev=m_prev, rank_map=rank_map)
    exp = c.expect()
    assert (exp[0][c.prev_rank >= 0] == -1).any() and not exp[3][::2].any()
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    r.check(exp, "rank map")


# ---- optional outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[200, 31, 300, 0, 77], [L + 1, 50]], ids=["lds", "global"])
def test_every_output_is_optional(ctx, torch_dev, sizes):
    stream = _stream(torch_dev[0])
    c = synthetic(8, sizes, 33)
    exp = c.expect()
    wants = [(k,) for k in OUTPUTS] + [tuple(x for x in OUTPUTS if x != k) for k in OUTPUTS]
    runs = [Run(ctx, c, stream, want=w) for w in wants]
    ctx.sync(stream)
    for w, r in zip(wants, runs):
        r.check(exp, "outputs %s" % (w,))
    with pytest.raises(N.LagAssignError) as ei:
        Run(ctx, c, stream, want=())
    assert ei.value.code == N.LA_EINVAL
    ctx.sync(stream)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def _broken(c, bad):
    """A copy of `c` with one entry of its middle topic broken."""
    b = Case(c.part_off, c.cur_pid.copy(), c.cur_rank.copy(), c.prev_pid.copy(), c.prev_rank.copy(), c.m,
             None if c.rank_map is None else c.rank_map.copy(), c.hint)
    i = int(c.part_off[1]) + 3
    if bad == "duplicate id, previous":
        b.prev_pid[i] = b.prev_pid[i + 1]
    elif bad == "duplicate id, current":
        b.cur_pid[i] = b.cur_pid[i + 1]
    elif bad == "foreign id":
        b.cur_pid[i] = 1 << 30
    elif bad == "current rank M":
        b.cur_rank[i] = c.m
    elif bad == "previous rank M":
        b.prev_rank[i] = c.m if c.rank_map is None else c.rank_map.size
    elif bad == "current rank -2":
        b.cur_rank[i] = -2
    elif bad == "previous rank -2":
        b.prev_rank[i] = -2
    elif bad == "map entry M":
        b.rank_map[int(b.prev_rank[i]) if b.prev_rank[i] >= 0 else 0] = c.m
        b.prev_rank[i] = max(int(b.prev_rank[i]), 0)
    else:
        raise ValueError(bad)
    return b


ERRORS = ["duplicate id, previous", "duplicate id, current", "foreign id", "current rank M", "previous rank M", "current rank -2",
          "previous rank -2", "map entry M"]


@pytest.mark.parametrize("m", [9, B + 1])
@pytest.mark.parametrize("bad", ERRORS)
def test_broken_input_is_reported_and_never_stored_through(ctx, torch_dev, bad, m):
    stream = _stream(torch_dev[0])
    rank_map = np.random.default_rng(1).permutation(m).astype(np.int32) if bad == "map entry M" else None
    c = synthetic(12, [20, 30, 20], m, rank_map=rank_map)
    b = _broken(c, bad)
    with pytest.raises(ValueError):
        b.expect()                                                   # the restatement refuses the same input
    r = Run(ctx, b, stream, shifts=shifts_for("mixed", INPUTS + OUTPUTS))
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_EINVAL and "la_assignment_moves_device" in str(ei.value)
    r.check_contract(bad)
    r = Run(ctx, c, stream, shifts=shifts_for("mixed", INPUTS + OUTPUTS))    # the next call on the same context is an ordinary one
    ctx.sync(stream)
    r.check(what="after " + bad)


@pytest.mark.parametrize("bad", ["duplicate id, previous", "duplicate id, current", "foreign id", "previous rank M", "current rank -2"])
def test_broken_input_in_the_global_form(ctx, torch_dev, bad):
    stream = _stream(torch_dev[0])
    c = synthetic(13, [10, L + 40, 25], 17)
    r = Run(ctx, _broken(c, bad), stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_EINVAL
    r.check_contract(bad)
    r = Run(ctx, c, stream)
    ctx.sync(stream)
    r.check(what="after " + bad)


def test_shape_errors(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = synthetic(14, [50, 120, 60, 0], 12, hint=100)
    r = Run(ctx, c, stream)
    with pytest.raises(N.LagAssignError) as ei:
        ctx.sync(stream)
    assert ei.value.code == N.LA_ESHAPE
    r.check_contract("a topic over the hint")
    got = r.outputs()
    lo, hi = int(c.part_off[1]), int(c.part_off[2])
    assert (got[0][lo:hi] == SENTINEL).all() and got[1][1] == SENTINEL          # nothing is written for that topic
    keep = np.r_[0:lo, hi:c.n]
    rest = Case(np.array([0, 50, 110, 110], np.int64), c.cur_pid[keep], c.cur_rank[keep], c.prev_pid[keep], c.prev_rank[keep], c.m)
    exp = rest.expect()
    np.testing.assert_array_equal(got[0][keep], exp[0])
    np.testing.assert_array_equal(got[1][[0, 2, 3]], exp[1])
    _same_moves(got[2:], exp[2:], "the other topics")
    # a hint beyond one workgroup's table needs the host's offsets
    with pytest.raises(N.LagAssignError) as ei:
        Run(ctx, c, stream, use_h=False, hint=L + 1)
    assert ei.value.code == N.LA_EINVAL and "h_part_off" in str(ei.value)
    r = Run(ctx, c, stream, hint=L + 1)                              # ... with them every topic is done by its real size
    ctx.sync(stream)
    r.check(what="large hint, small topics")
    assert r.launches == 1


def test_calls_without_entries_zero_the_outputs(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    e = np.empty(0, np.int32)
    for part_off in (np.zeros(1, np.int64), np.zeros(5, np.int64)):              # T == 0, and N == 0 with topics
        c = Case(part_off, e, e, e, e, 6)
        r = Run(ctx, c, stream)
        ctx.sync(stream)
        assert r.launches == 0
        r.check(what="T = %d, N = 0" % c.t)
        assert r.outputs()[4] == 0 and not r.outputs()[2].any()


# ---- buffer contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[37, 1, 300, 0, 64], [L + 3, 5]], ids=["lds", "global"])
@pytest.mark.parametrize("pattern", ["aligned", "odd", "three", "mixed"])
def test_buffer_contract_element_aligned_views_guards_and_untouched_inputs(ctx, torch_dev, pattern, sizes):
    stream = _stream(torch_dev[0])
    for m in (7, B + 2):
        c = synthetic(15, sizes, m, rank_map=np.random.default_rng(2).integers(-1, m, m + 4).astype(np.int32), m_prev=m + 4)
        r = Run(ctx, c, stream, shifts=shifts_for(pattern, INPUTS + OUTPUTS))
        ctx.sync(stream)
        r.check(what="%s, M = %d" % (pattern, m))


# ---- shards, kept results --------------------------------------------------------------------------------------------------
def test_on_shard_one_of_a_two_shard_context(torch_dev):
    c2 = N.Context([0, 0])
    try:
        stream = c2.shard_stream(1)
        torch_dev[0].cuda.synchronize()
        c = synthetic(16, [100, L + 1, 7], 20)
        r = Run(c2, c, stream, shard=1)
        c2.sync(stream, shard=1)
        r.check(what="shard 1")
        b = _broken(c, "foreign id")                                 # the error belongs to the shard that ran the call
        Run(c2, b, stream, shard=1)
        c2.sync(c2.shard_stream(0), shard=0)
        with pytest.raises(N.LagAssignError) as ei:
            c2.sync(stream, shard=1)
        assert ei.value.code == N.LA_EINVAL
        with pytest.raises(N.LagAssignError) as ei:
            Run(c2, c, stream, shard=2)
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
        case = synthetic(18, [2 * L + 1, 90, L + 5], 77)            # unrelated device arrays; the table is allocated here
        stream = _stream(torch)
        r = Run(c, case, stream)
        c.sync(stream)
        assert r.launches == 3
        r.check(what="unrelated arrays")
        off, g_t, g_p = c.group_last_by_member(w.n_partitions, m)
        np.testing.assert_array_equal(off, first)
        np.testing.assert_array_equal(g_t, topic)
        np.testing.assert_array_equal(g_p, pid)
    finally:
        c.close()
