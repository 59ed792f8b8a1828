"""The buffer contract of every entry point (include/lagassign.h): results only inside [0, N) / [0, K) -- guard bands of
GUARD_BYTES around every array stay as they were --, inputs never written, arrays that are only element-aligned, and nothing
written where the header says so.  Every case also checks the results against the oracle (round_form where the literal oracle
is too slow).  Shift patterns put inputs and outputs at element offsets 0, 1 and 3, independently of each other."""
import ctypes
import os

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle
from oracle.round_form import round_form
from gpu_helpers import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

DT = {"part_off": np.int64, "partition_id": np.int32, "lag": np.int64, "begin": np.int64, "end": np.int64, "committed": np.int64,
      "cons_off": np.int64, "cons_rank": np.int32, "h_part_off": np.int64, "h_cons_off": np.int64,
      "out_partition": np.int32, "out_member_rank": np.int32, "out_total_lag": np.int64}
FIELD = {"part_off": "d_part_off", "partition_id": "d_partition_id", "lag": "d_lag", "begin": "d_begin_off", "end": "d_end_off",
         "committed": "d_committed_off", "cons_off": "d_cons_off", "cons_rank": "d_cons_rank", "out_partition": "d_out_partition",
         "out_member_rank": "d_out_member_rank", "out_total_lag": "d_out_total_lag"}
PATTERNS = ("three", "mixed")


def _with_offsets(w, seed):
    """begin / end / committed for w's lags: ~10 % of the partitions without a committed offset (their `earliest` lag is end - begin,
    the drawn lag again; `latest` gives them 0).  No offset is negative when no lag is."""
    rng = np.random.default_rng(seed)
    n = w.n_partitions
    com = rng.integers(0, 1 << 20, n).astype(np.int64)
    none = rng.random(n) < 0.1
    with np.errstate(over="ignore"):
        end = com + w.lag
    w.begin, w.end, w.committed = np.where(none, com, np.int64(0)), end, np.where(none, np.int64(-1), com)
    return w


def _expect(w, lag, literal=True):
    f = oracle.assign_flat if literal else round_form
    return f(w.part_off, w.partition_id, lag, w.cons_off, w.cons_rank)


class DeviceCase:
    """One la_assign_batch_device call on guarded device arrays.  form: "lags", "latest" (d_begin_off NULL) or "earliest"."""

    def __init__(self, ctx, w, pattern="mixed", form="lags", flags=0, algo=N.LA_ALGO_AUTO, totals=True, results=True, hint=None,
                 bounds=None, wire=None):
        import torch
        self.w, self.form = w, form
        names = ["part_off", "partition_id"] + (["lag"] if form == "lags" else (["end", "committed"] if form == "latest" else
                                                                                ["begin", "end", "committed"])) + ["cons_off", "cons_rank"]
        outs = (["out_partition", "out_member_rank"] if results and wire is None else []) + (["out_total_lag"] if totals else [])
        sh = shifts_for(pattern, names + ["h_part_off", "h_cons_off"] + outs + ["wire"])
        n, k = w.n_partitions, w.cons_rank.size
        size = {"part_off": w.n_topics + 1, "cons_off": w.n_topics + 1, "cons_rank": k, "out_total_lag": k}
        self.ins = {a: Guarded("device", size.get(a, n), DT[a], sh[a], getattr(w, a), name=a) for a in names}
        self.hins = {a: Guarded("numpy", w.n_topics + 1, np.int64, sh[a], getattr(w, a[2:]), name=a) for a in ("h_part_off", "h_cons_off")}
        self.outs = {a: Guarded("device", size.get(a, n), DT[a], sh[a], name=a) for a in outs}
        b = N.DeviceBatch()
        b.n_topics, b.algo, b.flags = w.n_topics, algo, flags
        b.reset_mode = N.LA_RESET_EARLIEST if form == "earliest" else N.LA_RESET_LATEST
        b.n_partitions, b.n_consumers = n, k
        b.max_partitions_per_topic, b.max_consumers_per_topic = hint or (w.max_partitions, w.max_consumers)
        for a, g in list(self.ins.items()) + list(self.outs.items()):
            setattr(b, FIELD[a], g.ptr)
        b.h_part_off = ctypes.cast(self.hins["h_part_off"].ptr, ctypes.POINTER(ctypes.c_int64))
        b.h_cons_off = ctypes.cast(self.hins["h_cons_off"].ptr, ctypes.POINTER(ctypes.c_int64))
        if bounds is not None:
            b.flags |= N.LA_FLAG_BOUNDS
            b.max_lag_hint, b.max_partition_id_hint = bounds
        if wire is not None:
            self.outs["wire"] = Guarded("device", n, wire.dtype, sh["wire"], name="wire")
            b.flags |= N.LA_FLAG_WIRE_OUT
            b.d_out_wire, b.wire_elem_bytes, b.wire_id_bits = self.outs["wire"].ptr, wire.elem_bytes, wire.id_bits
        self.wire = wire
        stream = torch.cuda.current_stream().cuda_stream
        self.error = None
        try:
            ctx.assign_batch_device(b, stream)
            ctx.sync(stream)
        except N.LagAssignError as e:
            self.error = e
        self.launches = ctx.last_launches()

    def check(self, exp, what="", skip_topics=()):
        """Inputs bit for bit, every guard band, and the results against exp = (order, member, totals); topics in skip_topics
        must still hold the sentinel in all their ranges."""
        for g in list(self.ins.values()) + list(self.hins.values()):
            g.check_unchanged(what)
        for g in self.outs.values():
            g.check_guards(what)
        w = self.w
        keep_p = np.ones(w.n_partitions, bool)
        keep_k = np.ones(w.cons_rank.size, bool)
        for t in skip_topics:
            keep_p[w.part_off[t]:w.part_off[t + 1]] = False
            keep_k[w.cons_off[t]:w.cons_off[t + 1]] = False
        got = {a: g.values() for a, g in self.outs.items()}
        if self.wire is not None:
            want = sharding.pack_results_numpy(exp[0], exp[1], self.wire.elem_bytes, self.wire.id_bits)
            np.testing.assert_array_equal(got["wire"], want, err_msg="wire elements " + what)
        for a, e, m in (("out_partition", exp[0], keep_p), ("out_member_rank", exp[1], keep_p), ("out_total_lag", exp[2], keep_k)):
            if a in got:
                np.testing.assert_array_equal(got[a][m], e[m], err_msg="%s %s" % (a, what))
                assert (got[a][~m] == SENTINEL).all(), "%s written for a topic the call must leave alone %s" % (a, what)


def _run(ctx, w, exp, pattern, **kw):
    c = DeviceCase(ctx, w, pattern, **kw)
    if c.error is not None:
        raise c.error
    c.check(exp, "(%s, %s)" % (pattern, kw))
    return c


def _ragged_tail(p, c, topics, seed, kinds=("u20", "ties", "u40", "zero", "full")):
    """topics of the (p, c) shape, a few a little smaller; the LAST ends mid-tile (p - 3 partitions)."""
    shapes = [(p - (i % 3 == 1) * (i % 5), c - (i % 4 == 3)) for i in range(topics - 1)] + [(max(p - 3, 1), c)]
    return _batch_of(shapes, seed, kinds=list(kinds), negative=True)


# ---- tile path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("topics", [70, 71])          # the last topic's lags: full-range (wide records) / 20-bit (packed records)
@pytest.mark.parametrize("p,c", [(8, 8), (100, 16), (256, 32), (1024, 64)])
def test_tile_shapes_ragged_tail(ctx, p, c, topics, pattern):
    w = _ragged_tail(p, c, topics, p + c)
    _run(ctx, w, _expect(w, w.lag), pattern)
    _run(ctx, w, _expect(w, w.lag), pattern, totals=False)


def _assert_off_16(case, names):
    """The results' 16-byte stores start at a multiple of 4 elements from the array's start: with an element shift of 1 or 3
    every one of them is at an address that is not 16-byte aligned."""
    for a in names:
        g = case.outs[a]
        if g.shift % 4:
            assert g.ptr % 16 != 0, (a, g.ptr)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("p,c,topics", [(256, 32, 64), (1024, 64, 64), (256, 32, 2100), (128, 16, 4100)])
def test_tile_full_tiles_single_launch(ctx, p, c, topics, pattern):
    """Every topic fills its tile exactly and every wavefront is full (the topic count is a multiple of the topics per
    wavefront), so every wavefront -- the one that holds the batch's last topic included -- takes the FULL form of the packed
    kernel: 16-byte stores without a tail check, the last of them ending at the guard band.  LA_FLAG_DEFER_WIDE keeps the
    batch off the single-launch kernel with the wide code inline (which keeps to the general form); the bounds prove that every
    record packs, so the deferred-tile kernel is not launched: one launch.  Small batches widen to 64 lanes x 4 or 16 records,
    the 2 100- and 4 100-topic batches keep 32 x 8 and 16 x 8."""
    w = _batch_of([(p, c)] * topics, 5 * p + c, kinds=["u20", "ties", "zero"])
    bounds = (int(w.lag.max()), int(w.partition_id.max()))
    r = _run(ctx, w, _expect(w, w.lag), pattern, bounds=bounds, flags=N.LA_FLAG_DEFER_WIDE)
    assert r.launches == 1, r.launches
    _assert_off_16(r, ("out_partition", "out_member_rank"))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("algo,flags", [(N.LA_ALGO_ROUNDS_WIDE, 0), (N.LA_ALGO_ARGMIN, 0), (N.LA_ALGO_AUTO, N.LA_FLAG_INDEX64),
                                        (N.LA_ALGO_AUTO, N.LA_FLAG_DEFER_WIDE), (N.LA_ALGO_AUTO, N.LA_FLAG_RAGGED | N.LA_FLAG_SHAPE_CLASSES)])
def test_tile_algos_and_flags(ctx, algo, flags, pattern):
    rng = np.random.default_rng(algo * 100 + flags)
    shapes = [(int(rng.integers(1, 1025)), int(rng.integers(1, 65))) for _ in range(60)] + [(253, 32)]
    w = _batch_of(shapes, algo + flags, negative=True)
    _run(ctx, w, _expect(w, w.lag), pattern, algo=algo, flags=flags, hint=(1024, 64))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("form", ["latest", "earliest"])
def test_tile_offsets_forms(ctx, form, pattern):
    w = _with_offsets(_ragged_tail(256, 32, 90, 17, kinds=("u20", "u40", "ties")), 3)
    lag = oracle.compute_lags(w.begin, w.end, w.committed, form == "latest")
    _run(ctx, w, _expect(w, lag), pattern, form=form)


@pytest.mark.parametrize("pattern", ["odd", "mixed"])
@pytest.mark.parametrize("elem,p,c,full", [(2, 256, 32, False), (2, 61, 8, False), (4, 1024, 64, False), (4, 253, 32, False),
                                           (2, 256, 32, True), (4, 1024, 64, True)])
def test_wire_out_guarded(ctx, elem, p, c, full, pattern):
    """LA_FLAG_WIRE_OUT: 2- and 4-byte elements, guard bands around d_out_wire.  Ragged batches whose last topic ends mid-tile
    (the general form's tail), and batches of full tiles only, whose every wavefront takes the FULL form (8- / 16-byte stores
    of wire elements, the last of them ending at the guard band)."""
    if full:
        w = _with_offsets(_batch_of([(p, c)] * 64, elem * p + c, kinds=["u20", "ties", "zero"]), elem)
    else:
        w = _with_offsets(_ragged_tail(p, c, 50, elem * p + c, kinds=("u20", "ties", "zero")), elem)
    fmt = N.wire_format_for(p - 1, int(w.cons_rank.max()) + 1) if elem == 2 else N.WireFormat(4, 16)
    assert fmt.elem_bytes == elem
    lag = oracle.compute_lags(w.begin, w.end, w.committed, False)
    r = _run(ctx, w, _expect(w, lag), pattern, form="earliest", wire=fmt, bounds=(int(w.end.max()), p - 1))
    assert r.launches == 1, r.launches
    _assert_off_16(r, ("wire",))


# ---- block path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shapes", [
    [(300, 100), (1500, 200), (3000, 800), (7000, 1500), (12000, 900)],        # one topic per block_class, the largest last
    [(2000, 40), (2001, 64), (3000, 65), (2999, 256), (4001, 257), (4097, 1000)],   # greedy forms: slots, 32-bit keys, wide
    [(5000, 300), (7001, 130), (999, 70)],                                     # non-packed lags (negative, full range)
])
def test_block_path(ctx, shapes, pattern):
    kinds = ["full", "u40", "full"] if shapes[0] == (5000, 300) else ["u40", "ties", "pareto", "u20", "zero"]
    w = _batch_of(shapes, sum(p for p, _ in shapes), kinds=kinds, negative=True)
    exp = _expect(w, w.lag)
    _run(ctx, w, exp, pattern)
    _run(ctx, w, exp, pattern, totals=False)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("p,c,nonzero", [(4001, 40, 1010), (3001, 70, 1000), (7001, 128, 2000), (5003, 300, 40)])
def test_block_caught_up_topic_zeros_mid_round(ctx, p, c, nonzero, pattern):
    """A caught-up topic, last in the batch, whose zero lags begin in the middle of a round and C does not divide P.  The
    greedy runs only up to the round with the first zero (P_run = that round's end < P) and the workgroup copies the order
    down behind it: the slots greedy (40 consumers: zeros from round 25 on), the 32-bit-key greedy (70 and 128 consumers:
    rounds 14 and 15); 300 consumers take the wide greedy, which runs every round."""
    rng = np.random.default_rng(p + c)
    lag = np.zeros(p, np.int64)
    lag[:nonzero] = rng.integers(1, 1 << 30, nonzero)
    w0 = _batch_of([(1500, 100), (p, c)], p, kinds=["u20", "u20"])
    lag2 = w0.lag.copy()
    lag2[w0.part_off[1]:] = rng.permutation(lag)
    w = synth.Workload("zeros", 2, w0.part_off, w0.partition_id, w0.begin, lag2.copy(), w0.committed, lag2, w0.cons_off, w0.cons_rank,
                       w0.max_partitions, w0.max_consumers)
    _run(ctx, w, _expect(w, w.lag), pattern)


# ---- large path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shapes,kind", [
    ([(1000, 30), (20003, 5000)], "u20"),           # the narrow form (> 4 096 consumers, 32-bit lags), a partial last round, last
    ([(1000, 30), (20003, 5000)], "u40"),           # the same shape in 64-bit keys
    ([(1000, 30), (9001, 3000)], "u40"),            # four bins per thread: the I32x4 stores of the rounds kernel, 1 live of 4 at the end
    ([(1000, 30), (20001, 9000)], "u40"),           # more than 8 192 consumers: the bins in HBM
    ([(9001, 3000), (20003, 5000), (30001, 2500), (12289, 4097)], "u40"),      # several large topics in one item launch
    ([(9001, 3000), (20003, 5000), (12289, 4097)], "u20"),
])
def test_large_path(ctx, shapes, kind, pattern):
    w = _batch_of(shapes, sum(p + c for p, c in shapes), kinds=[kind])
    exp = _expect(w, w.lag, literal=False)
    _run(ctx, w, exp, pattern)
    if pattern == "mixed":
        _run(ctx, w, exp, pattern, totals=False)


# ---- empty topics and batches, the shape hint ------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shapes", [
    [(0, 5), (100, 8), (50, 0), (0, 0), (201, 16), (0, 3), (30, 0)],
    [(0, 300), (3000, 200), (2000, 0), (0, 0), (1001, 70), (0, 7)],
    [(0, 9000), (9001, 0), (9001, 3000), (100, 0), (0, 5)],
    [(30, 0), (0, 5), (9001, 3000), (0, 2)],
])
def test_empty_topics_anywhere(ctx, shapes, pattern):
    w = _batch_of(shapes, len(shapes), kinds=["u40"])
    _run(ctx, w, _expect(w, w.lag, literal=max(p for p, _ in shapes) < 5000), pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shapes", [[(0, 5), (0, 3)], [(0, 300), (0, 9000)], [(0, 0)]])
def test_batch_without_partitions_writes_totals_only(ctx, shapes, pattern):
    """N == 0: d_out_partition / d_out_member_rank are NULL (not looked at); every consumer's total is written (0)."""
    w = _batch_of(shapes, 1)
    c = _run(ctx, w, _expect(w, w.lag), pattern, results=False)
    assert set(c.outs) == {"out_total_lag"}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("bad", [0, 17, 39])
def test_shape_hint_violation_leaves_the_topic_alone(ctx, bad, pattern):
    """A shape hint within one wave tile (the plain tile dispatch) and one topic beyond it: LA_ESHAPE from la_sync, the topic's
    partition and consumer ranges keep the sentinel; every other topic is assigned as usual."""
    shapes = [(250 - (i % 3), 32) for i in range(40)]
    shapes[bad] = (300, 32)
    w = _batch_of(shapes, bad, kinds=["u20", "u40"])
    c = DeviceCase(ctx, w, pattern, hint=(256, 32))
    assert c.error is not None and c.error.code == N.LA_ESHAPE, c.error
    c.check(_expect(w, w.lag), "(oversize topic %d)" % bad, skip_topics=(bad,))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("hint,flags,big", [((2000, 100), 0, (3000, 100)), ((2000, 100), 0, (1500, 300)),
                                            ((256, 32), N.LA_FLAG_RAGGED | N.LA_FLAG_SHAPE_CLASSES, (300, 32))])
def test_shape_hint_beyond_one_tile_routes_by_the_real_shape(ctx, hint, flags, big, pattern):
    """A hint beyond one wave tile, or LA_FLAG_RAGGED with a hint within one: the library routes every topic by its real shape
    from h_part_off / h_cons_off, so a topic over the hint is assigned like any other (no LA_ESHAPE) -- the header says so."""
    shapes = [(250 - (i % 3), 32) for i in range(30)] + [(1200, 80)]
    shapes[11] = big
    w = _batch_of(shapes, big[0], kinds=["u20", "u40"])
    _run(ctx, w, _expect(w, w.lag), pattern, hint=hint, flags=flags)


# ---- device-resident grouping and the wire pack / unpack ----------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["odd", "three", "mixed"])
def test_group_by_member_device_guarded(ctx, pattern):
    import torch
    w = _ragged_tail(256, 32, 300, 9)
    e_p, e_m, _ = _expect(w, w.lag)
    m = int(w.cons_rank.max()) + 1
    n = w.n_partitions
    sh = shifts_for(pattern, ["part_off", "p", "m", "off", "t", "g"])
    ins = [Guarded("device", w.n_topics + 1, np.int64, sh["part_off"], w.part_off, name="part_off"),
           Guarded("device", n, np.int32, sh["p"], e_p, name="out_partition"), Guarded("device", n, np.int32, sh["m"], e_m, name="out_member_rank")]
    outs = [Guarded("device", m + 1, np.int64, sh["off"], name="member_off"), Guarded("device", n, np.int32, sh["t"], name="grouped_topic"),
            Guarded("device", n, np.int32, sh["g"], name="grouped_partition")]
    stream = torch.cuda.current_stream().cuda_stream
    ctx.group_by_member_device(w.n_topics, n, ins[0].ptr, ins[1].ptr, ins[2].ptr, m, outs[0].ptr, outs[1].ptr, outs[2].ptr, stream)
    ctx.sync(stream)
    for g in ins:
        g.check_unchanged()
    for g in outs:
        g.check_guards()
    order = np.argsort(e_m, kind="stable")
    topic_of = np.searchsorted(w.part_off, np.arange(n), side="right") - 1
    np.testing.assert_array_equal(outs[0].values(), np.cumsum(np.bincount(e_m + 1, minlength=m + 1))[: m + 1])
    np.testing.assert_array_equal(outs[1].values(), topic_of[order])
    np.testing.assert_array_equal(outs[2].values(), e_p[order])


@pytest.mark.parametrize("pattern", ["odd", "three", "mixed"])
@pytest.mark.parametrize("max_id,members,n", [(255, 30, 4099), (4000, 1000, 1027), (-1, 5, 333)])
def test_pack_unpack_guarded(ctx, max_id, members, n, pattern):
    import torch
    rng = np.random.default_rng(n)
    pid = rng.integers(0, (max_id if max_id >= 0 else 1 << 30) + 1, n).astype(np.int32)
    rank = rng.integers(-1, members, n).astype(np.int32)
    fmt = N.wire_format_for(max_id, members)
    sh = shifts_for(pattern, ["p", "m", "wire", "p2", "m2"])
    ins = [Guarded("device", n, np.int32, sh["p"], pid, name="pid"), Guarded("device", n, np.int32, sh["m"], rank, name="rank")]
    wire = Guarded("device", n, fmt.dtype, sh["wire"], name="wire")
    back = [Guarded("device", n, np.int32, sh["p2"], name="pid back"), Guarded("device", n, np.int32, sh["m2"], name="rank back")]
    stream = torch.cuda.current_stream().cuda_stream
    ctx.pack_results(n, ins[0].ptr, ins[1].ptr, fmt, wire.ptr, stream)
    ctx.sync(stream)
    ctx.unpack_results(n, wire.ptr, fmt, back[0].ptr, back[1].ptr, stream)
    ctx.sync(stream)
    for g in ins:
        g.check_unchanged()
    wire.check_guards()
    for g in back:
        g.check_guards()
    np.testing.assert_array_equal(wire.values(), sharding.pack_results_numpy(pid, rank, fmt.elem_bytes, fmt.id_bits))
    np.testing.assert_array_equal(back[0].values(), pid)
    np.testing.assert_array_equal(back[1].values(), rank)


# ---- host entry points, every pipeline ----------------------------------------------------------------------------------------
def _host_batch(big):
    """Tile- and block-sized topics with offsets.  The first topic has an odd partition count and every other one an even count:
    every topic boundary after the first lies at an odd partition index (where the shards and chunks of a split call begin)."""
    rng = np.random.default_rng(7 if big else 8)
    t = 600 if big else 40
    shapes = [(int(rng.integers(1, 257 if big else 129)) * 2 + (i == 0), int(rng.integers(0, 40))) for i in range(t)]
    shapes[t // 2] = (3000, 200)                           # one block-path topic
    shapes[-1] = (253, 32)                                 # the last ends mid-tile
    w = _with_offsets(_batch_of(shapes, t, kinds=["u20", "u40", "ties"]), t)
    return w


PIPES = {"ZERO_COPY": (0, "numpy", False, N.LA_PIPELINE_ZERO_COPY, False), "ONE_COPY": (0, "numpy", False, N.LA_PIPELINE_ONE_COPY, False),
         "LANES": (N.LA_CREATE_SPLIT_ALWAYS | 3, "numpy", True, N.LA_PIPELINE_LANES, False),
         "STREAMS": (0, "pinned", True, N.LA_PIPELINE_STREAMS, False), "MAPPED": (0, "pinned", True, N.LA_PIPELINE_MAPPED, False),
         "SHARDS": (N.LA_CREATE_SPLIT_ALWAYS, "numpy", True, N.LA_PIPELINE_LANES, True),
         "MAPPED_SHARDS": (N.LA_CREATE_SPLIT_ALWAYS, "pinned", True, N.LA_PIPELINE_MAPPED, True)}


@pytest.fixture(scope="module")
def host_batches():
    out = {}
    for big in (False, True):
        w = _host_batch(big)
        lag = oracle.compute_lags(w.begin, w.end, w.committed, False)
        out[big] = (w, lag, _expect(w, lag))
    return out


@pytest.mark.parametrize("pattern", ["odd", "mixed"])
@pytest.mark.parametrize("pipe", list(PIPES))
def test_host_entry_points(host_batches, pipe, pattern):
    flags, kind, big, want, sharded = PIPES[pipe]
    w, lag, exp = host_batches[big]
    n, k, T = w.n_partitions, w.cons_rank.size, w.n_topics
    m = int(w.cons_rank.max()) + 1
    if pipe == "ONE_COPY":
        os.environ["LA_ZERO_COPY_BYTES"] = "0"
    try:
        c = N.Context([0, 0, 0] if sharded else 0, flags=flags)
    finally:
        os.environ.pop("LA_ZERO_COPY_BYTES", None)
    if pipe == "STREAMS":
        os.environ["LA_NO_MAPPED_PIPELINE"] = "1"
    try:
        with c:
            names = ["part_off", "partition_id", "begin", "end", "committed", "cons_off", "cons_rank", "lag", "none_index", "none_begin"]
            idx, val = N.sparse_begin(w.begin, w.committed)
            src = {"part_off": w.part_off, "partition_id": w.partition_id, "begin": w.begin, "end": w.end, "committed": w.committed,
                   "cons_off": w.cons_off, "cons_rank": w.cons_rank, "lag": lag, "none_index": idx, "none_begin": val}
            sh = shifts_for(pattern, names + ["p", "m", "t", "off", "gt", "gp", "lagout"])
            G = {a: Guarded(kind, np.asarray(src[a]).size, np.asarray(src[a]).dtype, sh[a], src[a], ctx=c, name=a) for a in names}
            I = {a: g.array for a, g in G.items()}

            def outs(total):
                return [Guarded(kind, n, np.int32, sh["p"], ctx=c, name="out_partition"),
                        Guarded(kind, n, np.int32, sh["m"], ctx=c, name="out_member_rank"),
                        Guarded(kind, k, np.int64, sh["t"], ctx=c, name="out_total_lag") if total else None]

            def check(o, e, what):
                assert c.last_pipeline() == want, (what, c.last_pipeline())
                for g in G.values():
                    g.check_unchanged(what)
                for g, ev, name in zip(o, e, ("order", "member", "totals")):
                    if g is not None:
                        g.check_guards(what)
                        np.testing.assert_array_equal(g.values(), ev, err_msg="%s %s" % (name, what))
                if sharded and big:
                    b = c.last_shard_bounds()
                    assert b.size == 4 and all(int(w.part_off[x]) % 2 == 1 for x in b[1:-1] if 0 < x < T), b

            dense = (I["part_off"], I["partition_id"], I["begin"], I["end"], I["committed"], N.LA_RESET_EARLIEST, I["cons_off"], I["cons_rank"])
            for total in (True, False):
                o = outs(total)
                arr = tuple(None if g is None else g.array for g in o)
                c.assign_batch(*dense, out=arr)
                check(o, exp, "la_assign_batch totals=%s" % total)
                o = outs(total)
                c.assign_batch_sparse(I["part_off"], I["partition_id"], I["end"], I["committed"], N.LA_RESET_EARLIEST, I["none_index"],
                                      I["none_begin"], I["cons_off"], I["cons_rank"], out=tuple(None if g is None else g.array for g in o))
                check(o, exp, "la_assign_batch_sparse totals=%s" % total)
                o = outs(total)
                c.assign_batch_lags(I["part_off"], I["partition_id"], I["lag"], I["cons_off"], I["cons_rank"],
                                    out=tuple(None if g is None else g.array for g in o))
                check(o, exp, "la_assign_batch_lags totals=%s" % total)

            order = np.argsort(exp[1], kind="stable")
            topic_of = (np.searchsorted(w.part_off, np.arange(n), side="right") - 1).astype(np.int32)
            e_off = np.cumsum(np.bincount(exp[1] + 1, minlength=m + 1))[: m + 1]

            def grouped_outs(topic, total):
                return [Guarded(kind, m + 1, np.int64, sh["off"], ctx=c, name="member_off"),
                        Guarded(kind, n, np.int32, sh["gt"], ctx=c, name="grouped_topic") if topic else None,
                        Guarded(kind, n, np.int32, sh["gp"], ctx=c, name="grouped_partition"),
                        Guarded(kind, k, np.int64, sh["t"], ctx=c, name="out_total_lag") if total else None]

            def check_grouped(o, what, pipeline=True):
                if pipeline:
                    assert c.last_pipeline() == want, (what, c.last_pipeline())
                for g in G.values():
                    g.check_unchanged(what)
                for g, ev in zip(o, (e_off, topic_of[order], exp[0][order], exp[2])):
                    if g is not None:
                        g.check_guards(what)
                        np.testing.assert_array_equal(g.values(), ev, err_msg="%s %s" % (g.name, what))

            for topic, total in ((True, True), (False, False)):
                o = grouped_outs(topic, total)
                arr = tuple(None if g is None else g.array for g in o)
                c.assign_batch_grouped(*dense, m, out=arr)
                check_grouped(o, "la_assign_batch_grouped topic=%s totals=%s" % (topic, total))
                if topic:                                  # the results the grouped call left on the device
                    o2 = grouped_outs(True, False)
                    c.group_last_by_member(n, m, out=(o2[0].array, o2[1].array, o2[2].array))
                    check_grouped(o2, "la_group_last_by_member", pipeline=False)
                o = grouped_outs(topic, total)
                c.assign_batch_grouped_sparse(I["part_off"], I["partition_id"], I["end"], I["committed"], N.LA_RESET_EARLIEST,
                                              I["none_index"], I["none_begin"], I["cons_off"], I["cons_rank"], m,
                                              out=tuple(None if g is None else g.array for g in o))
                check_grouped(o, "la_assign_batch_grouped_sparse topic=%s totals=%s" % (topic, total))

            # la_compute_lag and la_group_by_member on the same guarded arrays
            lo = Guarded(kind, n, np.int64, sh["lagout"], ctx=c, name="out_lag")
            c.compute_lag(I["begin"], I["end"], I["committed"], N.LA_RESET_EARLIEST, out=lo.array)
            lo.check_guards("la_compute_lag")
            np.testing.assert_array_equal(lo.values(), lag)
            rp = Guarded(kind, n, np.int32, sh["p"], exp[0], ctx=c, name="out_partition (input)")
            rm = Guarded(kind, n, np.int32, sh["m"], exp[1], ctx=c, name="out_member_rank (input)")
            o = grouped_outs(True, False)
            off, g_t, g_p = o[0].array, o[1].array, o[2].array
            rc = N.load().la_group_by_member(c._h, T, N._addr(I["part_off"]), N._addr(rp.array), N._addr(rm.array), m, N._addr(off),
                                             N._addr(g_t), N._addr(g_p))
            assert rc == N.LA_OK, N.load().la_last_error(c._h)
            rp.check_unchanged("la_group_by_member")
            rm.check_unchanged("la_group_by_member")
            check_grouped(o, "la_group_by_member", pipeline=False)
            for g in G.values():
                g.check_unchanged("at the end")
    finally:
        os.environ.pop("LA_NO_MAPPED_PIPELINE", None)


# ---- call-history independence --------------------------------------------------------------------------------------------
def test_device_results_do_not_depend_on_the_calls_before(ctx):
    small = _ragged_tail(256, 32, 50, 31)
    other = _batch_of([(1000, 30), (9001, 3000), (3000, 200), (253, 32), (20003, 5000)], 32, kinds=["u40"])
    e_small = _expect(small, small.lag)
    first = _run(ctx, small, e_small, "mixed")
    _run(ctx, other, _expect(other, other.lag, literal=False), "three")
    again = _run(ctx, small, e_small, "mixed")
    for a in first.outs:
        np.testing.assert_array_equal(first.outs[a].raw_bytes(), again.outs[a].raw_bytes(), err_msg=a)


def test_host_results_do_not_depend_on_the_calls_before(ctx):
    small = _with_offsets(_ragged_tail(256, 32, 60, 41, kinds=("u20", "u40")), 1)
    other = _with_offsets(_batch_of([(1000, 30), (9001, 3000), (3000, 200), (253, 32)], 42, kinds=["u40"]), 2)

    def call(w):
        names = ["part_off", "partition_id", "begin", "end", "committed", "cons_off", "cons_rank"]
        sh = shifts_for("mixed", names + ["p", "m", "t"])
        i = {a: Guarded("numpy", getattr(w, a).size, getattr(w, a).dtype, sh[a], getattr(w, a), name=a) for a in names}
        o = [Guarded("numpy", w.n_partitions, np.int32, sh["p"], name="out_partition"),
             Guarded("numpy", w.n_partitions, np.int32, sh["m"], name="out_member_rank"),
             Guarded("numpy", w.cons_rank.size, np.int64, sh["t"], name="out_total_lag")]
        a = {k: g.array for k, g in i.items()}
        ctx.assign_batch(a["part_off"], a["partition_id"], a["begin"], a["end"], a["committed"], N.LA_RESET_EARLIEST, a["cons_off"],
                         a["cons_rank"], out=tuple(g.array for g in o))
        for g in i.values():
            g.check_unchanged()
        for g in o:
            g.check_guards()
        return o, ctx.last_pipeline()

    lag = oracle.compute_lags(small.begin, small.end, small.committed, False)
    e = _expect(small, lag)
    first, pipe1 = call(small)
    _, pipe2 = call(other)
    again, pipe3 = call(small)
    assert pipe1 == pipe3 == N.LA_PIPELINE_ZERO_COPY
    for g0, g1, ev in zip(first, again, e):
        np.testing.assert_array_equal(g0.values(), ev)
        np.testing.assert_array_equal(g0.raw_bytes(), g1.raw_bytes())
