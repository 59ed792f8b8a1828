"""What every shard-scoped entry point of the C ABI promises before it looks at its own arguments, through ctypes on
_native.load(): a NULL context is LA_EINVAL, a shard outside [0, la_shard_count()) is LA_EINVAL with "shard S of N" as the
last error, the calling thread's current device is left alone by refused and accepted calls alike, and the context goes on
working afterwards.  The real calls run on the smallest shape that exercises each entry (1 topic, 3 partitions with a tie in
their lags, 2 consumers) and are held to the oracle.

The current-device check can only fail where the process sees two or more devices: on a one-device machine the current device
is 0 before and after every call, and the `[0, 0]` context puts both of its shards on device 0.  There it still runs, and
checks nothing."""
import ctypes

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding
from oracle import oracle

pytestmark = pytest.mark.gpu

PART_OFF = np.array([0, 3], np.int64)
PID = np.array([0, 1, 2], np.int32)
LAG = np.array([5, 0, 5], np.int64)                   # a tie: the reference breaks it by partition id
CONS_OFF = np.array([0, 2], np.int64)
CONS_RANK = np.array([0, 1], np.int32)
T, P, K, M = 1, 3, 2, 2
SENTINEL = -7


class Rig:
    """Device arrays of the tiny workload on device 0 and, per entry point, the call with every argument valid but the shard."""

    def __init__(self, torch):
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.lib = N.load()
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        up = lambda a: torch.from_numpy(a.copy()).to(self.dev)
        self.d = {"part_off": up(PART_OFF), "pid": up(PID), "lag": up(LAG), "cons_off": up(CONS_OFF), "cons_rank": up(CONS_RANK)}
        self.fmt = N.wire_format_for(int(PID.max()), M)
        self.outputs = []
        for name, size, dtype in (("out_pid", P, torch.int32), ("out_rank", P, torch.int32), ("out_total", K, torch.int64),
                                  ("verdict", T, torch.int32), ("summary", 4, torch.int64),
                                  ("m_parts", M, torch.int64), ("m_lag", M, torch.int64), ("unassigned", 1, torch.int64),
                                  ("prev_owner", P, torch.int32), ("topic_moved", T, torch.int64), ("gained", M, torch.int64),
                                  ("lost", M, torch.int64), ("moved", 1, torch.int64),
                                  ("packed", P * int(self.fmt.elem_bytes), torch.uint8),
                                  ("back_pid", P, torch.int32), ("back_rank", P, torch.int32),
                                  ("g_off", M + 1, torch.int64), ("g_topic", P, torch.int32), ("g_part", P, torch.int32)):
            self.d[name] = torch.empty((size,), device=self.dev, dtype=dtype)
            self.outputs.append(name)
        self.reset()
        p = self.ptr
        b = N.DeviceBatch()
        b.n_topics, b.reset_mode, b.algo, b.flags = T, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, 0
        b.n_partitions, b.n_consumers, b.max_partitions_per_topic, b.max_consumers_per_topic = P, K, P, K
        b.d_part_off, b.d_partition_id, b.d_lag = p("part_off"), p("pid"), p("lag")
        b.d_cons_off, b.d_cons_rank = p("cons_off"), p("cons_rank")
        b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = p("out_pid"), p("out_rank"), p("out_total")
        self.batch = b
        m = N.MovesArgs()
        m.struct_size, m.n_topics, m.n_partitions, m.max_partitions_per_topic = ctypes.sizeof(N.MovesArgs), T, P, P
        m.d_part_off = p("part_off")
        m.d_out_partition, m.d_out_member_rank = p("out_pid"), p("out_rank")
        m.d_prev_partition, m.d_prev_member_rank = p("out_pid"), p("out_rank")            # against itself: nothing moved
        m.n_members, m.n_prev_members = M, M
        m.d_prev_owner, m.d_topic_moved, m.d_member_gained, m.d_member_lost, m.d_moved = (
            p("prev_owner"), p("topic_moved"), p("gained"), p("lost"), p("moved"))
        self.moves = m
        L, st, vp = self.lib, self.stream, lambda name: ctypes.c_void_p(p(name))
        # in the order of the real sequence below
        self.calls = {
            "la_assign_batch_device_on": lambda h, s: L.la_assign_batch_device_on(h, s, ctypes.byref(self.batch), st),
            "la_sync_on": lambda h, s: L.la_sync_on(h, s, st),
            "la_verify_assignment_device_on": lambda h, s: L.la_verify_assignment_device_on(
                h, s, ctypes.byref(self.batch), vp("verdict"), vp("summary"), st),
            "la_member_loads_device_on": lambda h, s: L.la_member_loads_device_on(
                h, s, P, vp("out_rank"), K, vp("cons_rank"), vp("out_total"), M, vp("m_parts"), vp("m_lag"), vp("unassigned"), st),
            "la_assignment_moves_device_on": lambda h, s: L.la_assignment_moves_device_on(h, s, ctypes.byref(self.moves), st),
            "la_pack_results_on": lambda h, s: L.la_pack_results_on(
                h, s, P, vp("out_pid"), vp("out_rank"), ctypes.byref(self.fmt), vp("packed"), st),
            "la_unpack_results_on": lambda h, s: L.la_unpack_results_on(
                h, s, P, vp("packed"), ctypes.byref(self.fmt), vp("back_pid"), vp("back_rank"), st),
            "la_group_by_member_device_on": lambda h, s: L.la_group_by_member_device_on(
                h, s, T, P, vp("part_off"), vp("out_pid"), vp("out_rank"), M, vp("g_off"), vp("g_topic"), vp("g_part"), st),
        }

    def reset(self):
        """Every output back to the sentinel: what a call of this run did not write cannot pass for its result."""
        for name in self.outputs:
            self.d[name].fill_(SENTINEL % 256 if self.d[name].dtype == self.torch.uint8 else SENTINEL)
        self.torch.cuda.synchronize()

    def ptr(self, name):
        return self.d[name].data_ptr()

    def host(self, name):
        return self.d[name].cpu().numpy()

    def current_device(self):
        return self.torch.cuda.current_device()                      # torch owns the HIP runtime: ask torch

    def error(self, h):
        return self.lib.la_last_error(h).decode()

    def refused(self, h, shard, count):
        """Every entry refuses `shard` with LA_EINVAL and "shard S of N", and leaves the current device alone."""
        before = self.current_device()
        for name, call in self.calls.items():
            assert call(h, shard) == N.LA_EINVAL, name
            assert self.error(h) == "shard %d of %d" % (shard, count), name
            assert self.current_device() == before, name

    def real_sequence(self, h, shard):
        """A real call of each kind on `shard`, every result against the oracle; the current device stays where it was."""
        self.reset()
        before = self.current_device()

        def run(name):
            assert self.calls[name](h, shard) == N.LA_OK, "%s: %s" % (name, self.error(h))
            assert self.current_device() == before, name

        def sync(after):
            assert self.calls["la_sync_on"](h, shard) == N.LA_OK, "la_sync_on after %s: %s" % (after, self.error(h))
            assert self.current_device() == before, after

        e_pid, e_rank, e_tot = oracle.assign_flat(PART_OFF, PID, LAG, CONS_OFF, CONS_RANK)
        run("la_assign_batch_device_on")
        sync("la_assign_batch_device_on")
        np.testing.assert_array_equal(self.host("out_pid"), e_pid)
        np.testing.assert_array_equal(self.host("out_rank"), e_rank)
        np.testing.assert_array_equal(self.host("out_total"), e_tot)

        run("la_verify_assignment_device_on")
        sync("la_verify_assignment_device_on")
        assert list(self.host("verdict")) == [0] and list(self.host("summary")) == [0, 0, -1, -1]

        run("la_member_loads_device_on")
        sync("la_member_loads_device_on")
        parts, lag, unassigned = sharding.member_loads_numpy(e_rank, CONS_RANK, e_tot, M)
        np.testing.assert_array_equal(self.host("m_parts"), parts)
        np.testing.assert_array_equal(self.host("m_lag"), lag)
        assert int(self.host("unassigned")[0]) == unassigned

        run("la_assignment_moves_device_on")
        sync("la_assignment_moves_device_on")
        owner, topic_moved, gained, lost, moved = sharding.assignment_moves_numpy(PART_OFF, e_pid, e_rank, e_pid, e_rank, M)
        assert moved == 0
        np.testing.assert_array_equal(self.host("prev_owner"), owner)
        np.testing.assert_array_equal(self.host("prev_owner"), e_rank)
        np.testing.assert_array_equal(self.host("topic_moved"), topic_moved)
        np.testing.assert_array_equal(self.host("gained"), gained)
        np.testing.assert_array_equal(self.host("lost"), lost)
        assert int(self.host("moved")[0]) == 0

        run("la_pack_results_on")
        run("la_unpack_results_on")
        sync("la_unpack_results_on")
        np.testing.assert_array_equal(self.host("back_pid"), e_pid)
        np.testing.assert_array_equal(self.host("back_rank"), e_rank)

        run("la_group_by_member_device_on")
        sync("la_group_by_member_device_on")
        order = np.argsort(e_rank, kind="stable")                    # member by member, inside a member in the reference's order
        np.testing.assert_array_equal(self.host("g_off"), np.searchsorted(e_rank[order], np.arange(M + 1)))
        np.testing.assert_array_equal(self.host("g_part"), e_pid[order])
        np.testing.assert_array_equal(self.host("g_topic"), np.zeros(P, np.int32))


@pytest.fixture(scope="module")
def rig(torch_dev):
    return Rig(torch_dev[0])


def test_the_table_holds_every_exported_on_entry(rig):
    exported = {name for name in N.EXPORTED_SYMBOLS if name.endswith("_on")}
    assert exported == set(rig.calls), "shard-scoped entry points missing from this file's table: %s" % sorted(exported - set(rig.calls))
    for name in rig.calls:
        assert hasattr(rig.lib, name), name


def test_a_null_context_is_einval(rig):
    before = rig.current_device()
    for name, call in rig.calls.items():
        assert call(None, 0) == N.LA_EINVAL, name
        assert rig.current_device() == before, name
    times = N.PhaseTimes()
    assert rig.lib.la_last_phase_times(None, ctypes.byref(times)) == N.LA_EINVAL
    assert rig.current_device() == before


def test_one_shard_refuses_the_shards_it_has_not_and_works_afterwards(ctx, rig):
    assert ctx.shard_count == 1
    rig.refused(ctx._h, -1, 1)
    rig.refused(ctx._h, ctx.shard_count, 1)
    rig.real_sequence(ctx._h, 0)


def test_two_shards_on_one_device_accept_the_second_and_refuse_a_third(rig):
    with N.Context([0, 0]) as c:
        assert c.shard_count == 2
        rig.refused(c._h, 2, 2)
        rig.refused(c._h, -1, 2)
        rig.real_sequence(c._h, 1)
