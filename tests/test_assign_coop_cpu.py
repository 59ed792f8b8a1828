"""la_assign_batch_cooperative without a GPU: the binding's struct against the C compiler's layout of the header, the numpy
restatement (sharding.assign_cooperative_numpy) against the dictionary model of tests/coop_cases.py over oracle targets, the
convergence and safety of repeated cooperative rounds, and the host's marshalling of the owned lists."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from kafka_lag_based_assignor_amd import _native, sharding
from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor, _host
from oracle import oracle

from coop_cases import CoopCase, claims_from, dict_model, layout, owned_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assign_coop_args_has_the_c_compilers_size_and_field_offsets():
    A = _native.AssignCoopArgs
    names = [n for n, _ in A._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_assign_coop_args));\n' +
           "".join('printf(" %%zu", offsetof(la_assign_coop_args, %s));\n' % n for n in names) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in names]
    assert "la_assign_batch_cooperative" in _native.EXPORTED_SYMBOLS
    assert _native.AssignCoop._fields[:3] == ("out_partition", "out_member_rank", "totals") and len(_native.AssignCoop._fields) == 14


def subscriptions(rng, t, m):
    """Every topic's subscribers: a random subset of the members (every fifth topic: nobody), ascending ranks."""
    segs = [np.sort(rng.choice(m, int(rng.integers(1, m + 1)), replace=False)) if i % 5 != 4 else np.empty(0, np.int64) for i in range(t)]
    off = np.concatenate([[0], np.cumsum([s.size for s in segs])]).astype(np.int64)
    return off, np.concatenate(segs + [np.empty(0, np.int64)]).astype(np.int32)


def test_the_numpy_restatement_equals_the_dictionary_model_over_oracle_targets():
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        sizes = rng.integers(0, 30, int(rng.integers(1, 7))).tolist()
        m = int(rng.integers(1, 7))
        part_off, pid = layout(seed, sizes, ("shuffled", "negative", "full")[seed % 3])
        lag = rng.integers(0, 1 << 30, pid.size)
        cons_off, cons_rank = subscriptions(rng, len(sizes), m)
        claims = claims_from(seed, part_off, pid, m, n_stale=seed % 4, n_unmapped=seed % 3)
        off, topic, opid = owned_arrays(m, claims, seed % 3, seed % 2, seed)
        got = sharding.assign_cooperative_numpy(part_off, pid, lag, cons_off, cons_rank, m, off, topic, opid, assign=oracle.assign_flat)
        assert len(got) == 14
        target = oracle.assign_flat(part_off, pid, lag, cons_off, cons_rank)
        for g, e in zip(got[:3], target):
            np.testing.assert_array_equal(g, e)
        model = dict_model(CoopCase(part_off, target[0], target[1], m, off, topic, opid))
        for k, (g, e) in enumerate(zip(got[3:11], model)):
            np.testing.assert_array_equal(g, e, err_msg="output %d, seed %d" % (k, seed))
        for g, e in zip(got[11:], sharding.group_by_member_numpy(part_off, target[0], model[1], m)):
            np.testing.assert_array_equal(g, e, err_msg="lists, seed %d" % seed)


def test_cooperative_rounds_converge_within_two_and_never_hand_out_what_is_still_owned():
    worst = 0
    for seed in range(240):
        rng = np.random.default_rng(seed)
        t, m = int(rng.integers(1, 6)), int(rng.integers(1, 7))
        sizes = rng.integers(0, 12, t).tolist()
        part_off, pid = layout(seed, sizes)
        # rebalance 0, eager: what everybody owns to begin with
        co0, cr0 = subscriptions(rng, t, m)
        first = oracle.assign_flat(part_off, pid, rng.integers(0, 1000, pid.size), co0, cr0)
        owned = sharding.group_by_member_numpy(part_off, first[0], first[1], m)
        # rebalance 1: other subscriptions, other lags
        lag = rng.integers(0, 1000, pid.size)
        cons_off, cons_rank = subscriptions(rng, t, m)
        target = oracle.assign_flat(part_off, pid, lag, cons_off, cons_rank)
        eager = sharding.group_by_member_numpy(part_off, target[0], target[1], m)
        rounds = 0
        while True:
            rounds += 1
            got = sharding.assign_cooperative_numpy(part_off, pid, lag, cons_off, cons_rank, m, *owned, assign=oracle.assign_flat)
            off, g_topic, g_pid = got[11:]
            lo = int(owned[0][0])
            owner = {(int(a), int(b)): int(np.searchsorted(owned[0], j, side="right") - 1)
                     for j, (a, b) in enumerate(zip(owned[1][lo:], owned[2][lo:]), lo)}
            for j in range(int(off[0]), pid.size):                   # safety: nobody is handed what another member still owns
                who = int(np.searchsorted(off, j, side="right") - 1)
                assert owner.get((int(g_topic[j]), int(g_pid[j])), who) == who, (seed, rounds)
            owned = (off, g_topic, g_pid)                            # as they lie: the head before off[0] is ignored
            if got[10][5] == 0:
                break
            assert rounds < 2, "seed %d needs a third round" % seed
        worst = max(worst, rounds)
        lo = int(off[0])
        np.testing.assert_array_equal(off, eager[0], err_msg="seed %d" % seed)
        np.testing.assert_array_equal(g_topic[lo:], eager[1][lo:], err_msg="seed %d" % seed)
        np.testing.assert_array_equal(g_pid[lo:], eager[2][lo:], err_msg="seed %d" % seed)
    assert worst == 2                                                  # (the cases do exercise a follow-up)


def test_host_marshalling_of_the_owned_lists():
    h = _host()
    assert LagBasedPartitionAssignor.supported_protocols() == ["COOPERATIVE", "EAGER"]
    # ids that sort differently from their insertion order ("app-10" < "app-2" < "b"); a deleted topic; nothing owned
    members = ["b", "app-2", "app-10", "idle"]
    topics = ["payments", "orders"]
    owned = [[("orders", 7), ("deleted", 1)], [("payments", 0)], [("orders", 3), ("payments", 2), ("nosub", 0)], []]
    off, topic, part = h.cooperative_owned_arrays(members, topics, owned)
    assert h.rank_members(members) == [2, 1, 0, 3]
    assert off == [0, 3, 4, 6, 6]                                      # app-10, app-2, b, idle (an empty slice)
    assert topic == [1, 0, -1, 0, 1, -1]
    assert part == [3, 2, 0, 0, 7, 1]
    assert h.cooperative_owned_arrays([], topics, []) == ([0], [], [])
    assert h.cooperative_owned_arrays(["a"], [], [[("x", 1)]]) == ([0, 1], [-1], [1])
