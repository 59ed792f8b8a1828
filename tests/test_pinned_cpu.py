"""The pinned assignment on the host: sharding.assign_pinned_numpy (the yardstick of tests/test_pinned_gpu.py) against the
dictionary model of pinned_cases.py and, with nothing owned, against the reference oracle; the settling scenario that is the
reason for the call; what the cooperative round withholds of a pinned target.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native, sharding
from oracle import oracle

from pinned_cases import BROKEN, CASES, OVER, PinnedCase, Scenario, broken, dict_model, drawn, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pinned_args_has_the_c_compilers_size_and_field_offsets():
    A = _native.PinnedArgs
    names = [n for n, _ in A._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_pinned_args));\n' +
           "".join('printf(" %%zu", offsetof(la_pinned_args, %s));\n' % n for n in names) +
           'printf(" %d %d %d", LA_PINNED_MAX_PARTITIONS, LA_PINNED_MAX_CONSUMERS, LA_COOP_PINNED);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(A)] + [getattr(A, n).offset for n in names] + [
        _native.PINNED_MAX_PARTITIONS, _native.PINNED_MAX_CONSUMERS, _native.LA_COOP_PINNED]
    assert (sharding.PINNED_MAX_PARTITIONS, sharding.PINNED_MAX_CONSUMERS) == (_native.PINNED_MAX_PARTITIONS, _native.PINNED_MAX_CONSUMERS)


def test_the_library_exports_the_pinned_call():
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "la_assign_pinned_device")


def test_the_worked_case_of_the_header():
    out_pid, out_rank, totals, topic_free, summary = CASES["the worked case"]().expect()
    assert out_pid.tolist() == [0, 1, 2, 3, 4, 5]
    assert out_rank.tolist() == [0, 0, 1, 2, 2, 1]
    assert totals.tolist() == [90, 35, 30]
    assert topic_free.tolist() == [3] and summary.tolist() == [3, 3, 0, 0]


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_equals_the_dictionary_model_on_the_table(name):
    c = CASES[name]()
    same(c.expect(), dict_model(c), name)


def test_numpy_equals_the_dictionary_model_on_200_draws():
    for seed in range(200):
        rng = np.random.default_rng(5000 + seed)
        m = int(rng.integers(1, 12))
        shapes = [(int(rng.integers(0, 40)), int(rng.integers(0, m + 1))) for _ in range(int(rng.integers(1, 5)))]
        c = drawn(seed, shapes, m, lags=["u20", "ties", "zero", "full", "huge"][seed % 5], ids=["shuffled", "negative", "spread"][seed % 3],
                  owned=float(rng.random()), foreign=float(rng.random()) * 0.5, n_stale=seed % 4, n_unmapped=seed % 3,
                  head=seed % 2, tail=(seed // 2) % 3)
        same(c.expect(), dict_model(c), "seed %d" % seed)


def test_with_nothing_owned_it_is_the_reference_assignment():
    for seed in range(30):
        rng = np.random.default_rng(6000 + seed)
        m = int(rng.integers(1, 70))
        shapes = [(int(rng.integers(0, 200)), int(rng.integers(0, m + 1))) for _ in range(4)]
        c = drawn(seed, shapes, m, lags=["u20", "ties", "zero", "huge"][seed % 4], owned=0.0)
        e_pid, e_rank, e_tot = oracle.assign_flat(c.part_off, c.pid, c.lag, c.cons_off, c.cons_rank)
        out_pid, out_rank, totals, topic_free, summary = c.expect()
        np.testing.assert_array_equal(out_pid, e_pid)
        np.testing.assert_array_equal(out_rank, e_rank)
        np.testing.assert_array_equal(totals, e_tot)
        np.testing.assert_array_equal(topic_free, np.diff(c.part_off))
        assert summary.tolist() == [0, c.n, 0, 0]


@pytest.mark.parametrize("bad", list(BROKEN))
def test_what_the_device_reports_is_a_value_error(bad):
    c, _ = broken(bad)
    with pytest.raises(ValueError):
        c.expect()
    with pytest.raises(ValueError):
        dict_model(c)


@pytest.mark.parametrize("name", list(OVER))
def test_a_topic_over_the_limits_is_refused_or_skipped(name):
    c = OVER[name]()
    with pytest.raises(ValueError):
        c.expect()
    got = c.expect(strict=False)
    over = c.over_limit()
    assert over.any() and not over.all()
    for t in np.flatnonzero(~over):                  # every other topic: what it is on its own
        p0, p1, c0, c1 = (int(x) for x in (c.part_off[t], c.part_off[t + 1], c.cons_off[t], c.cons_off[t + 1]))
        keep = c.owned_topic == t
        alone = sharding.assign_pinned_numpy([0, p1 - p0], c.pid[p0:p1], c.lag[p0:p1], [0, c1 - c0], c.cons_rank[c0:c1], c.m,
                                             c.owned_off, np.where(keep, 0, -1), c.owned_pid)
        np.testing.assert_array_equal(got[0][p0:p1], alone[0])
        np.testing.assert_array_equal(got[1][p0:p1], alone[1])
        np.testing.assert_array_equal(got[2][c0:c1], alone[2])
        assert got[3][t] == alone[3][0]
    assert (got[3][over] == 0).all()


def _settle(pinned_followups):
    """A settled group of 4 x 64 x 8, one rebalance in the full form, then five follow-ups -> what each of the six withheld and
    whether it asked for another."""
    s = Scenario(7, 4, 64, 8)
    full = lambda *a: oracle.assign_flat(*a)
    first = sharding.assign_cooperative_numpy(*s.inputs(), assign=full)
    assert first[10][2] == 0 and first[10][5] == 0                       # nothing owned: nothing withheld, the group is settled
    s.obey(first[0], first[4])
    withheld, followup = [], []
    for i in range(6):
        s.grow()
        if pinned_followups and i > 0:
            target = sharding.assign_pinned_numpy(*s.inputs())
            assign = lambda *a: target[:3]
        else:
            assign = full
        r = sharding.assign_cooperative_numpy(*s.inputs(), assign=assign)
        withheld.append(int(r[10][2]))
        followup.append(int(r[10][5]))
        s.obey(r[0], r[4])
    return withheld, followup


def test_full_followups_never_settle_and_pinned_followups_settle_at_once():
    withheld, followup = _settle(False)
    assert all(w > 0 for w in withheld) and all(followup), (withheld, followup)
    first = withheld[0]
    withheld, followup = _settle(True)
    assert withheld == [first, 0, 0, 0, 0, 0] and followup == [1, 0, 0, 0, 0, 0], (withheld, followup)


@pytest.mark.parametrize("name", list(CASES))
def test_the_round_withholds_exactly_the_foreign_partitions_of_topics_with_consumers(name):
    c = CASES[name]()
    out_pid, out_rank, _, _, _ = c.expect()
    claimed = {}
    for r in range(c.m):
        for j in range(int(c.owned_off[r]), int(c.owned_off[r + 1])):
            if c.owned_topic[j] >= 0:
                claimed[(int(c.owned_topic[j]), int(c.owned_pid[j]))] = r
    expect = np.zeros(c.t, np.int64)
    for t in range(c.t):
        ranks = set(c.cons_rank[c.cons_off[t]:c.cons_off[t + 1]].tolist())
        if ranks:
            expect[t] = sum(1 for i in c.pid[c.part_off[t]:c.part_off[t + 1]].tolist() if claimed.get((t, i), -1) not in ranks | {-1})
    r = sharding.cooperative_round_numpy(c.part_off, out_pid, out_rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)
    np.testing.assert_array_equal(r[6], expect)
    assert r[7][2] == expect.sum()
