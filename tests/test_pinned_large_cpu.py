"""The pinned assignment for topics of any size on the host: sharding.assign_pinned_numpy(max_partitions=PINNED_ANY_SIZE), the
yardstick of tests/test_pinned_large_gpu.py, against the dictionary model with its limit lifted; the settling scenario over a
topic of 4097 partitions, which is the reason for the large form; the host mirror's new key.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native, sharding
from oracle import oracle

import pinned_large_cases as PL
from pinned_cases import Scenario, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numpy_form(c, **kw):
    return sharding.assign_pinned_numpy(*c.args(), max_partitions=sharding.PINNED_ANY_SIZE, **kw)


def test_the_constants_are_the_c_compilers():
    src = ('#include <stdio.h>\n#include "lagassign.h"\nint main(void){printf("%d %d %d %d", LA_FLAG_PINNED_LARGE, LA_COOP_PINNED_LARGE, '
           'LA_PINNED_LARGE_MAX_PARTITIONS, LA_PINNED_LARGE_LAUNCHES);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [_native.LA_FLAG_PINNED_LARGE, _native.LA_COOP_PINNED_LARGE, _native.PINNED_LARGE_MAX_PARTITIONS,
                   _native.PINNED_LARGE_LAUNCHES]
    assert sharding.PINNED_ANY_SIZE == _native.PINNED_LARGE_MAX_PARTITIONS == PL.ANY_SIZE
    flags = [v for k, v in vars(_native).items() if k.startswith("LA_FLAG_") and isinstance(v, int)]
    assert len(set(flags)) == len(flags), "two LA_FLAG_ bits share a value"


@pytest.mark.parametrize("name", list(PL.CASES))
def test_numpy_with_the_limit_lifted_equals_the_dictionary_model(name):
    c, exp = PL.case(name)
    assert PL.is_large(c).any()
    same(numpy_form(c), exp, name)


def test_the_default_limit_is_unchanged_at_4097():
    c, _ = PL.case("one past")
    with pytest.raises(ValueError):
        sharding.assign_pinned_numpy(*c.args())
    with pytest.raises(ValueError):
        c.expect()
    got = sharding.assign_pinned_numpy(*c.args(), strict=False)
    assert not got[0].any() and not got[1].any() and not got[3].any() and got[4][:3].tolist() == [0, 0, 0]


def test_the_consumer_limit_stays():
    c = PL.OVER_CONSUMERS()
    with pytest.raises(ValueError):
        numpy_form(c)
    got = numpy_form(c, strict=False)
    p1, c1 = int(c.part_off[1]), int(c.cons_off[1])
    assert not got[0][p1:].any() and not got[2][c1:].any() and got[3][1] == 0
    keep = c.owned_topic == 0
    alone = sharding.assign_pinned_numpy([0, p1], c.pid[:p1], c.lag[:p1], [0, c1], c.cons_rank[:c1], c.m, c.owned_off,
                                         np.where(keep, 0, -1), c.owned_pid, max_partitions=sharding.PINNED_ANY_SIZE)
    np.testing.assert_array_equal(got[0][:p1], alone[0])
    np.testing.assert_array_equal(got[1][:p1], alone[1])
    np.testing.assert_array_equal(got[2][:c1], alone[2])


def test_with_nothing_owned_it_is_the_reference_assignment():
    c, exp = PL.case("nothing owned")
    e_pid, e_rank, e_tot = oracle.assign_flat(c.part_off, c.pid, c.lag, c.cons_off, c.cons_rank)
    np.testing.assert_array_equal(exp[0], e_pid)
    np.testing.assert_array_equal(exp[1], e_rank)
    np.testing.assert_array_equal(exp[2], e_tot)
    np.testing.assert_array_equal(exp[3], np.diff(c.part_off))


def test_the_lone_consumer_cases_reach_both_ends_of_the_run():
    for name, free, first_run in (("lone consumer: the run ends at m2", 560, 520), ("lone consumer: the run ends at F", 300, 300)):
        c, exp = PL.case(name)
        assert exp[3].tolist() == [free]
        free_ranks = exp[1][np.isin(exp[0], c.owned_pid, invert=True)]      # in position order
        assert (free_ranks[:first_run] == 0).all() and (free_ranks == 0).sum() == first_run + (free - first_run + 7) // 8


def _settle(pinned_followups):
    """Scenario(7, 1, 4097, 3): a settled group, one rebalance in the full form, then three follow-ups -> what each of the four
    withheld and whether it asked for another."""
    s = Scenario(7, 1, 4097, 3)
    full = lambda *a: oracle.assign_flat(*a)
    first = sharding.assign_cooperative_numpy(*s.inputs(), assign=full)
    assert first[10][2] == 0 and first[10][5] == 0
    s.obey(first[0], first[4])
    withheld, followup = [], []
    for i in range(4):
        s.grow()
        if pinned_followups and i > 0:
            target = sharding.assign_pinned_numpy(*s.inputs(), max_partitions=sharding.PINNED_ANY_SIZE)
            assign = lambda *a: target[:3]
        else:
            assign = full
        r = sharding.assign_cooperative_numpy(*s.inputs(), assign=assign)
        withheld.append(int(r[10][2]))
        followup.append(int(r[10][5]))
        s.obey(r[0], r[4])
    return withheld, followup


def test_over_4096_partitions_full_followups_never_settle_and_pinned_followups_settle_at_once():
    withheld, followup = _settle(False)
    assert all(w > 0 for w in withheld) and all(followup), (withheld, followup)
    first = withheld[0]
    withheld, followup = _settle(True)
    assert withheld == [first, 0, 0, 0] and followup == [1, 0, 0, 0], (withheld, followup)


def test_the_mirrors_key_is_parsed_and_rejected():
    from kafka_lag_based_assignor_amd.assignor import LagBasedPartitionAssignor
    a = LagBasedPartitionAssignor()
    a.configure({"group.id": "g"})
    assert a.cooperative_followup_large() is False
    for v, want in (("true", True), ("TRUE", True), (True, True), ("false", False), (False, False)):
        a.configure({"group.id": "g", "lag.assignor.cooperative.followup": "pinned", "lag.assignor.cooperative.followup.large": v})
        assert a.cooperative_followup_large() is want and a.cooperative_followup() == "pinned"
    a.configure({"group.id": "g", "lag.assignor.cooperative.followup.large": "true"})      # alone: read, and without effect
    assert a.cooperative_followup_large() is True and a.cooperative_followup() == "full"
    for bad in ("yes", "1", "", "pinned"):
        with pytest.raises(ValueError):
            LagBasedPartitionAssignor().configure({"group.id": "g", "lag.assignor.cooperative.followup.large": bad})


def test_the_library_knows_the_flag_by_its_constants():
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "la_assign_pinned_device")
    sig = __import__("inspect").signature(_native.Context.assign_batch_cooperative)
    assert "pinned_large" in sig.parameters
