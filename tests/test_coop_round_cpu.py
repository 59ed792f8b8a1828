"""sharding.cooperative_round_numpy -- the host restatement of la_cooperative_round[_device] and the yardstick of
tests/test_coop_round_gpu.py -- against the dictionary model of coop_cases.py plus a plain stable grouping; the struct, the limits
and the symbols of the new calls against the header and the C compiler.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import sharding

from coop_cases import CoopCase, break_case, dict_model, owned_arrays, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prev_owner", "coop_rank", "kept", "fresh", "pending", "release", "topic_withheld", "summary", "member_off",
         "grouped_topic", "grouped_partition")

CASES = {
    "one entry": lambda: synthetic(1, [1], 1, owned_frac=1.0),
    "ragged": lambda: synthetic(2, np.random.default_rng(2).integers(0, 41, 120).tolist(), 7, n_stale=30, n_unmapped=9),
    "full ids": lambda: synthetic(3, [9, 0, 130, 64, 5], 3, ids="full", n_stale=11, head=4, tail=6),
    "negative ids": lambda: synthetic(4, [65, 63, 1], 12, ids="negative", n_unmapped=5, head=1),
    "nobody owns anything": lambda: synthetic(5, [30, 0, 12], 5, owned_frac=0.0),
    "no members": lambda: synthetic(7, [4, 4], 0),
    "no topics": lambda: CoopCase(np.zeros(1, np.int64), [], [], 3, *owned_arrays(3, [(0, -1, 5), (2, -1, 5)], head=2, tail=1)),
    "no entries": lambda: synthetic(8, [0, 0, 0], 4, n_stale=6),
}


def plain_grouping(c, coop):
    """Every member's list by walking the entries in order: rank -1 first, then member by member."""
    lists = [[] for _ in range(c.m + 1)]
    po = c.part_off.tolist()
    for t in range(c.t):
        for e in range(po[t], po[t + 1]):
            lists[int(coop[e]) + 1].append((t, int(c.pid[e])))
    off = np.cumsum([len(x) for x in lists]).astype(np.int64)
    flat = [x for lst in lists for x in lst]
    return off, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32)


def round_of(c):
    return sharding.cooperative_round_numpy(c.part_off, c.pid, c.rank, c.m, c.owned_off, c.owned_topic, c.owned_pid)


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_form_equals_the_dictionary_model_and_a_plain_grouping(name):
    c = CASES[name]()
    got = round_of(c)
    assert len(got) == len(NAMES)
    model = dict_model(c)
    exp = tuple(model) + plain_grouping(c, model[1])
    for k, g, e in zip(NAMES, got, exp):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (k, name))
    off, topic, pid = got[8:]
    assert off.dtype == np.int64 and topic.dtype == pid.dtype == np.int32
    assert off.size == c.m + 1 and topic.size == pid.size == c.n
    assert off[0] == (got[1] == -1).sum() and off[-1] == c.n
    np.testing.assert_array_equal(np.diff(off), got[2] + got[3])    # a member's list is what it kept plus what it got fresh


def test_the_lists_of_one_round_are_the_owned_arrays_of_the_next():
    c = CASES["ragged"]()
    first = round_of(c)
    assert first[7][2] > 0 and first[7][3] > 0
    second = sharding.cooperative_round_numpy(c.part_off, c.pid, c.rank, c.m, *first[8:])
    assert second[7][2] == 0 and second[7][3] == 0 and second[7][4] == 0 and second[7][5] == 0
    live = c.rank >= 0
    np.testing.assert_array_equal(second[1][live], c.rank[live])
    assert second[8][0] == (c.rank == -1).sum()


@pytest.mark.parametrize("bad", ["duplicate claim, two members", "owned topic T", "target rank -2", "descending owned offsets",
                                 "part_off ends short of N"])
def test_what_the_adjustment_refuses_the_round_refuses(bad):
    c = synthetic(11, [20, 30, 20], 5, owned_frac=1.0, n_unmapped=2, head=2, tail=2)
    round_of(c)
    with pytest.raises(ValueError):
        round_of(break_case(c, bad))


# ---- header, binding, library ---------------------------------------------------------------------------------------------------
def test_coop_round_args_struct_is_the_c_compilers():
    from kafka_lag_based_assignor_amd import _native as N
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [name for name, _ in N.CoopRoundArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu %d", sizeof(la_coop_round_args), LA_COOP_FORCE_TABLE);' + \
          "".join('printf(" %%zu", offsetof(la_coop_round_args, %s));' % f for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(N.CoopRoundArgs), N.LA_COOP_FORCE_TABLE] + [getattr(N.CoopRoundArgs, f).offset for f in fields]
    assert N.CoopRoundArgs.adjust.size == ctypes.sizeof(N.CoopArgs)


def test_the_four_limits_are_those_of_the_source():
    from kafka_lag_based_assignor_amd import _native as N
    csrc = os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc")
    coop, group = open(os.path.join(csrc, "la_coop.h")).read(), open(os.path.join(csrc, "la_group_small.h")).read()
    consts = {"kTailGroupM": int(re.search(r"constexpr int kTailGroupM = (\d+);", group).group(1))}

    def limit(name):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, coop)
        assert m, name
        return int(eval(m.group(1), {"__builtins__": {}}, consts))

    assert limit("kCoopSmallEntries") == N.COOP_SMALL_ENTRIES
    assert limit("kCoopSmallOwned") == N.COOP_SMALL_OWNED
    assert limit("kCoopSmallMembers") == N.COOP_SMALL_MEMBERS
    assert limit("kCoopSmallTopics") == N.COOP_SMALL_TOPICS
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    for v in (N.COOP_SMALL_ENTRIES, N.COOP_SMALL_OWNED, N.COOP_SMALL_MEMBERS, N.COOP_SMALL_TOPICS):
        assert re.search(r"<= %s\b" % "{:,}".format(v).replace(",", " "), header) or re.search(r"<= %d\b" % v, header), v


def test_both_symbols_are_declared_bound_and_exported():
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import build
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    lib = N.load()                                                   # loads without a GPU
    for name in ("la_cooperative_round_device", "la_cooperative_round"):
        assert re.search(r"\bint %s\(" % name, header) and name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes[1] == ctypes.POINTER(N.CoopRoundArgs)
    assert "#define LA_VERSION 500" in header and lib.la_version() == 500, "added without an ABI bump"
    assert callable(N.Context.cooperative_round_device) and callable(N.Context.cooperative_round)
    assert callable(sharding.cooperative_round_numpy) and "la_coop_small.hip" in build.SOURCES
    nm = shutil.which("nm")
    if nm:
        out = subprocess.check_output([nm, "-D", "--defined-only", N.LIB_PATH]).decode()
        assert " T la_cooperative_round_device" in out and " T la_cooperative_round\n" in out
