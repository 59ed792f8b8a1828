"""la_assignment_moves_device with a layout per assignment (d_prev_part_off), the parts that need no device: the host restatement
(sharding.assignment_moves_layouts_numpy) against a deliberately naive per-topic dict join, the one-layout restatement where the
layouts are equal, the conservation of every member's holdings, sharding.prev_topic_map, the header's new fields against the
binding and the C compiler, and the compiled ISA of csrc/la_moves_layouts.hip (hipcc cross-compiles gfx950 without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import sharding

from moves_layouts_cases import LCase, build, naive, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "lagassign.h")

# grown, shrunk, new (None), emptied and deleted-today (P = 0) topics, equal ones, disjoint ones
PAIRS = [(40, 56), (56, 40), (None, 30), (25, 0), (0, 25), (0, 0), (64, 64), (30, 30, "disjoint"), (17, 17, "half"), (1, 1),
         (None, 0), (3, 400), (400, 3), (90, 91, "half")]


def _left_map(m_prev):
    """A third of the previous members left; the others keep their order, new members interleaved -> (map, M)."""
    rank_map = np.full(m_prev, -1, np.int32)
    stay = [r for r in range(m_prev) if r % 3 != 1]
    rank_map[stay] = np.arange(len(stay), dtype=np.int32) * 2 + 1
    return rank_map, 2 * len(stay) + 1


def _holdings(ranks, m):
    ranks = np.asarray(ranks, np.int64)
    return np.bincount(ranks[ranks >= 0], minlength=m).astype(np.int64)[:m]


def _conserved(c, got):
    """now(r) = before(r) + gained[r] - lost[r], before(r): the mapped owners over the previous topics that are named."""
    before = np.zeros(c.m, np.int64)
    for t in range(c.t):
        q0, nq = c.segment_of(t)
        p = c.prev_rank[q0:q0 + nq].astype(np.int64)
        q = p if c.rank_map is None else np.where(p < 0, -1, c.rank_map[np.maximum(p, 0)])
        before += _holdings(q, c.m)
    np.testing.assert_array_equal(_holdings(c.cur_rank, c.m), before + got[4] - got[5])
    assert got[6] == int(got[1].sum()) and got[7] == int(got[2].sum()) and got[8] == int(got[3].sum())
    assert c.n - got[7] == sum(c.segment_of(t)[1] for t in range(c.t)) - got[8], "matched entries, counted from either side"


def test_restatement_against_a_dict_join():
    seen = np.zeros(3, np.int64)
    for seed in range(6):
        rank_map, m = (None, 11) if seed % 2 == 0 else _left_map(15)
        c = build(seed, PAIRS, m, ids=("shuffled", "full", "4096")[seed % 3], m_prev=None if rank_map is None else 15,
                  rank_map=rank_map, topic_map="permute", extra_prev=(12, 0, 5))
        got = c.expect()
        same(got, naive(c), "seed %d" % seed)
        assert got[0].dtype == np.int32 and got[0].shape == (c.n,)
        assert all(a.dtype == np.int64 for a in got[1:6]) and got[1].shape == got[2].shape == got[3].shape == (c.t,)
        assert got[4].shape == got[5].shape == (c.m,)
        _conserved(c, got)
        seen += np.array(got[6:9])
        new = np.flatnonzero(c.prev_topic < 0)
        assert new.size == 2 and (got[2][new] == np.diff(c.part_off)[new]).all(), "every partition of a new topic is added"
        assert got[3][3] == 25 and got[2][4] == 25, "an emptied topic is all removed, a filled one all added"
        if rank_map is not None:
            assert not got[5][::2].any(), "nobody loses on behalf of a rank that did not exist"
    assert (seen > 0).all()


def test_identity_map_is_no_map_and_a_permuted_previous_layout_changes_nothing():
    pairs = [p for p in PAIRS if p[0] is not None]
    a = build(3, pairs, 9)
    b = build(3, pairs, 9, topic_map="same")
    same(b.expect(), a.expect(), "identity map")
    same(a.expect(), naive(a), "no map")
    # the previous segments in another order, unreferenced topics among them: the same numbers
    order = np.random.default_rng(0).permutation(a.t)
    segs = [a.segment_of(t) for t in order]
    ppo = np.concatenate([[0], np.cumsum([n for _, n in segs])])
    pick = np.concatenate([np.arange(q0, q0 + n) for q0, n in segs])
    moved_about = LCase(a.part_off, a.cur_pid, a.cur_rank, ppo, a.prev_pid[pick], a.prev_rank[pick], a.m, None, np.argsort(order))
    same(moved_about.expect(), a.expect(), "permuted previous layout")


def test_equal_layouts_reproduce_the_one_layout_restatement():
    for seed, (rank_map, m) in enumerate([(None, 7), _left_map(12)]):
        c = build(seed, [(p, p) for p in (50, 1, 0, 300, 64, 17)], m, ids="full", m_prev=None if rank_map is None else 12,
                  rank_map=rank_map)
        one = sharding.assignment_moves_numpy(c.part_off, c.cur_pid, c.cur_rank, c.prev_pid, c.prev_rank, m, rank_map)
        got = c.expect()
        same((got[0], got[1], got[4], got[5], got[6]), one, "equal layouts")
        assert got[7] == 0 and got[8] == 0 and not got[2].any() and not got[3].any()
        assert (got[0] != sharding.MOVES_NO_PREVIOUS).all()


def test_empty_sides():
    e = np.empty(0, np.int32)
    z1, z4 = np.zeros(1, np.int64), np.zeros(4, np.int64)
    got = LCase(z1, e, e, z1, e, e, 3).expect()                                     # T == 0
    assert got[0].size == 0 and got[1].size == 0 and got[4].tolist() == [0, 0, 0] and got[6:] == (0, 0, 0)
    got = LCase(z4, e, e, z4, e, e, 0).expect()                                     # N == 0 and N_prev == 0
    assert got[1].tolist() == got[2].tolist() == got[3].tolist() == [0, 0, 0] and got[4].size == 0
    ids, rk = np.array([5, 6, 7], np.int32), np.array([0, -1, 1], np.int32)
    po = np.array([0, 3], np.int64)
    got = LCase(z1[:1].repeat(2), e, e, po, ids, rk, 2).expect()                    # N == 0: everything removed
    assert got[0].size == 0 and got[3].tolist() == [3] and got[5].tolist() == [1, 1] and got[6:] == (0, 0, 3)
    got = LCase(po, ids, rk, z1[:1].repeat(2), e, e, 2).expect()                    # N_prev == 0: everything added
    assert got[0].tolist() == [-2, -2, -2] and got[2].tolist() == [3] and got[4].tolist() == [1, 1] and got[6:] == (0, 3, 0)
    got = LCase(z1, e, e, po, ids, rk, 2, prev_topic=e).expect()                    # T == 0 over a previous layout: not looked at
    assert got[6:] == (0, 0, 0) and not got[5].any()


def test_every_value_error():
    po, ppo = np.array([0, 3, 5], np.int64), np.array([0, 2, 6], np.int64)
    ids, rk = np.array([7, -1, I32_MIN, 4, 7], np.int32), np.array([0, 1, 2, -1, 1], np.int32)
    pids, prk = np.array([7, 9, 4, 5, 6, I32_MIN], np.int32), np.array([2, 2, 0, -1, 1, 1], np.int32)
    ok = sharding.assignment_moves_layouts_numpy(po, ids, rk, ppo, pids, prk, 3)
    assert ok[0].tolist() == [2, -2, -2, 0, -2] and ok[6:] == (2, 3, 4)
    assert ok[1].tolist() == [1, 1] and ok[2].tolist() == [2, 1] and ok[3].tolist() == [1, 3]
    assert ok[4].tolist() == [1, 2, 1] and ok[5].tolist() == [1, 2, 2]

    def call(po=po, cur_id=ids, cur_rk=rk, ppo=ppo, prev_id=pids, prev_rk=prk, m=3, rank_map=None, prev_topic=None):
        return sharding.assignment_moves_layouts_numpy(po, cur_id, cur_rk, ppo, prev_id, prev_rk, m, rank_map, prev_topic)

    def with_(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    bad = {
        "duplicate id, previous": dict(prev_id=with_(pids, 3, 4)),
        "duplicate id, current": dict(cur_id=with_(ids, 1, 7)),
        "duplicate id, current, among the added": dict(cur_id=with_(ids, 2, -1)),
        "current rank M": dict(cur_rk=with_(rk, 0, 3)),
        "current rank -2": dict(cur_rk=with_(rk, 0, -2)),
        "previous rank M": dict(prev_rk=with_(prk, 2, 3)),
        "previous rank -2": dict(prev_rk=with_(prk, 2, -2)),
        "previous rank M_prev with a map": dict(rank_map=np.array([0, 1], np.int32)),
        "map entry M": dict(rank_map=np.array([0, 3, 1], np.int32)),
        "map entry -2": dict(rank_map=np.array([0, -2, 1], np.int32)),
        "topic map entry T_prev": dict(prev_topic=np.array([0, 2], np.int32)),
        "topic map entry -2": dict(prev_topic=np.array([-2, 1], np.int32)),
        "topic map of another length": dict(prev_topic=np.array([0], np.int32)),
        "a previous topic named twice": dict(prev_topic=np.array([1, 1], np.int32)),
        "no map and T_prev != T": dict(ppo=np.array([0, 2, 6, 6], np.int64)),
        "negative M": dict(m=-1),
        "short current array": dict(cur_rk=rk[:4]),
        "short previous array": dict(prev_id=pids[:5]),
        "offsets descend": dict(po=np.array([0, 6, 5], np.int64)),
        "previous offsets do not start at 0": dict(ppo=np.array([1, 2, 6], np.int64)),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            call(**kw)
    # the same id in two topics is no duplicate; what an unreferenced previous topic holds is not looked at
    assert call(prev_topic=np.array([-1, 1], np.int32), prev_id=with_(pids, 1, 7), prev_rk=with_(prk, 0, 99))[6:] == (1, 4, 3)
    assert call(rank_map=np.array([0, -1, 1, 2], np.int32), prev_rk=with_(prk, 0, 1))[0].tolist() == [-1, -2, -2, 0, -2]


I32_MIN = np.iinfo(np.int32).min


def test_prev_topic_map():
    got = sharding.prev_topic_map(["a", "b", "c", "d"], ["c", "new", "a", "d"])
    assert got.dtype == np.int32 and got.tolist() == [2, -1, 0, 3]
    assert sharding.prev_topic_map([], ["x"]).tolist() == [-1]
    assert sharding.prev_topic_map(["x"], []).shape == (0,)
    for prev, cur in ((["a", "a"], ["a"]), (["a"], ["b", "b"])):
        with pytest.raises(ValueError):
            sharding.prev_topic_map(prev, cur)


NEW_FIELDS = ("n_prev_topics", "reserved", "n_prev_partitions", "d_prev_part_off", "h_prev_part_off", "d_prev_topic", "h_prev_topic",
              "d_topic_added", "d_topic_removed", "d_added", "d_removed")


def test_header_and_binding_declare_the_new_fields():
    from kafka_lag_based_assignor_amd import _native as N
    from kafka_lag_based_assignor_amd import build as la_build
    header = open(HEADER).read()
    assert re.search(r"^#define LA_MOVES_NO_PREVIOUS \(-2\)$", header, re.M)
    assert N.LA_MOVES_NO_PREVIOUS == sharding.MOVES_NO_PREVIOUS == -2
    body = re.search(r"typedef struct la_moves_args \{(.*?)\} la_moves_args;", header, re.S).group(1)
    declared = re.findall(r"^\s+((?:const )?int(?:32|64)_t \*?)(\w+);", body, re.M)
    assert [n for _, n in declared][-len(NEW_FIELDS):] == list(NEW_FIELDS)
    assert [n for _, n in declared].index("n_prev_topics") == [n for _, n in declared].index("d_moved") + 1
    types = dict((n, t) for t, n in declared)
    assert types["d_prev_part_off"] == types["h_prev_part_off"] == "const int64_t *"
    assert types["d_prev_topic"] == types["h_prev_topic"] == "const int32_t *"
    assert types["d_topic_added"] == types["d_topic_removed"] == types["d_added"] == types["d_removed"] == "int64_t *"
    assert types["n_prev_topics"] == types["reserved"] == "int32_t " and types["n_prev_partitions"] == "int64_t "
    assert [f for f, _ in N.MovesArgs._fields_][-len(NEW_FIELDS):] == list(NEW_FIELDS)
    assert N.MovesArgs.n_prev_topics.offset == 128, "the one-layout struct ends where the new fields begin"
    assert "#define LA_VERSION 500" in header
    assert "la_moves_layouts.hip" in la_build.SOURCES and "la_moves.hip" in la_build.SOURCES
    assert not N.MovesArgs().d_prev_part_off, "an args struct that sets nothing new asks for the one-layout form"


def test_new_fields_sit_where_the_c_compiler_puts_them():
    from kafka_lag_based_assignor_amd import _native as N
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_moves_args));\n' + \
          "".join('printf(" %%zu", offsetof(la_moves_args, %s));\n' % f for f in NEW_FIELDS) + \
          'printf(" %d", LA_MOVES_NO_PREVIOUS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(N.MovesArgs)] + [getattr(N.MovesArgs, f).offset for f in NEW_FIELDS] + [-2]


@pytest.fixture(scope="module")
def layouts_isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = os.path.join(str(tmp_path_factory.mktemp("isa")), "la_moves_layouts.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                           os.path.join(CSRC, "la_moves_layouts.hip")], stderr=subprocess.DEVNULL)
    return open(dst).read()


def _instructions(text):
    return re.findall(r"^\s+([a-z][a-z0-9_]+)\b", text, re.M)


def test_isa_the_unit_compiles_for_gfx950_without_scratch_or_flat_accesses(layouts_isa):
    assert ".amdgcn_target" in layouts_isa and "gfx950" in layouts_isa
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", layouts_isa)
    assert len(sizes) == 7, "moves_layouts_lds_kernel<bins>, moves_layouts_global_kernel<insert>, <lookup, bins>, <sweep, bins>: %s" % sizes
    assert all(int(s) == 0 for s in sizes), sizes
    ins = _instructions(layouts_isa)
    assert not [i for i in ins if i.startswith("scratch_")]
    assert not [i for i in ins if i.startswith("flat_")], "a pointer the compiler could not place"
    assert any(i == "ds_cmpst_rtn_b64" for i in ins) and any(i == "ds_or_rtn_b64" for i in ins), "la_join.h's insert and lookup, in LDS"
    assert any(i.startswith("global_atomic_cmpswap_x2") for i in ins), "... and on the table in device memory"
