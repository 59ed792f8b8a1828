"""Who moved between two rebalances, the parts that need no device: the host restatement (sharding.assignment_moves_numpy) against
a deliberately naive dict join over the ORACLE's assignments of two workloads with one layout and different lags, the C ABI's
declarations against the binding and the built library, and the compiled ISA of csrc/la_moves.hip (hipcc cross-compiles gfx950
without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import sharding, synth
from oracle import oracle

from gpu_helpers import _batch_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_lag_based_assignor_amd", "csrc")


def two_assignments(w, seed):
    """The oracle's assignment of `w` (the PREVIOUS one) and of the same layout with every lag redrawn (the CURRENT one)."""
    rng = np.random.default_rng(seed)
    prev_pid, prev_rank, _ = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    lag2 = rng.integers(0, 1 << 40, w.n_partitions).astype(np.int64)
    cur_pid, cur_rank, _ = oracle.assign_flat(w.part_off, w.partition_id, lag2, w.cons_off, w.cons_rank)
    return (cur_pid, cur_rank), (prev_pid, prev_rank)


def naive_moves(part_off, cur, prev, n_members, rank_map=None):
    cur_pid, cur_rank = cur
    prev_pid, prev_rank = prev
    t_count = len(part_off) - 1
    owner_of = {}
    for t in range(t_count):
        for j in range(int(part_off[t]), int(part_off[t + 1])):
            key = (t, int(prev_pid[j]))
            assert key not in owner_of
            owner_of[key] = int(prev_rank[j])
    owner = np.empty(len(cur_pid), np.int32)
    topic_moved = np.zeros(t_count, np.int64)
    gained, lost = np.zeros(n_members, np.int64), np.zeros(n_members, np.int64)
    moved = to_none = from_none = 0
    for t in range(t_count):
        for i in range(int(part_off[t]), int(part_off[t + 1])):
            p = owner_of.pop((t, int(cur_pid[i])))
            q = -1 if p < 0 else (p if rank_map is None else int(rank_map[p]))
            c = int(cur_rank[i])
            owner[i] = q
            if q != c:
                moved += 1
                topic_moved[t] += 1
                if c >= 0:
                    gained[c] += 1
                else:
                    to_none += 1
                if q >= 0:
                    lost[q] += 1
                else:
                    from_none += 1
    assert not owner_of
    return (owner, topic_moved, gained, lost, moved), to_none, from_none


def _same_moves(got, exp, what=""):
    for g, e, name in zip(got[:4], exp[:4], ("prev_owner", "topic_moved", "gained", "lost")):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (name, what))
    assert got[4] == exp[4], "moved %s: %d != %d" % (what, got[4], exp[4])


def _check(w, seed, n_members, what, rank_map=None, prev_ranks=None):
    cur, prev = two_assignments(w, seed)
    if prev_ranks is not None:
        prev = (prev[0], prev_ranks(prev[1]))
    got = sharding.assignment_moves_numpy(w.part_off, cur[0], cur[1], prev[0], prev[1], n_members, rank_map)
    exp, to_none, from_none = naive_moves(w.part_off, cur, prev, n_members, rank_map)
    _same_moves(got, exp, what)
    owner, topic_moved, gained, lost, moved = got
    assert owner.dtype == np.int32 and owner.shape == (w.n_partitions,)
    assert topic_moved.dtype == gained.dtype == lost.dtype == np.int64
    assert topic_moved.shape == (w.n_topics,) and gained.shape == lost.shape == (n_members,)
    assert int(gained.sum()) + to_none == int(lost.sum()) + from_none == moved
    assert int(topic_moved.sum()) == moved
    return got


def test_restatement_against_a_dict_join_ragged_batches():
    some_moved = False
    for seed in range(4):
        w = synth.ragged(200 + seed, 50, 90, 12)
        m = int(w.cons_rank.max()) + 1 + 3
        got = _check(w, seed, m, "ragged seed %d" % seed)
        some_moved |= got[4] > 0
    assert some_moved


def test_restatement_topics_without_consumers_and_empty_topics():
    w = _batch_of([(100, 0), (50, 4), (0, 3), (900, 0), (256, 32), (7, 0), (0, 0), (33, 5)], 5)
    m = int(w.cons_rank.max()) + 1
    owner, topic_moved, _, _, _ = _check(w, 9, m, "no consumers / empty")
    assert topic_moved[0] == 0 and topic_moved[3] == 0 and topic_moved[2] == 0          # -1 -> -1 is no move
    assert (owner[:100] == -1).all()


def test_restatement_rank_map_with_members_that_left_and_members_that_joined():
    w = synth.ragged(77, 40, 120, 10)
    m_prev = int(w.cons_rank.max()) + 1
    # the previous membership had m_prev ranks; a third of them left, the rest keep their order with new members interleaved
    rank_map = np.full(m_prev, -1, np.int32)
    stay = [r for r in range(m_prev) if r % 3 != 1]
    rank_map[stay] = np.arange(len(stay), dtype=np.int32) * 2 + 1           # new ranks 0, 2, 4, ... belong to members that joined
    m = 2 * len(stay) + 1
    cur, prev = two_assignments(w, 3)
    # the current assignment's ranks are today's: those of the members that stayed, spread over the new numbering
    remap = np.arange(m_prev, dtype=np.int32) * m // m_prev
    cur = (cur[0], np.where(cur[1] < 0, -1, remap[np.maximum(cur[1], 0)]).astype(np.int32))
    got = sharding.assignment_moves_numpy(w.part_off, cur[0], cur[1], prev[0], prev[1], m, rank_map)
    exp, to_none, from_none = naive_moves(w.part_off, cur, prev, m, rank_map)
    _same_moves(got, exp, "rank map")
    assert from_none > 0, "entries whose owner left"
    assert int(got[2].sum()) + to_none == int(got[3].sum()) + from_none == got[4]
    left = np.flatnonzero(rank_map < 0)
    assert np.isin(prev[1], left).any() and not got[3][::2].any()           # nobody loses on behalf of a rank that did not exist
    # the identity map is the NULL map
    ident = sharding.assignment_moves_numpy(w.part_off, cur[0], cur[1], prev[0], prev[1], m_prev + m,
                                            np.arange(m_prev + m, dtype=np.int32))
    plain = sharding.assignment_moves_numpy(w.part_off, cur[0], cur[1], prev[0], prev[1], m_prev + m)
    _same_moves(ident, plain, "identity map")


def test_identical_assignments_do_not_move():
    w = synth.ragged(5, 30, 200, 20)
    pid, rank, _ = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    m = int(w.cons_rank.max()) + 1
    owner, topic_moved, gained, lost, moved = sharding.assignment_moves_numpy(w.part_off, pid, rank, pid, rank, m)
    assert moved == 0 and not topic_moved.any() and not gained.any() and not lost.any()
    np.testing.assert_array_equal(owner, rank)
    # ... also when the previous side comes in another order
    rng = np.random.default_rng(1)
    order = np.concatenate([w.part_off[t] + rng.permutation(int(w.part_off[t + 1] - w.part_off[t])) for t in range(w.n_topics)])
    got = sharding.assignment_moves_numpy(w.part_off, pid, rank, pid[order], rank[order], m)
    assert got[4] == 0
    np.testing.assert_array_equal(got[0], rank)


def test_restatement_edge_cases_and_every_value_error():
    e32 = np.empty(0, np.int32)
    owner, topic_moved, gained, lost, moved = sharding.assignment_moves_numpy(np.zeros(1, np.int64), e32, e32, e32, e32, 3)
    assert owner.size == 0 and topic_moved.size == 0 and gained.tolist() == [0, 0, 0] and lost.tolist() == [0, 0, 0] and moved == 0
    got = sharding.assignment_moves_numpy(np.zeros(4, np.int64), e32, e32, e32, e32, 0)
    assert got[1].tolist() == [0, 0, 0] and got[2].size == 0 and got[4] == 0
    po = np.array([0, 3, 5], np.int64)
    ids = np.array([7, -1, np.iinfo(np.int32).min, 4, 7], np.int32)
    rk = np.array([0, 1, 2, -1, 1], np.int32)
    ok = sharding.assignment_moves_numpy(po, ids, rk, ids[[2, 0, 1, 4, 3]], rk, 3)
    np.testing.assert_array_equal(ok[0], [1, 2, 0, 1, -1])
    assert ok[4] == 5 and ok[1].tolist() == [3, 2] and ok[2].tolist() == [1, 2, 1] and ok[3].tolist() == [1, 2, 1]

    def call(cur_id=ids, cur_rk=rk, prev_id=ids, prev_rk=rk, m=3, rank_map=None):
        return sharding.assignment_moves_numpy(po, cur_id, cur_rk, prev_id, prev_rk, m, rank_map)

    def with_(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    bad = {
        "duplicate id, previous": dict(prev_id=with_(ids, 1, 7)),
        "duplicate id, current": dict(cur_id=with_(ids, 4, 4)),
        "duplicate id, both": dict(prev_id=with_(ids, 1, 7), cur_id=with_(ids, 1, 7)),
        "foreign id": dict(cur_id=with_(ids, 3, 99)),
        "current rank M": dict(cur_rk=with_(rk, 0, 3)),
        "current rank -2": dict(cur_rk=with_(rk, 0, -2)),
        "previous rank M": dict(prev_rk=with_(rk, 2, 3)),
        "previous rank -2": dict(prev_rk=with_(rk, 2, -2)),
        "previous rank M_prev with a map": dict(rank_map=np.array([0, 1], np.int32)),
        "map entry M": dict(rank_map=np.array([0, 3, 1], np.int32)),
        "map entry -2": dict(rank_map=np.array([0, -2, 1], np.int32)),
        "negative M": dict(m=-1),
        "short array": dict(cur_rk=rk[:4]),
    }
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        sharding.assignment_moves_numpy(np.array([0, 3, 2], np.int64), ids[:2], rk[:2], ids[:2], rk[:2], 3)
    # the same id in two topics is no duplicate; a map entry of -1 is a member that left
    assert call(rank_map=np.array([0, -1, 1, 2], np.int32))[0].tolist() == [0, -1, 1, -1, -1]


NEW_SYMBOLS = ("la_assignment_moves_device", "la_assignment_moves_device_on")


def test_header_binding_and_library_agree():
    from kafka_lag_based_assignor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "lagassign.h")).read()
    assert re.search(r"^int la_assignment_moves_device\(la_ctx \*ctx, const la_moves_args \*args, void \*stream\);", header, re.M)
    assert re.search(r"^int la_assignment_moves_device_on\(la_ctx \*ctx, int shard, const la_moves_args \*args, void \*stream\);",
                     header, re.M)
    for name in NEW_SYMBOLS:
        assert name in N.EXPORTED_SYMBOLS
    assert "#define LA_VERSION 500" in header
    lib = N.load()                                                   # loads without a GPU
    assert lib.la_version() == 500
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert callable(N.Context.assignment_moves_device)
    from kafka_lag_based_assignor_amd import build
    assert "la_moves.hip" in build.SOURCES


def test_exported_limits_are_the_kernels_constants():
    from kafka_lag_based_assignor_amd import _native as N
    kernels = open(os.path.join(CSRC, "la_kernels.h")).read()
    m = re.search(r"constexpr int64_t kMovesLdsMaxPartitions = (\d+);", kernels)
    assert m and int(m.group(1)) == N.MOVES_LDS_MAX_PARTITIONS
    m = re.search(r"constexpr int32_t kMovesLdsMaxMembers = (\d+);", kernels)
    assert m and int(m.group(1)) == N.MOVES_LDS_MAX_MEMBERS
    # the widest table (2 x the limit, 8 bytes a slot) and one copy of the widest bins (2 M counters) fit a gfx950 workgroup's LDS
    assert 16 * N.MOVES_LDS_MAX_PARTITIONS + 8 * N.MOVES_LDS_MAX_MEMBERS + 16 <= 160 * 1024
    bit = re.search(r"constexpr uint32_t kStatusMoves = (\d+)u;", kernels)
    others = [int(x) for x in re.findall(r"constexpr uint32_t kStatus(?!Moves)\w+ = (\d+)u;", kernels)]
    assert bit and int(bit.group(1)) == 2 * max(others), "the next free status bit"


def test_moves_args_struct_is_the_c_compilers():
    from kafka_lag_based_assignor_amd import _native as N
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ("n_partitions", "d_part_off", "h_part_off", "d_prev_member_rank", "n_members", "n_prev_members", "d_prev_rank_map",
              "d_prev_owner", "d_moved")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lagassign.h"\nint main(void){printf("%zu", sizeof(la_moves_args));\n' + \
          "".join('printf(" %%zu", offsetof(la_moves_args, %s));\n' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(N.MovesArgs)] + [getattr(N.MovesArgs, f).offset for f in fields]
    assert [f for f, _ in N.MovesArgs._fields_] == re.findall(
        r"^\s+(?:const )?int(?:32|64)_t \*?(\w+);", re.search(r"typedef struct la_moves_args \{(.*?)\} la_moves_args;",
                                                            open(os.path.join(ROOT, "include", "lagassign.h")).read(), re.S).group(1), re.M)


@pytest.fixture(scope="module")
def moves_isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = os.path.join(str(tmp_path_factory.mktemp("isa")), "la_moves.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst,
                           os.path.join(CSRC, "la_moves.hip")], stderr=subprocess.DEVNULL)
    return open(dst).read()


def _instructions(text):
    return re.findall(r"^\s+([a-z][a-z0-9_]+)\b", text, re.M)


def test_isa_the_probing_routine_is_lds_and_global_atomics(moves_isa):
    ins = _instructions(moves_isa)
    assert any(i == "ds_cmpst_rtn_b64" for i in ins), "LDS 64-bit compare-and-swap (insert)"
    assert any(i == "ds_or_rtn_b64" for i in ins), "LDS 64-bit atomic OR (the matched mark)"
    assert any(i.startswith("global_atomic_cmpswap_x2") for i in ins), "the same insert on the table in device memory"
    assert any(i.startswith("global_atomic_add_x2") for i in ins), "64-bit global atomic add"
    assert any(i in ("ds_add_u32", "ds_add_rtn_u32") for i in ins), "32-bit LDS bins"
    assert not [i for i in ins if i.startswith("flat_")], "a pointer the compiler could not place"


def test_isa_no_kernel_of_the_unit_uses_scratch(moves_isa):
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", moves_isa)
    assert len(sizes) == 5, "moves_lds_kernel<bins>, moves_global_kernel<insert>, <lookup, bins>: %s" % sizes
    assert all(int(s) == 0 for s in sizes), sizes
    assert not [i for i in _instructions(moves_isa) if i.startswith("scratch_")]
