"""What the report calls share on the host side (csrc/la_launch.h): the per-kernel cache of resident workgroups, which remembers
the LAST (workgroup size, LDS bytes) request only, and the staged topic list of a global form, which grows and is reused.  Each
test makes one context's calls in an order that a stale cache word or a stale list would turn into wrong numbers or a launch
failure: a small LDS request behind a large one, a short list behind a long one, the two kernels of a bins / no-bins pair at ONE
LDS byte count.  Every call is checked like any other call of its feature: against the CPU model its own tests use, bit for
bit, on guarded buffers (the Run classes of those tests)."""
import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import sharding

import coop_cases
import verify_cases as V
import verify_large_cases as VL
from moves_layouts_cases import NAMES as LAYOUTS_OUTPUTS, build as layouts_case
from test_coop_gpu import Run as CoopRun
from test_member_loads_gpu import Outs, _dev, _same_loads, _synthetic as loads_case
from test_moves_gpu import OUTPUTS as MOVES_OUTPUTS, Run as MovesRun, synthetic as moves_case
from test_moves_layouts_gpu import Run as LayoutsRun
from test_verify_gpu import Run as VerifyRun
from test_verify_large_gpu import LargeRun

pytestmark = pytest.mark.gpu

L = N.MOVES_LDS_MAX_PARTITIONS
ABA = (0, 1, 0)                         # a request, another one, the first again: the cache holds the other one by then


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


# ---- alternating LDS requests on one context -------------------------------------------------------------------------------------
def test_moves_with_alternating_hints(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = moves_case(41, [64, 1, 63, 0, 17, 64, 33] * 9, 12)
    exp = c.expect()
    for hint in (64, L, 64):
        r = MovesRun(ctx, c, stream, hint=hint)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(exp, "hint %d" % hint)


def test_moves_layouts_with_alternating_hints(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    c = layouts_case(42, [(64, 60), (0, 64), (64, 0), (33, 64, "half"), (1, 1), (64, 64, "disjoint")] * 6, 12)
    exp = c.expect()
    for hint in (64, L, 64):
        r = LayoutsRun(ctx, c, stream, hint=hint)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(exp, "hint %d" % hint)


def test_verify_with_alternating_hints_and_workgroup_sizes(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    w = V.batch([(64, 8), (63, 64), (1, 1), (0, 3), (64, 5), (40, 0), (17, 31)] * 5, 43)
    res = V.oracle_result(w)
    for hint in ((64, 64), (V.LIMIT, V.LIMIT), (64, 64)):       # 64 partitions: one wavefront per topic; 4096: four
        r = VerifyRun(ctx, w, res, stream, hint=hint)
        ctx.sync(stream)
        assert r.launches == 1
        got_v, got_s = r.check("hint %s" % (hint,))
        assert not got_v.any() and list(got_s) == [0, 0, -1, -1]


def test_member_loads_with_alternating_member_counts(ctx, torch_dev):
    torch, _ = torch_dev
    stream = _stream(torch)
    for m in (3, N.LOADS_LDS_MAX_MEMBERS, 3):
        rank, cons_rank, total = loads_case(44 + m, 5003, 1501, m)
        exp = sharding.member_loads_numpy(rank, cons_rank, total, m)
        d_rank, d_cr, d_tot = _dev(torch, rank), _dev(torch, cons_rank), _dev(torch, total)
        outs = Outs(torch, m)
        torch.cuda.synchronize()
        ctx.member_loads_device(rank.size, d_rank.data_ptr(), cons_rank.size, d_cr.data_ptr(), d_tot.data_ptr(), m,
                                outs.parts.data_ptr(), outs.lag.data_ptr(), outs.un.data_ptr(), stream=stream)
        assert ctx.last_launches() == 1
        ctx.sync(stream)
        _same_loads(outs.numpy(), exp, "M = %d" % m)


def test_cooperative_adjust_with_alternating_member_counts(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    for m in (3, N.MOVES_LDS_MAX_MEMBERS, 3):
        c = coop_cases.synthetic(45 + m, [700, 0, 33, 1500, 64, 900], m, n_stale=9, n_unmapped=3, head=2, tail=1)
        r = CoopRun(ctx, c, stream)
        ctx.sync(stream)
        assert r.launches == N.COOP_MAX_LAUNCHES
        r.check(what="M = %d" % m)


# ---- the staged list of a global form grows and shrinks ----------------------------------------------------------------------------
def test_moves_topic_list_of_one_three_and_one_large_topics(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    cases = [moves_case(50 + k, [L + 1] * k, 9, ids="full") for k in (1, 3)]
    for i in ABA:
        r = MovesRun(ctx, cases[i], stream)
        ctx.sync(stream)
        assert r.launches == 2
        r.check(what="%d large topics" % cases[i].t)


def test_moves_layouts_pair_list_of_one_three_and_one_large_pairs(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    cases = [layouts_case(52 + k, [(L + 1, L + 1, "half")] * k, 9, ids="full") for k in (1, 3)]
    for i in ABA:
        r = LayoutsRun(ctx, cases[i], stream)
        ctx.sync(stream)
        assert r.launches == 4                                       # the LDS form for the map entries, then three phases
        r.check(what="%d large pairs" % cases[i].t)


def test_verify_large_topic_list_of_one_three_and_one_large_topics(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    batches = [VL.batch([(L + 1, 8)] * k, 54 + k) for k in (1, 3)]
    for i in ABA:
        w = batches[i]
        r = LargeRun(ctx, w, V.oracle_result(w), stream)
        ctx.sync(stream)
        assert r.launches == N.VERIFY_MAX_LAUNCHES
        got_v, got_s = r.check("%d large topics" % w.n_topics)
        assert not got_v.any() and list(got_s) == [0, 0, -1, -1]


# ---- both kernels of a bins / no-bins pair at one LDS byte count -------------------------------------------------------------------
# 255 members with a hint of 1: a table of 2 slots, four copies of 511 bins -- 16 + 8176 bytes.  No bins with a hint of 512: a
# table of 1024 slots -- 8192 bytes.  Behind them both forms add the same few bytes of counters, so the two kernels ask for the
# same LDS one after the other, and a cache that did not tell them apart would answer the second with the first's residency.
M_TWIN, HINT_BINS, HINT_PLAIN = 255, 1, 512


def test_moves_bins_and_no_bins_kernels_at_one_lds_size(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    binned = moves_case(60, [1] * 700, M_TWIN)
    plain = moves_case(61, [512, 1, 300, 0, 511] * 8, M_TWIN)
    assert binned.hint == HINT_BINS and plain.hint == HINT_PLAIN
    no_bins = tuple(k for k in MOVES_OUTPUTS if k not in ("gained", "lost"))
    for case, want in ((binned, MOVES_OUTPUTS), (plain, no_bins), (binned, MOVES_OUTPUTS)):
        r = MovesRun(ctx, case, stream, want=want)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(what="hint %d, outputs %s" % (case.hint, want))


def test_moves_layouts_bins_and_no_bins_kernels_at_one_lds_size(ctx, torch_dev):
    stream = _stream(torch_dev[0])
    binned = layouts_case(62, [(1, 1), (0, 1), (1, 0), (1, 1, "disjoint")] * 150, M_TWIN)
    plain = layouts_case(63, [(512, 400), (1, 1), (300, 512, "half"), (0, 0), (511, 512, "disjoint")] * 6, M_TWIN)
    assert binned.hint == HINT_BINS and plain.hint == HINT_PLAIN
    no_bins = tuple(k for k in LAYOUTS_OUTPUTS if k not in ("gained", "lost"))
    for case, want in ((binned, LAYOUTS_OUTPUTS), (plain, no_bins), (binned, LAYOUTS_OUTPUTS)):
        r = LayoutsRun(ctx, case, stream, want=want)
        ctx.sync(stream)
        assert r.launches == 1
        r.check(what="hint %d, outputs %s" % (case.hint, want))
