"""The three device-memory forms on the GPU at the cases of scale_cases.py: past one grid of workgroup steps (the second trip of
every grid-stride loop), past one chunk word per scan thread, past one topic per levels workgroup, past one sort tile class, the
sticky sort with digit 10 in its pass mask and the sticky match past one grid.  test_scale_cases_cpu.py holds that every case
crosses the threshold it names.  The harness is that of the forms' own modules, imported from them: every array a guarded device
buffer at an element shift, outputs preset to SENTINEL, inputs back byte for byte, ctx.sync without an error, every output equal
to its yardstick bit for bit (the verify verdicts as test_verify_gpu.Run.check holds them: zero / non-zero, UNCHECKED and the four
summary words equal to the yardstick's, the planted class bits among those set -- lagassign.h leaves the further bits of a failed
topic open as diagnostics; where a fault can touch one class only, the TOTALS one, the word is the yardstick's).  After each call
past one grid a small call on the same context is exact: the scratch has grown and nothing of the large call may leak.

Left out on purpose:
  - sticky digit 11 (the fourth byte of a run start): it needs n_pos >= 2^24
  - phase 4 of verify past one grid on topics of MANY rounds (a long walk per (chunk, consumer) pair in every step): about
    P x C = 2.7e11, which the oracle cannot produce in a test's time.  Its pair steps do pass one grid here, through topics of 8
    partitions and 4 097 consumers -- one round, one chunk -- which are also what takes phase 3, the consumer domain, past it
  - the cooperative host entries with the LARGE flags: they enqueue these same kernels"""
import time

import numpy as np
import pytest

import pinned_large_cases as PL
import scale_cases as X
import sticky_large_cases as SL
import verify_cases as V
import verify_large_cases as VL
from gpu_helpers import shifts_for
from pinned_cases import OUTPUTS as PINNED_OUTPUTS
from test_pinned_large_gpu import INPUTS as PINNED_INPUTS
from test_pinned_large_gpu import MAX_LAUNCHES as PINNED_MAX_LAUNCHES
from test_pinned_large_gpu import Run as PinnedRun
from test_sticky_large_gpu import MAX_LAUNCHES as STICKY_MAX_LAUNCHES
from test_sticky_large_gpu import Run as StickyRun
from test_verify_large_gpu import CLEAN, LargeRun

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(torch_dev):
    torch, dev = torch_dev
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _report(what, t0, *keys):
    ref = sum(X.SECONDS.get(k, 0.0) for k in keys)
    print("%s: %.1f s, of which the CPU reference %.1f s (0.0: built by an earlier test)" % (what, time.perf_counter() - t0, ref))


# ---- pinned ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.PINNED))
def test_pinned(ctx, cus, name):
    t0 = time.perf_counter()
    X.SECONDS.pop(("pinned", name, cus), None)
    c, exp = X.pinned_case(name, cus)
    big = X.pinned_large(c.shapes())
    print("%s at %d CUs: steps %d, n_big %d, n_pos %d" % (name, cus, X.steps_of(big), len(big), sum(big)))
    small, small_exp = PL.case("one past")
    one = PinnedRun(ctx, small)
    ctx.sync(one.stream)
    one.check(small_exp, "one past")
    r = PinnedRun(ctx, c, shifts_for("mixed", PINNED_INPUTS + PINNED_OUTPUTS))
    ctx.sync(r.stream)
    r.check(exp, name)
    # the launches of `one past` (one tile class), and the sort's 12 digit passes once more for every further tile class of the
    # call (lagassign.h): they depend on the classes, not on the number or the size of the large topics
    n_classes = len({X.tile_class(p) for p in big})
    assert r.launches == one.launches + X.SORT_DIGITS * (n_classes - 1) <= PINNED_MAX_LAUNCHES
    if name in X.PINNED_PAST_ONE_GRID:
        two, two_exp = PL.case("two large")
        again = PinnedRun(ctx, two)
        ctx.sync(again.stream)
        again.check(two_exp, "two large, after %s" % name)
        assert again.launches == one.launches
    _report(name, t0, ("pinned", name, cus))


# ---- sticky ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", X.STICKY_RUNS)
def test_sticky(ctx, torch_dev, cus, name, kind):
    t0 = time.perf_counter()
    keys = (("sticky target", name, cus), ("sticky", name, cus, kind))
    for k in keys:
        X.SECONDS.pop(k, None)
    stream = _stream(torch_dev[0])
    w, res = X.sticky_case(name, cus)
    ps = [int(w.part_off[t + 1] - w.part_off[t]) for t in SL.big_topics(w)]
    print("%s at %d CUs: steps %d, n_big %d, n_pos %d" % (name, cus, X.steps_of(ps), len(ps), sum(ps)))
    prev = X.sticky_prev(name, cus, kind)
    exp = X.sticky_expected(name, cus, kind)
    r = StickyRun(ctx, w, res, prev, stream)
    ctx.sync(stream)
    got = r.check(exp, "%s, %s" % (name, kind))
    assert 1 < r.launches <= STICKY_MAX_LAUNCHES and got["summary"][3] == 0
    if kind == "shifted":
        assert got["summary"][1] > got["summary"][0] and (got["sticky"] != res[0]).any()      # the case saves something
    if name == "past one grid":
        w2, res2 = SL.case("two large")
        again = StickyRun(ctx, w2, res2, SL.prev_of("two large", kind), stream)
        ctx.sync(stream)
        again.check(SL.expected("two large", kind), "two large, after %s" % name)
    _report("%s, %s" % (name, kind), t0, *keys)


# ---- verify ----------------------------------------------------------------------------------------------------------------------
def _verify_second_call(ctx, stream, what):
    w = VL.two_large_batch()
    res = V.oracle_result(w)
    clean, bad = LargeRun(ctx, w, res, stream), LargeRun(ctx, w, V.mutate("total + 1", w, res, 3), stream)
    ctx.sync(stream)
    got_v, got_s = clean.check("two large, after %s" % what)
    assert not got_v.any() and list(got_s) == CLEAN
    got_v, got_s = bad.check("two large with a fault, after %s" % what)
    assert list(np.flatnonzero(got_v)) == [3] and got_v[3] & V.TOTALS and list(got_s) == [1, 0, 3, -1]


def test_verify_clean(ctx, torch_dev, cus):
    t0 = time.perf_counter()
    keys = (("verify target", cus), ("verify", cus))
    for k in keys:
        X.SECONDS.pop(k, None)
    stream = _stream(torch_dev[0])
    w, res, exp = X.verify_case(cus)
    shapes = X.verify_shapes(cus)
    print("past one grid at %d CUs: partition, consumer, pair steps %s, n_big %d, n_pos %d" % (
        cus, X.first_steps(shapes)[1], len(shapes), w.n_partitions))
    assert not exp[0].any() and list(exp[1]) == CLEAN
    r = LargeRun(ctx, w, res, stream)
    ctx.sync(stream)
    got_v, got_s = r.check("past one grid", exp=exp)
    assert not got_v.any(), "topics %s: %s" % (np.flatnonzero(got_v), got_v[got_v != 0])
    assert list(got_s) == CLEAN
    _verify_second_call(ctx, stream, "the clean call")
    _report("verify, clean", t0, *keys)


def test_verify_planted(ctx, torch_dev, cus):
    t0 = time.perf_counter()
    X.SECONDS.pop(("verify planted", cus), None)
    stream = _stream(torch_dev[0])
    w, _, _ = X.verify_case(cus)
    res, exp = X.verify_planted(cus)
    faults = X.verify_faults(cus)
    assert list(np.flatnonzero(exp[0])) == sorted(faults) and list(exp[1]) == [len(faults), 0, min(faults), -1]
    r = LargeRun(ctx, w, res, stream)
    ctx.sync(stream)
    got_v, got_s = r.check("past one grid, planted", exp=exp)
    assert list(np.flatnonzero(got_v)) == sorted(faults)
    for t, name in faults.items():
        cls = X.FAULT_CLASS[name]
        assert got_v[t] & cls == cls, "%s in topic %d: verdict %d lacks its class" % (name, t, got_v[t])
        if name == "total + 1":                                          # out_total_lag alone differs: no other class can see it
            assert got_v[t] == exp[0][t] == V.TOTALS
    np.testing.assert_array_equal(got_s, exp[1])
    _verify_second_call(ctx, stream, "the planted call")
    _report("verify, planted", t0, ("verify planted", cus))
