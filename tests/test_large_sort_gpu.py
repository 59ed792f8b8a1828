"""The large path's device-wide radix sort (csrc/la_radix.hip) at its tile, digit, id-descent, tie-run and bound edges: every
case of sort_cases.py through the C ABI -- alone, side by side with a second large topic of another tile count (the launches
over items) and with the four-kernel passes -- exactly against the comparator's order and the round-form oracle, and the
decisions the sort reports (la_last_phase_times, la_last_launches) against the model written from the source.  That the cases
reach the edges they are named after is held by test_sort_cases_cpu.py on the same table."""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from oracle.round_form import round_form
from gpu_helpers import ROOT, _same3
import sort_cases as sc

pytestmark = pytest.mark.gpu

FORMS = ("alone", "side by side", "four-kernel passes")


@contextlib.contextmanager
def sort_context(sweep=None, keys_first=False, ctx=None):
    """LA_SWEEP_THREADS / LA_SORT_KEYS_FIRST (read per call) set around a fresh context -- or around `ctx` -- and put back."""
    want = {"LA_SWEEP_THREADS": None if sweep is None else str(sweep), "LA_SORT_KEYS_FIRST": "2" if keys_first else None}
    saved = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if ctx is not None:
            yield ctx
        else:
            with N.Context(0) as c:
                yield c
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def device_call(ctx, w, flags=0, bounds=None):
    """la_assign_batch_device on lags -> ((partition order, member ranks, totals), launches of the call)."""
    import torch
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(w, k))).to(dev) for k in ("part_off", "partition_id", "lag", "cons_off", "cons_rank")}
    out_pid = torch.full((max(w.n_partitions, 1),), -7, device=dev, dtype=torch.int32)
    out_rank = torch.full((max(w.n_partitions, 1),), -7, device=dev, dtype=torch.int32)
    out_total = torch.full((max(w.cons_rank.size, 1),), -7, device=dev, dtype=torch.int64)
    b = N.DeviceBatch()
    b.n_topics, b.reset_mode, b.algo, b.flags = w.n_topics, N.LA_RESET_LATEST, N.LA_ALGO_AUTO, flags
    b.n_partitions, b.n_consumers = w.n_partitions, w.cons_rank.size
    b.max_partitions_per_topic, b.max_consumers_per_topic = w.max_partitions, w.max_consumers
    b.d_part_off, b.d_partition_id, b.d_lag = d["part_off"].data_ptr(), d["partition_id"].data_ptr(), d["lag"].data_ptr()
    b.d_cons_off, b.d_cons_rank = d["cons_off"].data_ptr(), d["cons_rank"].data_ptr()
    b.d_out_partition, b.d_out_member_rank, b.d_out_total_lag = out_pid.data_ptr(), out_rank.data_ptr(), out_total.data_ptr()
    po, co = np.ascontiguousarray(w.part_off, np.int64), np.ascontiguousarray(w.cons_off, np.int64)
    b.h_part_off = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    b.h_cons_off = co.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    if bounds is not None:
        b.flags |= N.LA_FLAG_BOUNDS
        b.max_lag_hint, b.max_partition_id_hint = int(bounds[0]), int(bounds[1])
    stream = torch.cuda.current_stream().cuda_stream
    ctx.assign_batch_device(b, stream)
    ctx.sync(stream)
    got = (out_pid.cpu().numpy()[: w.n_partitions], out_rank.cpu().numpy()[: w.n_partitions], out_total.cpu().numpy()[: w.cons_rank.size])
    return got, ctx.last_launches()


def _forms(c, ids, lags, bounds):
    """(form, workload, expectation, flags, the model's plan, is the case the profiled topic) of the three call forms; the oracle
    runs once, over the pair."""
    pair = sc.workload([(ids, lags, c.C), sc.companion_of(c, bounds)])
    exp2 = round_form(pair.part_off, pair.partition_id, pair.lag, pair.cons_off, pair.cons_rank)
    alone = sc.workload([(ids, lags, c.C)])
    exp = (exp2[0][: c.n], exp2[1][: c.n], exp2[2][: c.C])
    np.testing.assert_array_equal(exp[0], sc.expected_order(ids, lags), err_msg="the oracle's order is the comparator's")
    if c.C == 0:
        assert (exp[1] == -1).all()
    single = sc.plan(ids, lags, c.sweep, c.keys_first, bounds)
    multi = sc.plan(ids, lags, c.sweep, c.keys_first, bounds, multi_kernel=True)
    # the profile is of the first topic of the narrowest tile class of a launch over items: the case's, unless its companion is narrower
    first = sc.sweep_threads(c.n, c.sweep) <= sc.sweep_threads(sc.companion_shape(c)[0], c.sweep)
    return ((FORMS[0], alone, exp, 0, single, True), (FORMS[1], pair, exp2, 0, single, first),
            (FORMS[2], alone, exp, N.LA_FLAG_SORT_MULTIKERNEL, multi, True))


def _check_profile(cx, c, p, what):
    t = cx.last_phase_times()
    assert t.n_partitions == c.n, (what, t.n_partitions)
    got = (t.id_passes, t.key_passes, t.keys_first, t.redone)
    assert got == (p.id_passes, p.key_passes, int(p.keys_first), p.redone), "%s %s: (id passes, key passes, keys first, redone) = %r, the model says %r" % (
        c.name, what, got, (p.id_passes, p.key_passes, int(p.keys_first), p.redone))


def check_case(c, ctx=None):
    """One case of the table in the three call forms; `ctx`: an existing context instead of a fresh one."""
    ids, lags = sc.data_of(c)
    bounds = sc.bounds_of(c, ids, lags)
    with sort_context(c.sweep, c.keys_first, ctx) as cx:
        for what, w, exp, flags, p, profiled in _forms(c, ids, lags, bounds):
            flags |= N.LA_FLAG_PROFILE
            tag = "%s, %s" % (c.name, what)
            if c.broken:
                # one partition one above a bound of 2^(8 d) - 1: an error of the call, and the context is as good as before
                with pytest.raises(N.LagAssignError) as e:
                    device_call(cx, w, flags, bounds)
                assert e.value.code == N.LA_EINVAL, tag
                _same3(device_call(cx, w, flags)[0], exp, tag + ", unbounded after the error")
                own = (max(int(w.lag.max()), bounds[0]), max(int(w.partition_id.max()), bounds[1]))
                _same3(device_call(cx, w, flags, own)[0], exp, tag + ", its own bounds after the error")
                continue
            if c.bounds is None:
                got, _ = device_call(cx, w, flags)
                _same3(got, exp, tag)
                if profiled:
                    _check_profile(cx, c, p, what)
                continue
            # Tight bounds.  sort_run_passes walks the 12 digits and skips, before any launch, those outside the mask; a digit inside
            # it is ONE launch (the single-kernel pass) or FOUR (count, two scans, scatter).  A launch over items calls it once per
            # tile class.  These topics are far below 2^22 partitions and no hook is set, so no tie repair or redo launch exists,
            # and the data is inside the bounds, so nothing else differs: unbounded minus bounded = dropped digits x launches per pass
            # x tile classes.
            plain, n_plain = device_call(cx, w, flags)
            _same3(plain, exp, tag + ", unbounded")
            tight, n_tight = device_call(cx, w, flags, bounds)
            _same3(tight, exp, tag + ", tight bounds")
            if profiled:
                _check_profile(cx, c, p, what)
            dropped = sc.DIGITS - bin(p.mask).count("1")
            per_pass = 4 if flags & N.LA_FLAG_SORT_MULTIKERNEL else 1
            classes = len({sc.sweep_threads(int(n), c.sweep) for n in np.diff(w.part_off)})
            assert n_plain - n_tight == dropped * per_pass * classes, "%s: %d launches unbounded, %d bounded; the mask %s drops %d passes" % (
                tag, n_plain, n_tight, bin(p.mask), dropped)


@pytest.mark.parametrize("c", [pytest.param(c, id=sc.case_id(c)) for c in sc.CASES])
def test_sort_case(ctx, c):
    """Groups a to e of the table.  A case that sets a hook runs on a fresh context with the hook set around it."""
    check_case(c, ctx if c.sweep is None and not c.keys_first else None)


@pytest.mark.parametrize("m", [pytest.param(m, id="members%d" % m) for m in sc.GROUP_MEMBERS])
def test_group_by_member_radix_form_at_its_pass_borders(ctx, m):
    """65 537 entries (one past the mid form) grouped by 255 .. 65 537 members: key = rank + 1 takes one pass per byte of
    n_members, and the highest rank is the key that needs the last of them."""
    part_off, out_p, out_m = sc.group_case(m)
    off, g_t, g_p = ctx.group_by_member(part_off, out_p, out_m, m)
    e_off, e_t, e_p = sc.expected_groups(part_off, out_p, out_m, m)
    np.testing.assert_array_equal(off, e_off, err_msg="member_off")
    np.testing.assert_array_equal(g_t, e_t, err_msg="grouped_topic")
    np.testing.assert_array_equal(g_p, e_p, err_msg="grouped_partition")


@pytest.mark.parametrize("p,c,w", [pytest.param(p, c, w, id="%dx%d-w%d" % (p, c, w)) for p, c, w in sc.HUGE_CASES])
def test_bins_in_hbm_under_every_width(p, c, w):
    """More than 8 192 consumers: every round sorts the C totals with the same passes, laid out for C elements."""
    ids, lags, _ = sc.huge_topic(p, c)
    wl = sc.workload([(ids, lags, c)])
    exp = round_form(wl.part_off, wl.partition_id, wl.lag, wl.cons_off, wl.cons_rank)
    with sort_context(w) as cx:
        _same3(device_call(cx, wl)[0], exp, "%d x %d, %d threads" % (p, c, w))
        _same3(device_call(cx, wl, N.LA_FLAG_SORT_MULTIKERNEL)[0], exp, "%d x %d, four-kernel passes of the partitions" % (p, c))


def test_match_ranks_and_a_three_block_keys_grid_in_a_fresh_process():
    """LA_SORT_RANK and LA_KEYS_GRID are read once per process: groups a to d again with ranks from wave-match ballots (both pass
    forms) and the keys kernel on three workgroups, each striding over the whole topic."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from kafka_lag_based_assignor_amd import _native as N
import sort_cases as sc
import test_large_sort_gpu as t
ctx = N.Context(0)
assert not (ctx.device_features(0) & N.LA_FEATURE_ATOMIC_RANK)
n = 0
for c in sc.CASES:
    if c.group in "abcd":
        t.check_case(c, ctx)
        n += 1
print("ok", n)
"""
    n = sum(1 for c in sc.CASES if c.group in "abcd")
    env = dict(os.environ, LA_SORT_RANK="match", LA_KEYS_GRID="3")
    out = subprocess.run([sys.executable, "-c", code % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "ok %d" % n in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
