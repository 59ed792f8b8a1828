"""Every greedy form at the exact limit where its bins stop packing (packing_cases.py: lag bits + round bits + index bits on
both sides of 62, the total field filled to its top bit), through the C ABI, bit for bit against the literal oracle.  The
conditions that make a mismatch here the kernel's fault are held by test_packing_cases_cpu.py on the same table."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kafka_lag_based_assignor_amd import _native as N
from kafka_lag_based_assignor_amd import synth
from oracle import oracle
from oracle.round_form import round_form
from gpu_helpers import *  # noqa: F401,F403
import packing_cases as pc

pytestmark = pytest.mark.gpu

# the per-round sort inside greedy_rounds_packed is picked by these (large path only)
LARGE_FLAGS = (N.LA_FLAG_NO_MOVED_SORT, N.LA_FLAG_SAMPLE_TIGHT, N.LA_FLAG_NO_SAMPLE_SORT, N.LA_FLAG_NO_RUN_MERGE)
# the host entry too: the first shape of every form
HOST_SHAPES = {}
for _s in pc.SHAPES:
    HOST_SHAPES.setdefault(_s[0], _s[1:3])


def topic_of(c):
    lag = pc.lags_of(c)
    if c.form in pc.LARGE_FORMS:
        return _topic_with_lags(lag, c.C, pc.seed_of(c))
    return _one_topic(c.P, c.C, lag, pc.seed_of(c))


def check_case(ctx, c):
    """One case: the literal oracle once (the round form beside it), then every entry and hook against it."""
    w = topic_of(c)
    what = pc.case_id(c)
    exp = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    _same3(round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), exp, "round form vs literal " + what)
    _same3(_device_call(ctx, w), exp, "device entry " + what)
    if HOST_SHAPES[c.form] == (c.P, c.C):
        _same3(ctx.assign_batch_lags(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), exp, "host entry " + what)
    if c.form in pc.LARGE_FORMS:
        for fl in LARGE_FLAGS:
            _same3(_device_call(ctx, w, flags=fl), exp, "flag %d %s" % (fl, what))


@pytest.mark.parametrize("c", [c for c in pc.CASES if not c.env], ids=pc.case_id)
def test_bins_pack_up_to_62_bits_and_not_beyond(ctx, c):
    check_case(ctx, c)


def side_by_side_batch():
    """One ragged batch: for every form its first shape with "brim" lags at S = 62 and again at S = 63, tile-sized topics and
    topics without partitions or without consumers between them."""
    shapes, brims = [], {}
    for i, (form, (P, C)) in enumerate(HOST_SHAPES.items()):
        for S in (62, 63):
            c = next(c for c in pc.CASES if (c.form, c.P, c.C, c.S, c.kind) == (form, P, C, S, "brim"))
            brims[len(shapes)] = c
            shapes.append((P, C))
            shapes.append([(100, 5), (0, 3), (1024, 64), (0, 0), (17, 0)][(2 * i + S) % 5])
    w = _batch_of(shapes, 62, kinds=["u20"])
    lag = w.lag.copy()
    for t, c in brims.items():
        lag[w.part_off[t]:w.part_off[t + 1]] = pc.lags_of(c)
    return synth.Workload("packing limit batch", w.n_topics, w.part_off, w.partition_id, w.begin, lag.copy(), w.committed, lag,
                          w.cons_off, w.cons_rank, w.max_partitions, w.max_consumers)


def check_side_by_side(ctx):
    w = side_by_side_batch()
    exp = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
    _same3(ctx.assign_batch_lags(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank), exp, "host entry")
    _same3(_device_call(ctx, w), exp, "device entry")


def test_packing_limit_side_by_side(ctx):
    """Neighbours in one launch decide independently (a workgroup per topic in the block path, a RoundsIo per item in the
    large path's launches over items): topics that just pack next to topics that just do not."""
    check_side_by_side(ctx)


@pytest.mark.parametrize("mode", ["0", "2"])
def test_forms_behind_block_key32_modes_in_a_fresh_process(mode):
    """LA_BLOCK_KEY32 is read once per process: =0 puts 65 .. 256 consumers on the 64-bit bins (one per lane on two wavefronts,
    or two / four per lane on one where the workgroup is one wavefront), =2 puts 129 .. 256 consumers on the 32-bit keys.  The
    table's cases of that mode one after another (the first failure ends the child), then the side-by-side batch."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from kafka_lag_based_assignor_amd import _native as N
import packing_cases as pc
import test_packing_limit_gpu as t
ctx = N.Context(0)
n = 0
for c in pc.CASES:
    if c.env == %r:
        t.check_case(ctx, c)
        n += 1
t.check_side_by_side(ctx)
print("ok", n)
"""
    n = sum(1 for c in pc.CASES if c.env == mode)
    assert n > 0
    env = dict(os.environ, LA_BLOCK_KEY32=mode)
    out = subprocess.run([sys.executable, "-c", code % (ROOT, os.path.join(ROOT, "tests"), mode)], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "ok %d" % n in out.stdout, (mode, out.stdout[-1500:], out.stderr[-3000:])
