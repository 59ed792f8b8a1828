"""Group-wide moves on CPU: world_size-2 gloo.  Each rank joins the oracle's two assignments of its own contiguous shard of topics
(sharding.assignment_moves_numpy); shards are disjoint topic ranges, so sharding.reduce_member_loads(gained, lost, moved) -- ONE
all_reduce of 2 * M + 1 int64 -- must give every rank the gained / lost counts and the moved total of the whole batch: what a
multi-GPU step does with nccl (= RCCL) on the outputs of la_assignment_moves_device_on."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kafka_lag_based_assignor_amd import sharding, synth  # noqa: E402

N_MEMBERS = 30


def _two(part_off, pid, lag, lag2, cons_off, cons_rank):
    from oracle import oracle
    prev = oracle.assign_flat(part_off, pid, lag, cons_off, cons_rank)
    cur = oracle.assign_flat(part_off, pid, lag2, cons_off, cons_rank)
    return sharding.assignment_moves_numpy(part_off, cur[0], cur[1], prev[0], prev[1], N_MEMBERS)


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    w = synth.ragged(44, 97, 60, 9)
    lag2 = np.random.default_rng(1).integers(0, 1 << 40, w.n_partitions).astype(np.int64)
    t0, t1 = sharding.shard_bounds(w.part_off, world)[rank]
    po, co, ps, cs = sharding.shard_slices(w.part_off, w.cons_off, t0, t1)
    part = _two(po, w.partition_id[ps], w.lag[ps], lag2[ps], co, w.cons_rank[cs])
    got = sharding.reduce_member_loads(part[2], part[3], part[4])
    exp = _two(w.part_off, w.partition_id, w.lag, lag2, w.cons_off, w.cons_rank)
    ok = np.array_equal(got[0], exp[2]) and np.array_equal(got[1], exp[3]) and got[2] == exp[4]
    ok = ok and got[0].dtype == np.int64 and got[1].dtype == np.int64
    ok = ok and exp[4] > 0 and int(exp[1].sum()) == exp[4]
    ok = ok and np.array_equal(part[1], exp[1][t0:t1])                              # the per-topic counts are the shard's slice
    ok = ok and not np.array_equal(part[2], exp[2])                                 # ... and one shard alone is not the answer
    ret[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gloo_reduce_equals_whole_batch():
    world = 2
    port = 33500 + (os.getpid() % 2000)
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, world, port, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(240)
            assert p.exitcode == 0
        assert dict(ret) == {0: True, 1: True}
