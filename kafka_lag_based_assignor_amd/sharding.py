"""Multi-GPU layout: one process per GPU, topics sharded across ranks.

``assignTopic`` reads and writes only its own topic's bins (Main.java:216-225), so topics are
independent units: each rank runs the whole hot path on a contiguous range of topics and
there is NO collective on the data path.  Reassembling the global (partition -> member) map
on every rank -- the north star's "single RCCL all-gather over xGMI" -- is an optional output
step (``gather_results``): with ``torch.distributed`` backend "nccl" it is RCCL, with "gloo"
it runs on CPU (tests).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def shard_bounds(part_off: np.ndarray, world_size: int) -> List[Tuple[int, int]]:
    """Contiguous topic ranges [t0, t1) per rank, balanced by partition count (the kernels'
    cost is per partition).  Every topic lands in exactly one range; ranges may be empty.

    This IS the library's planner (``la_plan_shards`` of include/lagassign.h, pure host code): the split a
    one-process-per-GPU launcher makes here is the split a multi-device context (``la_create_multi``) makes
    inside ``la_assign_batch``."""
    try:
        from . import _native
        b = _native.plan_shards(part_off, world_size)
    except (OSError, ImportError):
        # liblagassign.so (and with it the HIP runtime) cannot be loaded on this host -- a launcher node, a gloo-only
        # test: the planner is pure host arithmetic, so the same formula is restated here.  tests/test_sharding_gloo.py
        # asserts that the two agree.
        b = plan_shards_numpy(part_off, world_size)
    return [(int(b[r]), int(b[r + 1])) for r in range(world_size)]


def plan_shards_numpy(part_off: np.ndarray, n_shards: int) -> np.ndarray:
    """la_plan_shards restated: bounds[r] = first topic boundary at or after r/n_shards of the partitions
    (target = base + (total // S) * r + (total % S) * r // S), searched from the previous bound on."""
    po = np.ascontiguousarray(part_off, dtype=np.int64)
    t = po.size - 1
    if t < 0 or n_shards < 1 or np.any(np.diff(po) < 0):
        raise ValueError("bad offsets or shard count")
    base, total = int(po[0]), int(po[t] - po[0])
    bounds = np.zeros(n_shards + 1, dtype=np.int32)
    for r in range(1, n_shards):
        target = base + (total // n_shards) * r + (total % n_shards) * r // n_shards
        lo = int(bounds[r - 1])
        bounds[r] = min(t, lo + int(np.searchsorted(po[lo:], target, side="left")))
    bounds[n_shards] = t
    return bounds


def shard_slices(part_off: np.ndarray, cons_off: np.ndarray, t0: int, t1: int):
    """(local part_off, local cons_off, partition slice, consumer slice) of topics [t0, t1)."""
    po = np.asarray(part_off[t0:t1 + 1], dtype=np.int64)
    co = np.asarray(cons_off[t0:t1 + 1], dtype=np.int64)
    return po - po[0], co - co[0], slice(int(po[0]), int(po[-1])), slice(int(co[0]), int(co[-1]))


def strong_plan(part_off: np.ndarray, world_size: int):
    """The split of ONE batch over `world_size` ranks (strong scaling): (bounds, counts, cap) with
    bounds[r]..bounds[r+1] the topics of rank r (la_plan_shards), counts[r] its partitions and cap the largest
    count -- ncclAllGather moves equal counts, so every rank's result buffers are `cap` long and the tail is padding."""
    bounds = shard_bounds(part_off, world_size)
    counts = [int(part_off[t1] - part_off[t0]) for t0, t1 in bounds]
    return bounds, counts, (max(counts) if counts else 0)


def strip_padding(gathered, counts: List[int], cap: int):
    """[world * cap] all-gathered array -> the global array (rank order = topic order: shards are contiguous)."""
    import torch
    if isinstance(gathered, np.ndarray):
        return np.concatenate([gathered[r * cap: r * cap + counts[r]] for r in range(len(counts))])
    return torch.cat([gathered[r * cap: r * cap + counts[r]] for r in range(len(counts))])


def wire_format_numpy(max_partition_id: int, n_members: int) -> Tuple[int, int]:
    """la_wire_format_for restated (elem_bytes, id_bits): the narrowest unsigned element that holds
    ((member rank + 1) << id_bits) | partition id for ids in [0, max_partition_id] and ranks in [-1, n_members);
    (8, 32) carries any int32 pair.  tests/test_sharding_gloo.py asserts that the library agrees."""
    if max_partition_id < 0 or max_partition_id > 0x7FFFFFFF or n_members < 0 or n_members > 0x7FFFFFFF:
        return 8, 32
    ib, rb = int(max_partition_id).bit_length(), int(n_members).bit_length()
    if ib + rb <= 16:
        return 2, ib
    if ib + rb <= 32:
        return 4, ib
    return 8, 32


_WIRE_DTYPE = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def pack_results_numpy(pid: np.ndarray, rank: np.ndarray, elem_bytes: int, id_bits: int) -> np.ndarray:
    """The wire format on the host (what la_pack_results_on does on the device): raises if a pair does not fit."""
    p = np.asarray(pid, dtype=np.int32).view(np.uint32).astype(np.uint64)
    r1 = (np.asarray(rank, dtype=np.int64) + 1)
    if (r1 < 0).any():
        raise ValueError("member ranks must be >= -1")
    r1 = r1.astype(np.uint64)
    if elem_bytes != 8:
        if (p >> np.uint64(id_bits)).any() or (r1 >> np.uint64(8 * elem_bytes - id_bits)).any():
            raise ValueError("a partition id or member rank does not fit the wire format")
    return ((r1 << np.uint64(id_bits)) | p).astype(_WIRE_DTYPE[elem_bytes])


def unpack_results_numpy(packed: np.ndarray, elem_bytes: int, id_bits: int):
    w = np.asarray(packed).astype(np.uint64)
    mask = np.uint64(0xFFFFFFFF if id_bits >= 32 else (1 << id_bits) - 1)
    pid = (w & mask).astype(np.uint32).view(np.int32)
    rank = ((w >> np.uint64(id_bits)).astype(np.int64) - 1).astype(np.int32)
    return pid, rank


def gather_results_packed(local_pid, local_rank, counts: List[int], max_partition_id: int, n_members: int, group=None):
    """gather_results through the narrow wire format: ONE all_gather_into_tensor of `cap` elements of 2 / 4 / 8 bytes per
    rank instead of two int32 arrays (8 B per partition).  Host tensors (gloo; the CPU test): packed with the numpy
    restatement; device tensors go through la_pack_results_on / la_unpack_results_on in bench.py."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    cap = max(counts) if counts else 0
    eb, ib = wire_format_numpy(max_partition_id, n_members)
    dt = {2: torch.int16, 4: torch.int32, 8: torch.int64}[eb]           # same width; gloo has no unsigned 16 / 32
    send = torch.zeros(cap, dtype=dt)
    packed = pack_results_numpy(local_pid.numpy(), local_rank.numpy(), eb, ib)
    send[: packed.size] = torch.from_numpy(packed.view({2: np.int16, 4: np.int32, 8: np.int64}[eb]))
    recv = torch.empty(world * cap, dtype=dt)
    dist.all_gather_into_tensor(recv, send, group=group)
    g = strip_padding(recv.numpy().view(_WIRE_DTYPE[eb]), counts, cap)
    pid, rank = unpack_results_numpy(g, eb, ib)
    return torch.from_numpy(pid), torch.from_numpy(rank), eb * cap


def gather_results(local_pid, local_rank, counts: List[int], group=None):
    """All-gathers the per-rank result arrays into the global arrays (topic order = rank
    order, because shards are contiguous).  ``counts[r]`` = partitions owned by rank r.
    Shards are padded to the largest so ONE all_gather_into_tensor per array suffices
    (ncclAllGather needs equal counts)."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    cap = max(counts) if counts else 0
    dev = local_pid.device

    def one(x):
        send = torch.zeros(cap, dtype=x.dtype, device=dev)
        send[: x.numel()] = x
        recv = torch.empty(world * cap, dtype=x.dtype, device=dev)
        dist.all_gather_into_tensor(recv, send, group=group)
        return strip_padding(recv, counts, cap)

    return one(local_pid), one(local_rank)


def member_loads_numpy(out_member_rank, cons_rank, out_total_lag, n_members: int):
    """la_member_loads_device restated on the host -> (partitions int64[M], lag int64[M], unassigned int):
    partitions[r] = entries of out_member_rank equal to r, unassigned = its entries equal to -1 (topics without consumers,
    Main.java:211-213), lag[r] = sum of out_total_lag[k] over cons_rank[k] == r in Java long arithmetic (wraps).  A rank
    outside [-1, M) / [0, M) raises ValueError.  The yardstick of the GPU tests, and what a gloo-only launcher uses."""
    m = int(n_members)
    rank = np.asarray(out_member_rank, dtype=np.int64).ravel()
    cr = np.asarray(cons_rank, dtype=np.int64).ravel()
    tot = np.ascontiguousarray(np.asarray(out_total_lag, dtype=np.int64).ravel())
    if m < 0 or cr.size != tot.size:
        raise ValueError("n_members < 0, or cons_rank and out_total_lag differ in length")
    if (rank.size and (rank.min() < -1 or rank.max() >= m)) or (cr.size and (cr.min() < 0 or cr.max() >= m)):
        raise ValueError("a member rank lies outside [-1, n_members) or a consumer rank outside [0, n_members)")
    counts = np.bincount(rank + 1, minlength=m + 1).astype(np.int64)
    lag = np.zeros(m, dtype=np.uint64)
    np.add.at(lag, cr, tot.view(np.uint64))          # unsigned adds wrap silently: the bits of Java's long sum
    return counts[1:].copy(), lag.view(np.int64), int(counts[0])


def assignment_moves_numpy(part_off, out_partition, out_member_rank, prev_partition, prev_member_rank, n_members: int,
                           prev_rank_map=None):
    """la_assignment_moves_device restated on the host -> (prev_owner int32[N], topic_moved int64[T], gained int64[M],
    lost int64[M], moved int).  Both assignments share the layout `part_off` and come in their own assignment order: each side is
    sorted by (topic, partition id) with np.lexsort, after which the two line up position by position.  prev_owner[i] is the
    previous owner of current entry i in today's ranks (prev_rank_map[p], or p itself without a map; -1 stays -1); an entry
    moved when that differs from out_member_rank[i]; a moved entry counts for its topic, for the member that gained it (>= 0)
    and the one that lost it (>= 0).  ValueError for what the device reports as LA_EINVAL: a duplicate id inside a topic, id
    sets that differ, a previous rank outside [-1, M_prev), a mapped or current rank outside [-1, M).  The yardstick of the GPU
    tests."""
    m = int(n_members)
    po = np.asarray(part_off, dtype=np.int64).ravel()
    cur_id = np.asarray(out_partition, dtype=np.int64).ravel()
    prev_id = np.asarray(prev_partition, dtype=np.int64).ravel()
    c = np.asarray(out_member_rank, dtype=np.int64).ravel()
    p = np.asarray(prev_member_rank, dtype=np.int64).ravel()
    if m < 0 or po.size < 1 or po[0] != 0 or (np.diff(po) < 0).any():
        raise ValueError("n_members < 0, or part_off does not ascend from 0")
    t, n = po.size - 1, int(po[-1])
    if not (cur_id.size == prev_id.size == c.size == p.size == n):
        raise ValueError("the four assignment arrays must hold part_off[T] entries each")
    if prev_rank_map is None:
        m_prev, q = m, p
    else:
        rank_map = np.asarray(prev_rank_map, dtype=np.int64).ravel()
        m_prev = rank_map.size
    if n and (p.min() < -1 or p.max() >= m_prev):
        raise ValueError("a previous member rank lies outside [-1, n_prev_members)")
    if prev_rank_map is not None:
        q = np.where(p < 0, -1, rank_map[np.maximum(p, 0)]) if m_prev else p
    if n and (q.min() < -1 or q.max() >= m or c.min() < -1 or c.max() >= m):
        raise ValueError("a mapped previous rank or a current member rank lies outside [-1, n_members)")
    topic = np.repeat(np.arange(t, dtype=np.int64), np.diff(po))
    by_cur, by_prev = np.lexsort((cur_id, topic)), np.lexsort((prev_id, topic))
    a, b = cur_id[by_cur], prev_id[by_prev]                 # (topic is ascending already: both sorted sides share it)
    for ids in (a, b):
        if n > 1 and ((ids[1:] == ids[:-1]) & (topic[1:] == topic[:-1])).any():
            raise ValueError("a partition id appears twice inside a topic")
    if (a != b).any():
        raise ValueError("a topic's current and previous partition ids differ")
    owner = np.empty(n, dtype=np.int64)
    owner[by_cur] = q[by_prev]
    moved = owner != c
    topic_moved = np.bincount(topic[moved], minlength=t).astype(np.int64)[:t]
    gained = np.bincount(c[moved & (c >= 0)], minlength=m).astype(np.int64)[:m]
    lost = np.bincount(owner[moved & (owner >= 0)], minlength=m).astype(np.int64)[:m]
    return owner.astype(np.int32), topic_moved, gained, lost, int(moved.sum())


MOVES_NO_PREVIOUS = -2          # LA_MOVES_NO_PREVIOUS: prev_owner of a partition that was added


def prev_topic_map(prev_names, names):
    """d_prev_topic of la_assignment_moves_device from the topic names of the two layouts -> int32[len(names)]: the index of each
    of today's names among the previous names, -1 for a name that is new.  ValueError when a list names a topic twice."""
    prev_names, names = list(prev_names), list(names)
    index = {name: i for i, name in enumerate(prev_names)}
    if len(index) != len(prev_names) or len(set(names)) != len(names):
        raise ValueError("a topic is named twice")
    return np.array([index.get(name, -1) for name in names], dtype=np.int32).reshape(len(names))


def assignment_moves_layouts_numpy(part_off, out_partition, out_member_rank, prev_part_off, prev_partition, prev_member_rank,
                                   n_members: int, prev_rank_map=None, prev_topic=None):
    """la_assignment_moves_device with two layouts (d_prev_part_off) restated on the host -> (prev_owner int32[N],
    topic_moved, topic_added, topic_removed int64[T], gained, lost int64[M], moved, added, removed int).  Today's topic t is
    topic prev_topic[t] of the previous layout (-1: new; no map: t itself, both layouts then hold the same number of topics).
    Entries are keyed by (today's topic, id) and both sides sorted; np.searchsorted finds each current key among the previous
    ones.  A current entry with a previous one: prev_owner is that owner in today's ranks, moved iff it differs from the
    current owner, counted as in assignment_moves_numpy.  Without one it is ADDED: prev_owner = MOVES_NO_PREVIOUS, it counts
    for topic_added, added and gained[c] (c >= 0), not as moved.  A previous entry of a named topic that no current entry
    matched is REMOVED: topic_removed, removed, lost[q] (q >= 0).  Previous topics that no entry of prev_topic names are not
    looked at.  ValueError for what the device reports as LA_EINVAL: a duplicate id inside a segment, a rank out of range
    (assignment_moves_numpy's rules, over the segments that are looked at), a map entry outside [-1, T_prev) -- and for a
    previous topic named twice, which the device leaves to the caller.  The yardstick of the GPU tests."""
    m = int(n_members)
    po = np.asarray(part_off, dtype=np.int64).ravel()
    ppo = np.asarray(prev_part_off, dtype=np.int64).ravel()
    cur_id = np.asarray(out_partition, dtype=np.int64).ravel()
    prev_id = np.asarray(prev_partition, dtype=np.int64).ravel()
    c = np.asarray(out_member_rank, dtype=np.int64).ravel()
    p = np.asarray(prev_member_rank, dtype=np.int64).ravel()
    for off in (po, ppo):
        if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any():
            raise ValueError("an offset array does not ascend from 0")
    if m < 0:
        raise ValueError("n_members < 0")
    t, n, t_prev, n_prev = po.size - 1, int(po[-1]), ppo.size - 1, int(ppo[-1])
    if not (cur_id.size == c.size == n and prev_id.size == p.size == n_prev):
        raise ValueError("the assignment arrays must hold part_off[T] / prev_part_off[T_prev] entries")
    if prev_topic is None:
        if t_prev != t:
            raise ValueError("without prev_topic both layouts hold the same number of topics")
        s = np.arange(t, dtype=np.int64)
    else:
        s = np.asarray(prev_topic, dtype=np.int64).ravel()
        if s.size != t or (t and (s.min() < -1 or s.max() >= t_prev)):
            raise ValueError("prev_topic must hold T entries inside [-1, T_prev)")
    named = s[s >= 0]
    if np.unique(named).size != named.size:
        raise ValueError("a previous topic is named twice")
    # the previous entries that are looked at, under today's topic numbers
    today_of = np.full(t_prev, -1, dtype=np.int64)
    today_of[named] = np.flatnonzero(s >= 0)
    prev_topic_of_entry = today_of[np.repeat(np.arange(t_prev, dtype=np.int64), np.diff(ppo))]
    seen = prev_topic_of_entry >= 0
    b_topic, b_id, p = prev_topic_of_entry[seen], prev_id[seen], p[seen]
    if prev_rank_map is None:
        m_prev, q = m, p
    else:
        rank_map = np.asarray(prev_rank_map, dtype=np.int64).ravel()
        m_prev = rank_map.size
    if p.size and (p.min() < -1 or p.max() >= m_prev):
        raise ValueError("a previous member rank lies outside [-1, n_prev_members)")
    if prev_rank_map is not None:
        q = np.where(p < 0, -1, rank_map[np.maximum(p, 0)]) if m_prev else p
    if (q.size and (q.min() < -1 or q.max() >= m)) or (n and (c.min() < -1 or c.max() >= m)):
        raise ValueError("a mapped previous rank or a current member rank lies outside [-1, n_members)")
    a_topic = np.repeat(np.arange(t, dtype=np.int64), np.diff(po))
    a_key = (a_topic << 32) | (cur_id & 0xFFFFFFFF)
    b_key = (b_topic << 32) | (b_id & 0xFFFFFFFF)
    by_prev = np.argsort(b_key, kind="stable")
    b_sorted = b_key[by_prev]
    for keys in (np.sort(a_key), b_sorted):
        if (keys[1:] == keys[:-1]).any():
            raise ValueError("a partition id appears twice inside a topic")
    at = np.minimum(np.searchsorted(b_sorted, a_key), max(b_sorted.size - 1, 0))
    hit = (b_sorted[at] == a_key) if b_sorted.size else np.zeros(n, dtype=bool)
    owner = np.full(n, MOVES_NO_PREVIOUS, dtype=np.int64)
    owner[hit] = q[by_prev[at[hit]]]
    matched = np.zeros(b_sorted.size, dtype=bool)
    matched[by_prev[at[hit]]] = True
    moved = hit & (owner != c)
    added = ~hit
    count = lambda idx, size: np.bincount(idx, minlength=size).astype(np.int64)[:size]
    gained = count(c[(moved | added) & (c >= 0)], m)
    lost = count(owner[moved & (owner >= 0)], m) + count(q[~matched & (q >= 0)], m)
    return (owner.astype(np.int32), count(a_topic[moved], t), count(a_topic[added], t), count(b_topic[~matched], t), gained, lost,
            int(moved.sum()), int(added.sum()), int((~matched).sum()))


VERDICT_IDS, VERDICT_ORDER, VERDICT_OWNER, VERDICT_GREEDY, VERDICT_TOTALS, VERDICT_UNCHECKED = 1, 2, 4, 8, 16, 32


def verify_assignment_numpy(part_off, partition_id, cons_off, cons_rank, out_partition, out_member_rank, out_total_lag=None, *,
                            lag=None, begin=None, end=None, committed=None, reset_latest: bool = True,
                            max_partitions: int = 4096, max_consumers: int = 4096):
    """la_verify_assignment_device restated on the host -> (verdict int32[T], summary int64[4]).  Written from the statement of
    the reference's result (Main.java:204-266), not by computing that result: per topic with distinct ids and strictly ascending
    ranks,
      V1  the output ids are the topic's input ids, none twice; lag_i is the lag of the input partition with that id
          (`lag`, or Java's computePartitionLag of begin / end / committed; no begin array: 0)
      V2  neighbours: lag_i > lag_(i+1) signed, or equal lags and id_i < id_(i+1)
      V3  no consumers: every owner is -1.  Otherwise every owner subscribes, the owners of a round of C positions are
          distinct, their keys (the owner's wrapping total over the earlier rounds, rank) ascend strictly along the round,
          and every consumer a partial last round left out has a key above the last picked one
      V4  out_total_lag (when given) holds every consumer's final wrapping total
    verdict[t] is 0 or a mask of VERDICT_*; VERDICT_UNCHECKED stands alone: more than max_partitions / max_consumers, duplicate
    input ids, ranks that do not ascend.  Once a class fails the later ones are not looked at (their bits are diagnostics).
    summary = topics failed, topics unchecked, the lowest index of each or -1.  Offsets that leave the arrays raise ValueError.
    The yardstick of the GPU tests; tests/test_verify_cpu.py holds it against the oracle."""
    po = np.asarray(part_off, dtype=np.int64).ravel()
    co = np.asarray(cons_off, dtype=np.int64).ravel()
    pid = np.asarray(partition_id, dtype=np.int32).ravel()
    ranks = np.asarray(cons_rank, dtype=np.int32).ravel()
    o_pid = np.asarray(out_partition, dtype=np.int32).ravel()
    o_own = np.asarray(out_member_rank, dtype=np.int32).ravel()
    o_tot = None if out_total_lag is None else np.asarray(out_total_lag, dtype=np.int64).ravel()
    n, k_all, t_all = pid.size, ranks.size, po.size - 1
    if lag is not None:
        lag = np.ascontiguousarray(np.asarray(lag, dtype=np.int64).ravel())
    else:
        e = np.ascontiguousarray(np.asarray(end, dtype=np.int64).ravel())
        c = np.asarray(committed, dtype=np.int64).ravel()
        fallback = e if reset_latest else (np.zeros_like(e) if begin is None else np.asarray(begin, dtype=np.int64).ravel())
        nxt = np.ascontiguousarray(np.where(c >= 0, c, fallback))
        d = (e.view(np.uint64) - nxt.view(np.uint64)).view(np.int64)         # Java's wrapping subtract
        lag = np.ascontiguousarray(np.where(d > 0, d, np.int64(0)))
    if t_all < 0 or co.size != po.size or not (lag.size == o_pid.size == o_own.size == n) or (o_tot is not None and o_tot.size != k_all):
        raise ValueError("array sizes do not fit one layout")
    verdict = np.zeros(t_all, dtype=np.int32)
    u64 = np.uint64
    for t in range(t_all):
        a, z, ca, cz = int(po[t]), int(po[t + 1]), int(co[t]), int(co[t + 1])
        if not (0 <= a <= z <= n and 0 <= ca <= cz <= k_all):
            raise ValueError("the offsets of topic %d leave the arrays" % t)
        p, c = z - a, cz - ca
        ids, r = pid[a:z], ranks[ca:cz]
        if p > max_partitions or c > max_consumers or np.unique(ids).size != p or (np.diff(r.astype(np.int64)) <= 0).any():
            verdict[t] = VERDICT_UNCHECKED
            continue
        oid, own = o_pid[a:z], o_own[a:z]
        # V1: the join
        by_id = np.argsort(ids, kind="stable")
        sorted_ids = ids[by_id]
        at = np.minimum(np.searchsorted(sorted_ids, oid), max(p - 1, 0))
        if p and ((sorted_ids[at] != oid).any() or np.unique(oid).size != p):
            verdict[t] = VERDICT_IDS
            continue
        l = np.ascontiguousarray(lag[a:z][by_id[at]]) if p else np.empty(0, np.int64)
        v = 0
        # V2
        if p > 1 and not ((l[:-1] > l[1:]) | ((l[:-1] == l[1:]) & (oid[:-1] < oid[1:]))).all():
            v |= VERDICT_ORDER
        # V3, V4
        if c == 0:
            if (own != -1).any():
                v |= VERDICT_OWNER
            verdict[t] = v
            continue
        k = np.minimum(np.searchsorted(r, own), c - 1)
        rnd = np.arange(p, dtype=np.int64) // c
        if (r[k] != own).any() or np.unique(rnd * c + k).size != p:
            verdict[t] = v | VERDICT_OWNER
            continue
        lu = l.view(u64)
        tot = np.zeros(c, dtype=u64)
        np.add.at(tot, k, lu)                                               # unsigned adds wrap: the bits of Java's long sum
        if p:
            by_k = np.argsort(k, kind="stable")                             # a consumer's entries, in position order
            ls, ks = lu[by_k], k[by_k]
            excl = np.cumsum(ls, dtype=u64) - ls
            first = np.r_[True, ks[1:] != ks[:-1]]
            before = np.empty(p, dtype=u64)
            before[by_k] = excl - excl[first][np.cumsum(first) - 1]
            before = before.view(np.int64)                                  # compared signed, as Long.compare does
            rk = r[k]
            asc = (before[:-1] < before[1:]) | ((before[:-1] == before[1:]) & (rk[:-1] < rk[1:]))
            if ((rnd[:-1] == rnd[1:]) & ~asc).any():
                v |= VERDICT_GREEDY
            if p % c:
                lo = (p // c) * c
                left_out = np.ones(c, dtype=bool)
                left_out[k[lo:]] = False
                start = tot.copy()
                np.subtract.at(start, k[lo:], lu[lo:])                      # totals at the start of the last round
                start = start.view(np.int64)
                above = (start > before[p - 1]) | ((start == before[p - 1]) & (r > rk[p - 1]))
                if (left_out & ~above).any():
                    v |= VERDICT_GREEDY
        if o_tot is not None and (tot.view(np.int64) != o_tot[ca:cz]).any():
            v |= VERDICT_TOTALS
        verdict[t] = v
    unchecked = (verdict & VERDICT_UNCHECKED) != 0
    failed = (verdict != 0) & ~unchecked
    first = lambda m: int(np.flatnonzero(m)[0]) if m.any() else -1
    return verdict, np.array([int(failed.sum()), int(unchecked.sum()), first(failed), first(unchecked)], dtype=np.int64)


STICKY_MAX_PARTITIONS = 4096      # topics beyond it are passed through by la_sticky_ties_device (kVerifyMaxPartitions of csrc/la_kernels.h)
# max_partitions of the functions below for a call with LA_FLAG_STICKY_LARGE / LA_COOP_STICKY_LARGE: no limit -- what the device
# re-matches then (kStickyGlobalMaxPartitions of csrc/la_kernels.h; nothing a host array holds reaches it)
STICKY_ANY_SIZE = (1 << 30) - 2


def sticky_ties_numpy(part_off, partition_id, lag, out_partition, out_member_rank, prev_owner, *,
                      max_partitions: int = STICKY_MAX_PARTITIONS, strict: bool = True):
    """la_sticky_ties_device restated on the host -> (sticky_partition int32[N], topic_kept int64[T], topic_saved int64[T],
    summary int64[4]).  Per topic, lag_i is the lag of the input partition whose id is out_partition[i] (a join on the id); a run
    is a maximal range of consecutive positions of equal lag_i; c_i = out_member_rank[i], q_i = prev_owner[i].  Inside one run:
      1  for every c >= 0, S_c = the run's positions with c_i == c, ascending
      2  for every c >= 0, W_c = the run's positions with q_i == c, ascending
      3  for k < min(|S_c|, |W_c|) the partition at W_c[k] goes to S_c[k]
      4  the partitions not placed by 3 go, in ascending position, to the positions not filled by 3, in ascending position
      5  sticky_partition[dest] = out_partition[src]
    A position is kept when the partition placed there has q >= 0 and q equals the position's c.  topic_kept counts them after,
    topic_saved = after - before, summary = kept before, kept after, topics whose order changed, topics passed through.  A topic
    of more than max_partitions partitions is passed through: copied, saved 0, kept the count before.  ValueError for what the
    device reports as LA_EINVAL -- a duplicate id in a topic's input segment, an output id that is no input id of the topic or
    appears twice -- unless strict is False: such a topic is then passed through as the device passes it.  Offsets that leave
    the arrays raise ValueError.  Plain loops, rule by rule: the yardstick of tests/test_sticky_gpu.py, not a fast path."""
    po = np.asarray(part_off, dtype=np.int64).ravel()
    pid = np.asarray(partition_id, dtype=np.int32).ravel()
    lag = np.asarray(lag, dtype=np.int64).ravel()
    o_pid = np.asarray(out_partition, dtype=np.int32).ravel()
    o_own = np.asarray(out_member_rank, dtype=np.int32).ravel()
    o_prev = np.asarray(prev_owner, dtype=np.int32).ravel()
    n, t_all = pid.size, po.size - 1
    if t_all < 0 or not (lag.size == o_pid.size == o_own.size == o_prev.size == n):
        raise ValueError("array sizes do not fit one layout")
    sticky = o_pid.copy()
    topic_kept = np.zeros(t_all, dtype=np.int64)
    topic_saved = np.zeros(t_all, dtype=np.int64)
    kept_before = changed = passed = 0
    for t in range(t_all):
        a, z = int(po[t]), int(po[t + 1])
        if not 0 <= a <= z <= n:
            raise ValueError("the offsets of topic %d leave the arrays" % t)
        p = z - a
        ids, oid = pid[a:z], o_pid[a:z]
        c, q = [int(x) for x in o_own[a:z]], [int(x) for x in o_prev[a:z]]
        before = sum(1 for i in range(p) if q[i] >= 0 and q[i] == c[i])
        kept_before += before
        topic_kept[t] = before
        if p > max_partitions:
            passed += 1
            continue
        by_id = np.argsort(ids, kind="stable")
        sorted_ids = ids[by_id]
        at = np.minimum(np.searchsorted(sorted_ids, oid), max(p - 1, 0))
        problem = None
        if np.unique(ids).size != p:
            problem = "a partition id appears twice in the input segment of topic %d" % t
        elif p and ((sorted_ids[at] != oid).any() or np.unique(oid).size != p):
            problem = "an output id of topic %d is no input id of the topic, or appears twice" % t
        if problem:
            if strict:
                raise ValueError(problem)
            passed += 1
            continue
        l = [int(x) for x in lag[a:z][by_id[at]]] if p else []
        src_of = list(range(p))                     # position -> the position its partition comes from
        r0 = 0
        while r0 < p:
            r1 = r0 + 1
            while r1 < p and l[r1] == l[r0]:
                r1 += 1
            s_of, w_of = {}, {}
            for i in range(r0, r1):
                if c[i] >= 0:
                    s_of.setdefault(c[i], []).append(i)             # 1
                if q[i] >= 0:
                    w_of.setdefault(q[i], []).append(i)             # 2
            placed, filled = set(), set()
            for member, s in s_of.items():
                w = w_of.get(member, [])
                for k in range(min(len(s), len(w))):                # 3
                    src_of[s[k]] = w[k]
                    placed.add(w[k])
                    filled.add(s[k])
            rest = [i for i in range(r0, r1) if i not in placed]
            holes = [i for i in range(r0, r1) if i not in filled]
            for src, dst in zip(rest, holes):                       # 4
                src_of[dst] = src
            r0 = r1
        for d in range(p):
            sticky[a + d] = oid[src_of[d]]                          # 5
        after = sum(1 for d in range(p) if q[src_of[d]] >= 0 and q[src_of[d]] == c[d])
        topic_kept[t] = after
        topic_saved[t] = after - before
        changed += 1 if any(src_of[d] != d for d in range(p)) else 0
    summary = np.array([kept_before, int(topic_kept.sum()), changed, passed], dtype=np.int64)
    return sticky, topic_kept, topic_saved, summary


def group_by_member_numpy(part_off, out_partition, member_rank, n_members: int):
    """la_group_by_member restated on the host -> (member_off int64[M+1], grouped_topic int32[N], grouped_partition int32[N]):
    the entries stably grouped by rank, those with rank -1 first (before member_off[0]).  The body of owned_after_round, and the
    yardstick tests/test_coop_gpu.py holds la_group_by_member_device to where it chains two rebalances on the device."""
    m = int(n_members)
    po = np.asarray(part_off, dtype=np.int64).ravel()
    pid = np.asarray(out_partition, dtype=np.int32).ravel()
    rank = np.asarray(member_rank, dtype=np.int64).ravel()
    if rank.size and (rank.min() < -1 or rank.max() >= m):
        raise ValueError("a member rank lies outside [-1, n_members)")
    order = np.argsort(rank, kind="stable")
    member_off = np.searchsorted(rank[order], np.arange(m + 1)).astype(np.int64)
    topic = (np.searchsorted(po, order, side="right") - 1).astype(np.int32)
    return member_off, topic, pid[order]


def cooperative_adjust_numpy(part_off, out_partition, out_member_rank, n_members: int, owned_off, owned_topic, owned_partition):
    """la_cooperative_adjust_device restated on the host -> (prev_owner int32[N], coop_member_rank int32[N], kept int64[M],
    fresh int64[M], pending int64[M], release int64[M], topic_withheld int64[T], summary int64[6]).  The target is
    (part_off, out_partition, out_member_rank); member r owns the entries [owned_off[r], owned_off[r+1]) of (owned_topic,
    owned_partition), entries outside [owned_off[0], owned_off[M]) are not looked at and an owned topic of -1 is stale.  With no
    owned entries owned_off may be None.  prev_owner[i] is the member that owns (topic of i, out_partition[i]) or -1;
    coop_member_rank[i] is the target rank c where that is -1 or c itself, otherwise -1 (withheld for this round).  Entries are
    KEPT (c >= 0, q == c), FRESH (c >= 0, q == -1), WITHHELD (c >= 0, q >= 0, q != c), DROPPED (c == -1, q >= 0) or idle;
    kept / fresh / pending count the first three by c, release counts WITHHELD + DROPPED by q, summary = kept, fresh, withheld,
    dropped, stale (owned entries looked at that matched nothing), followup (1 when withheld + dropped > 0).  ValueError for what
    the device reports as LA_EINVAL (a target rank outside [-1, M), an owned topic outside [-1, T), a (topic, id) claimed twice)
    and as LA_ESHAPE (owned offsets that do not ascend inside [0, n_owned], part_off that does not ascend from 0 to N).  The
    yardstick of the GPU tests."""
    m = int(n_members)
    po = np.asarray(part_off, dtype=np.int64).ravel()
    pid = np.asarray(out_partition, dtype=np.int64).ravel()
    c = np.asarray(out_member_rank, dtype=np.int64).ravel()
    o_topic = np.asarray(owned_topic if owned_topic is not None else [], dtype=np.int64).ravel()
    o_pid = np.asarray(owned_partition if owned_partition is not None else [], dtype=np.int64).ravel()
    n, n_owned = pid.size, o_topic.size
    if m < 0 or po.size < 1 or c.size != n or o_pid.size != n_owned:
        raise ValueError("n_members < 0, no part_off, or arrays that differ in length")
    t = po.size - 1
    if po[0] != 0 or po[-1] != n or (np.diff(po) < 0).any():
        raise ValueError("part_off does not ascend from 0 to the number of entries")
    if owned_off is None:
        if n_owned:
            raise ValueError("owned entries without owned_off")
        off = np.zeros(m + 1, dtype=np.int64)
    else:
        off = np.asarray(owned_off, dtype=np.int64).ravel()
    if off.size != m + 1 or off.min() < 0 or off.max() > n_owned or (np.diff(off) < 0).any():
        raise ValueError("owned_off must hold n_members + 1 offsets ascending inside [0, n_owned]")
    if n and (c.min() < -1 or c.max() >= m):
        raise ValueError("a target member rank lies outside [-1, n_members)")
    lo, hi = int(off[0]), int(off[-1])
    w_topic, w_pid = o_topic[lo:hi], o_pid[lo:hi]
    if w_topic.size and (w_topic.min() < -1 or w_topic.max() >= t):
        raise ValueError("an owned topic lies outside [-1, n_topics)")
    w_member = np.searchsorted(off, np.arange(lo, hi), side="right") - 1
    live = w_topic >= 0
    key = (w_topic[live] << 32) | (w_pid[live] & 0xFFFFFFFF)              # (topic, id) as one int64: topic < 2^31
    by_key = np.argsort(key, kind="stable")
    key, owner = key[by_key], w_member[live][by_key]
    if key.size > 1 and (key[1:] == key[:-1]).any():
        raise ValueError("a (topic, partition id) is claimed twice")
    topic = np.repeat(np.arange(t, dtype=np.int64), np.diff(po))
    want = (topic << 32) | (pid & 0xFFFFFFFF)
    at = np.searchsorted(key, want)
    hit = (at < key.size) & (key[np.minimum(at, max(key.size - 1, 0))] == want) if key.size else np.zeros(n, dtype=bool)
    q = np.where(hit, owner[np.minimum(at, max(key.size - 1, 0))], -1) if key.size else np.full(n, -1, dtype=np.int64)
    kept_e, fresh_e, held_e = (c >= 0) & (q == c), (c >= 0) & (q < 0), (c >= 0) & (q >= 0) & (q != c)
    drop_e = (c < 0) & (q >= 0)
    count = lambda idx: np.bincount(idx, minlength=m).astype(np.int64)[:m]
    kept, fresh, pending = count(c[kept_e]), count(c[fresh_e]), count(c[held_e])
    release = count(q[held_e | drop_e])
    topic_withheld = np.bincount(topic[held_e], minlength=t).astype(np.int64)[:t]
    n_held, n_drop = int(held_e.sum()), int(drop_e.sum())
    stale = int(w_topic.size) - int(hit.sum())
    summary = np.array([int(kept_e.sum()), int(fresh_e.sum()), n_held, n_drop, stale, 1 if n_held + n_drop else 0], dtype=np.int64)
    coop = np.where((q < 0) | (q == c), c, -1)
    return q.astype(np.int32), coop.astype(np.int32), kept, fresh, pending, release, topic_withheld, summary


def owned_after_round(part_off, out_partition, coop_member_rank, n_members: int):
    """Every member's owned list after it obeyed one adjusted assignment -> (owned_off int64[M+1], owned_topic int32[N],
    owned_partition int32[N]), ready to be the owned arrays of the next cooperative_adjust_numpy call.  A member then owns its
    KEPT and FRESH entries and nothing else (what was withheld or dropped it has revoked or never got), which is the
    group-by-member of coop_member_rank: the entries with rank -1 sit before owned_off[0], where the call does not look."""
    return group_by_member_numpy(part_off, out_partition, coop_member_rank, n_members)


def cooperative_round_numpy(part_off, out_partition, out_member_rank, n_members: int, owned_off, owned_topic, owned_partition):
    """la_cooperative_round[_device] restated on the host: cooperative_adjust_numpy, then owned_after_round on its adjusted ranks
    -> the eight outputs of the former followed by (member_off int64[M+1], grouped_topic int32[N], grouped_partition int32[N]).
    The withheld entries and those of topics without consumers sit before member_off[0]; the three lists are the owned arrays
    of the next round as they are.  ValueError as cooperative_adjust_numpy.  The yardstick of tests/test_coop_round_gpu.py."""
    adjusted = cooperative_adjust_numpy(part_off, out_partition, out_member_rank, n_members, owned_off, owned_topic, owned_partition)
    return adjusted + owned_after_round(part_off, out_partition, adjusted[1], n_members)


def cooperative_round_sticky_numpy(part_off, partition_id, lag, out_partition, out_member_rank, n_members: int, owned_off, owned_topic,
                                   owned_partition, *, max_partitions: int = STICKY_MAX_PARTITIONS):
    """la_cooperative_round_sticky_device restated on the host, as the composition its header defines and nothing else:
    cooperative_adjust_numpy on the target for prev_owner; sticky_ties_numpy with strict=False (a topic the device passes
    through is passed through) and max_partitions (the batch's hint, where it lies below the limit); cooperative_round_numpy
    with the sticky order in place of out_partition -> (sticky_partition int32[N], topic_kept int64[T], topic_saved int64[T],
    sticky_summary int64[4]) followed by the eleven outputs of cooperative_round_numpy, which describe the STICKY order.
    ValueError as cooperative_adjust_numpy.  The yardstick of tests/test_coop_sticky_gpu.py."""
    prev_owner = cooperative_adjust_numpy(part_off, out_partition, out_member_rank, n_members, owned_off, owned_topic, owned_partition)[0]
    sticky = sticky_ties_numpy(part_off, partition_id, lag, out_partition, out_member_rank, prev_owner,
                               max_partitions=max_partitions, strict=False)
    return sticky + cooperative_round_numpy(part_off, sticky[0], out_member_rank, n_members, owned_off, owned_topic, owned_partition)


def assign_cooperative_numpy(part_off, partition_id, lag, cons_off, cons_rank, n_members: int, owned_off, owned_topic,
                             owned_partition, *, assign):
    """la_assign_batch_cooperative restated on the host: cooperative_round_numpy over the target that
    assign(part_off, partition_id, lag, cons_off, cons_rank) -> (out_partition, out_member_rank, totals) produced -> those three
    followed by the eleven outputs of cooperative_round_numpy.  `assign` is the caller's restatement of the assign call (the
    tests pass the reference oracle's); ValueError as cooperative_adjust_numpy.  The yardstick of tests/test_assign_coop_gpu.py."""
    out_partition, out_member_rank, totals = assign(part_off, partition_id, lag, cons_off, cons_rank)
    return (out_partition, out_member_rank, totals) + cooperative_round_numpy(
        part_off, out_partition, out_member_rank, n_members, owned_off, owned_topic, owned_partition)


def assign_cooperative_sticky_numpy(part_off, partition_id, lag, cons_off, cons_rank, n_members: int, owned_off, owned_topic,
                                    owned_partition, *, assign, max_partitions: int = STICKY_MAX_PARTITIONS):
    """la_assign_batch_cooperative_sticky restated on the host: cooperative_round_sticky_numpy over the target that
    assign(part_off, partition_id, lag, cons_off, cons_rank) -> (out_partition, out_member_rank, totals) produced -> those three
    (the TARGET) followed by the fifteen outputs of cooperative_round_sticky_numpy (the sticky order).  `assign` is the caller's
    restatement of the assign call; max_partitions goes to cooperative_round_sticky_numpy (STICKY_ANY_SIZE: the call with
    LA_COOP_STICKY_LARGE); ValueError as cooperative_adjust_numpy."""
    out_partition, out_member_rank, totals = assign(part_off, partition_id, lag, cons_off, cons_rank)
    return (out_partition, out_member_rank, totals) + cooperative_round_sticky_numpy(
        part_off, partition_id, lag, out_partition, out_member_rank, n_members, owned_off, owned_topic, owned_partition,
        max_partitions=max_partitions)


PINNED_MAX_PARTITIONS = 4096      # LA_PINNED_MAX_PARTITIONS
PINNED_MAX_CONSUMERS = 2048       # LA_PINNED_MAX_CONSUMERS
PINNED_ANY_SIZE = (1 << 30) - 2   # LA_PINNED_LARGE_MAX_PARTITIONS: max_partitions of a call with LA_FLAG_PINNED_LARGE


def assign_pinned_numpy(part_off, partition_id, lag, cons_off, cons_rank, n_members: int, owned_off, owned_topic, owned_partition,
                        *, strict: bool = True, max_partitions: int = PINNED_MAX_PARTITIONS):
    """la_assign_pinned_device restated on the host, rule by rule -> (out_partition int32[N], out_member_rank int32[N],
    totals int64[K], topic_free int64[T], summary int64[4]).  For every topic: a partition whose claimant (the member whose
    owned slice holds (topic, id); owned lists as cooperative_adjust_numpy reads them) is one of the topic's consumers is PINNED
    and stays with it; every consumer's bin starts from its pinned partitions (count, wrapping int64 sum of lags); the
    positions are the reference's order (lag descending, signed; id ascending); walking them in that order every other
    partition -- unowned, or FOREIGN: claimed by a member that does not consume the topic -- goes to the consumer with the
    least (count, total, rank), which then counts it.  A topic without consumers gets rank -1 everywhere and none of its
    partitions is pinned.  topic_free[t]: the partitions of t that are not pinned; summary = pinned, free, foreign (part of
    free), stale (owned entries looked at that matched no partition, topic -1 included).  With nothing owned the result is the
    reference's assignment.  ValueError for what the device reports: offsets that do not ascend inside their arrays, a
    cons_rank segment that does not ascend strictly, an owned topic outside [-1, T), a (topic, id) claimed twice, and a topic of
    more than PINNED_MAX_PARTITIONS partitions or PINNED_MAX_CONSUMERS consumers -- with strict=False such a topic is skipped
    as the device skips it (its entries of the three results stay 0, it counts nowhere).  max_partitions: the partition limit;
    PINNED_ANY_SIZE stands for a call with LA_FLAG_PINNED_LARGE (the consumer limit stays).  The yardstick of
    tests/test_pinned_gpu.py and tests/test_pinned_large_gpu.py."""
    import heapq

    m = int(n_members)
    po = np.asarray(part_off, dtype=np.int64).ravel()
    co = np.asarray(cons_off, dtype=np.int64).ravel()
    pid = np.asarray(partition_id, dtype=np.int64).ravel()
    lags = np.asarray(lag, dtype=np.int64).ravel()
    ranks = np.asarray(cons_rank, dtype=np.int64).ravel()
    o_topic = np.asarray(owned_topic if owned_topic is not None else [], dtype=np.int64).ravel()
    o_pid = np.asarray(owned_partition if owned_partition is not None else [], dtype=np.int64).ravel()
    n, k_all, n_owned = pid.size, ranks.size, o_topic.size
    if m < 0 or po.size < 1 or co.size != po.size or lags.size != n or o_pid.size != n_owned:
        raise ValueError("n_members < 0, no part_off, or arrays that differ in length")
    t_all = po.size - 1
    if po[0] != 0 or po[-1] != n or (np.diff(po) < 0).any():
        raise ValueError("part_off does not ascend from 0 to the number of partitions")
    if co[0] != 0 or co[-1] != k_all or (np.diff(co) < 0).any():
        raise ValueError("cons_off does not ascend from 0 to the number of consumers")
    if owned_off is None:
        if n_owned:
            raise ValueError("owned entries without owned_off")
        off = np.zeros(m + 1, dtype=np.int64)
    else:
        off = np.asarray(owned_off, dtype=np.int64).ravel()
    if off.size != m + 1 or off.min() < 0 or off.max() > n_owned or (np.diff(off) < 0).any():
        raise ValueError("owned_off must hold n_members + 1 offsets ascending inside [0, n_owned]")
    owner, looked_at = {}, 0
    for r in range(m):
        for j in range(int(off[r]), int(off[r + 1])):
            looked_at += 1
            key = (int(o_topic[j]), int(o_pid[j]))
            if key[0] == -1:
                continue
            if key[0] < -1 or key[0] >= t_all:
                raise ValueError("an owned topic lies outside [-1, n_topics)")
            if key in owner:
                raise ValueError("a (topic, partition id) is claimed twice")
            owner[key] = r
    wrap = lambda x: ((x + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)
    out_pid, out_rank = np.zeros(n, np.int32), np.zeros(n, np.int32)
    totals, topic_free = np.zeros(k_all, np.int64), np.zeros(t_all, np.int64)
    pinned = free = foreign = hits = 0
    for t in range(t_all):
        p0, p1, c0, c1 = int(po[t]), int(po[t + 1]), int(co[t]), int(co[t + 1])
        r_t = ranks[c0:c1].tolist()
        if any(b <= a for a, b in zip(r_t, r_t[1:])):
            raise ValueError("a cons_rank segment does not ascend strictly")
        if p1 - p0 > max_partitions or c1 - c0 > PINNED_MAX_CONSUMERS:
            if strict:
                raise ValueError("topic %d exceeds the limits of the pinned assignment" % t)
            continue
        index_of = {r: k for k, r in enumerate(r_t)}
        ids, lg = pid[p0:p1], lags[p0:p1]
        order = np.lexsort((ids, ~lg))                               # lag descending (signed), id ascending
        ids, lg = ids[order].tolist(), lg[order].tolist()
        q = [owner.get((t, i), -1) for i in ids]                     # rule 1
        k_of = [index_of.get(x, -1) if x >= 0 else -1 for x in q]
        count, total = [0] * len(r_t), [0] * len(r_t)
        for k, l in zip(k_of, lg):                                   # rule 2
            if k >= 0:
                count[k] += 1
                total[k] = wrap(total[k] + l)
        heap = [(count[k], total[k], r_t[k], k) for k in range(len(r_t))]
        heapq.heapify(heap)
        for pos, (k, l) in enumerate(zip(k_of, lg)):                 # rules 3 and 4
            hits += q[pos] >= 0
            if k >= 0:
                pinned += 1
                out_rank[p0 + pos] = q[pos]
                continue
            free += 1
            foreign += q[pos] >= 0
            topic_free[t] += 1
            if not r_t:                                              # rule 5
                out_rank[p0 + pos] = -1
                continue
            cnt, tot, r, k = heapq.heappop(heap)
            out_rank[p0 + pos] = r
            total[k] = wrap(tot + l)
            heapq.heappush(heap, (cnt + 1, total[k], r, k))
        out_pid[p0:p1] = np.asarray(ids, np.int64).astype(np.int32)
        totals[c0:c1] = total
    summary = np.array([pinned, free, foreign, looked_at - hits], dtype=np.int64)
    return out_pid, out_rank, totals, topic_free, summary


def reduce_member_loads(partitions, lag, unassigned, group=None):
    """Partial roll-ups of the ranks' shards -> the group-wide roll-up on every rank: ONE all_reduce(SUM) over a single int64
    tensor of 2 * M + 1 entries (shards are disjoint topic ranges, so the sum of the partial roll-ups IS the roll-up; int64
    sums wrap like Java's).  It is also the group-wide reduction of la_assignment_moves_device's per-shard results, for the same
    reason: reduce_member_loads(gained, lost, moved) gives every rank the gained / lost counts and the moved total of the batch.  numpy arrays / host tensors travel as a host tensor (gloo), device tensors stay on their device
    (nccl = RCCL).  Returns (partitions, lag, unassigned) in the kind that came in (numpy in, numpy out)."""
    import torch
    import torch.distributed as dist

    as_numpy = not isinstance(partitions, torch.Tensor)
    p = torch.from_numpy(np.ascontiguousarray(partitions, dtype=np.int64)) if as_numpy else partitions
    g = torch.from_numpy(np.ascontiguousarray(lag, dtype=np.int64)) if not isinstance(lag, torch.Tensor) else lag
    m = p.numel()
    if g.numel() != m:
        raise ValueError("partitions and lag differ in length")
    buf = torch.empty(2 * m + 1, dtype=torch.int64, device=p.device)
    buf[:m] = p
    buf[m:2 * m] = g.to(p.device)
    buf[2 * m] = unassigned if isinstance(unassigned, torch.Tensor) else int(unassigned)
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    if as_numpy:
        out = buf.numpy()
        return out[:m].copy(), out[m:2 * m].copy(), int(out[2 * m])
    return buf[:m], buf[m:2 * m], buf[2 * m]
