"""The large path's radix sort (csrc/la_radix.hip) at its tile, digit, id-descent, tie-run and bound edges.  Not a test module:
test_sort_cases_cpu.py (the table holds what it says, proved on each case's own data) and test_large_sort_gpu.py (every case
through the C ABI against independent references) import it by name, so both run the same cases.

What is restated here are the sort's DECISIONS, in words and plain numpy, written from the source and never fitted to what a
device answers.  Expected RESULTS never come from this model: the partition order is ids[lexsort((ids, ~lags))], ranks and
totals are the oracle's.

The decisions.
  route         A topic of P partitions and C consumers takes the large path when it fits neither a wave tile (P <= 1024 and
                C <= 64) nor one workgroup of the block path (block_fits, la_kernels.h: P <= 8192 and C <= 2048, or P <= 16384
                and C <= 1024).  So 2 049 consumers are on the large path from P = 1 on, and a topic without consumers from
                P = 16 385 on: every `n` of the table is reached with one of the two.
  layout        The single-kernel passes run workgroups of 256 threads below 2^17 elements, of 512 below 3 * 2^20, of 1 024
                above; LA_SWEEP_THREADS (read per call) forces 256 or 1 024 and takes any other value as 512.  A tile is 16
                elements per thread.  The four-kernel passes (LA_FLAG_SORT_MULTIKERNEL) always use tiles of 4 096 and scan the
                tile counts in groups of 32 tiles.
  plan          key = lag ^ 0x7FFF..., val = id ^ 0x80000000; the 12 digits are val's 4 bytes, then key's 8, least significant
                first.  A digit that holds one value in every record is skipped.  The ids are "unsorted" when some id is smaller
                (signed) than the one before it; while they are not, the 4 id passes are skipped (stable passes keep the order).
                Keys first: the sort was laid out for it (LA_SORT_KEYS_FIRST=2 forces it on any size; by default from 2^22
                elements on and only when a sample of the lags shows no frequent one; never with the four-kernel passes), the
                ids are unsorted and some key digit is not constant.  Then the id passes are skipped too and the runs of equal
                keys are put in id order afterwards.
  repair        Over the key-sorted data in windows of 4 096 positions.  A run of two to four equal keys is settled where it is
                met; a window in which a run of MORE than four starts is flagged.  A flagged window takes every run that starts
                in it, from the first start in the window (position 0 of the data counts as a start) to the end of the last
                such run, if that end lies within 8 192 positions of the first start; if it does not, the sort is redone in
                full through the redo slots (ids first), which the profile shows as redone = 1 and as twice the key passes.
  bounds        LA_FLAG_BOUNDS: a key pass d is launched only when 8 d < bit length of the largest lag, an id pass only when
                8 d < bit length of the largest id; a partition outside the bounds is LA_EINVAL.
  group passes  la_group_by_member's radix form sorts key = rank + 1 <= n_members: one key pass per byte of n_members."""
import zlib
from collections import namedtuple

import numpy as np

from kafka_lag_based_assignor_amd import synth

WIDTHS = (256, 512, 1024)
ITEMS = 16                      # elements per thread of a pass
MULTI_TILE = 4096               # the four-kernel passes' tile
SCAN_ROWS = 32                  # ... and their scan groups, in tiles
DIGITS = 12                     # 4 id digits, then 8 key digits
WINDOW = 4096                   # tie repair
CAP = 8192
SETTLED = 4                     # runs of up to four are settled by the scan
C_LARGE = 2049                  # the fewest consumers that put a topic of any size on the large path
SORT_ONLY_MIN = 16385           # without consumers: the fewest partitions
PC_MAX = 30_000_000             # the literal oracle beside the round form up to here (as in packing_cases.py)
KEY_FLIP = np.uint64(0x7FFFFFFFFFFFFFFF)
ID_BIAS = np.uint32(0x80000000)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# ---- the decisions -----------------------------------------------------------------------------------------------------------
def block_fits(P, C):
    return (P <= 8192 and C <= 2048) or (P <= 16384 and C <= 1024)


def route(P, C):
    """ "large" | "block" | "tile" for one topic of a mixed batch (plan_batch, la_api.hip)."""
    if P <= 1024 and C <= 64:
        return "tile"
    return "block" if block_fits(P, C) else "large"


def sweep_threads(n, env=None):
    """Workgroup width of the single-kernel passes; env: the value of LA_SWEEP_THREADS, None where it is not set."""
    if env is not None:
        w = int(env)
        return w if w in (256, 1024) else 512
    return 1024 if n >= 3 << 20 else 512 if n >= 1 << 17 else 256


def tile_size(n, env=None, multi_kernel=False):
    return MULTI_TILE if multi_kernel else ITEMS * sweep_threads(n, env)


def n_tiles(n, env=None, multi_kernel=False):
    return -(-n // tile_size(n, env, multi_kernel))


def keys_of(lags):
    return np.ascontiguousarray(lags, np.int64).view(np.uint64) ^ KEY_FLIP


def vals_of(ids):
    return np.ascontiguousarray(ids, np.int32).view(np.uint32) ^ ID_BIAS


def constant_digits(ids, lags):
    """12 booleans: digit d holds one value in every record."""
    val, key = vals_of(ids), keys_of(lags)
    out = []
    for d in range(4):
        b = (val >> np.uint32(8 * d)) & np.uint32(0xFF)
        out.append(bool((b == b[0]).all()))
    for d in range(8):
        b = (key >> np.uint64(8 * d)) & np.uint64(0xFF)
        out.append(bool((b == b[0]).all()))
    return tuple(out)


def bounds_pass_mask(max_lag, max_id):
    """Bit d: pass d is launched under the bounds (0 <= lag <= max_lag, 0 <= id <= max_id)."""
    mask = 0
    for d in range(4):
        if 8 * d < int(max_id).bit_length():
            mask |= 1 << d
    for d in range(8):
        if 8 * d < int(max_lag).bit_length():
            mask |= 1 << (4 + d)
    return mask


def group_key_passes(n_members):
    d = 0
    while d < 8 and (n_members >> (8 * d)) != 0:
        d += 1
    return d


Repair = namedtuple("Repair", "flagged windows redone")
RepairWindow = namedtuple("RepairWindow", "window first last end fits")


def repair(sorted_keys):
    """The tie repair of a keys-first sort over the key-sorted data (any array whose equal neighbours are the equal keys: the
    lags in descending order do).  flagged: the windows in which a run of more than four starts; per flagged window the first and
    the last run start inside it, the end of the last such run and whether it lies within CAP of the first; redone: 1 if not."""
    k = np.asarray(sorted_keys)
    n = k.size
    start = np.ones(n, bool)
    start[1:] = k[1:] != k[:-1]
    pos = np.flatnonzero(start)
    ends = np.append(pos[1:], n)
    flagged = sorted(set((pos[(ends - pos) > SETTLED] // WINDOW).tolist()))
    windows = []
    for w in flagged:
        w0, w1 = w * WINDOW, min((w + 1) * WINDOW, n)
        inside = pos[(pos >= w0) & (pos < w1)]
        first, last = int(inside[0]), int(inside[-1])
        end = int(ends[np.searchsorted(pos, last)])                      # where the last run that starts in the window ends
        windows.append(RepairWindow(w, first, last, end, end <= first + CAP))
    return Repair(tuple(flagged), tuple(windows), int(any(not x.fits for x in windows)))


Plan = namedtuple("Plan", "constant unsorted_ids keys_first id_passes key_passes redone mask threads tiles")


def plan(ids, lags, sweep=None, keys_first_forced=False, bounds=None, multi_kernel=False):
    """What the sort decides on this topic.  (id_passes, key_passes, keys_first, redone) is what la_last_phase_times reports:
    the passes that are not skipped, over the sort's own slots and the redo slots together."""
    ids, lags = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lags, np.int64)
    n = ids.size
    assert n >= 1 and (keys_first_forced or n < 1 << 22), "the sampled decision is not restated here"
    constant = constant_digits(ids, lags)
    unsorted_ids = bool((ids[1:] < ids[:-1]).any())
    active_ids = sum(1 for d in range(4) if not constant[d])
    active_keys = sum(1 for d in range(4, DIGITS) if not constant[d])
    keys_first = bool(keys_first_forced and not multi_kernel and unsorted_ids and active_keys > 0)
    redone = 0
    if keys_first:
        redone = repair(np.sort(lags)[::-1]).redone
        id_passes, key_passes = (active_ids, 2 * active_keys) if redone else (0, active_keys)
    else:
        id_passes, key_passes = (active_ids if unsorted_ids else 0), active_keys
    mask = (1 << DIGITS) - 1 if bounds is None else bounds_pass_mask(*bounds)
    return Plan(constant, unsorted_ids, keys_first, id_passes, key_passes, redone, mask,
                sweep_threads(n, sweep), n_tiles(n, sweep, multi_kernel))


def expected_order(ids, lags):
    """The comparator's order: lag descending, id ascending."""
    return ids[np.lexsort((ids, ~np.asarray(lags, np.int64)))]


# ---- the case table ----------------------------------------------------------------------------------------------------------
# group: "a" .. "e"; n, C: the topic; sweep: LA_SWEEP_THREADS (None: not set); keys_first: LA_SORT_KEYS_FIRST=2; build: the
# generator's name in BUILDERS with its arguments; bounds: "tight" (the data's own maxima), None, or for a broken case the
# (max_lag, max_id) that one partition exceeds by one.
Case = namedtuple("Case", "group name n C sweep keys_first build args bounds broken")
CASES = []


def _add(group, name, n, build, args=(), C=C_LARGE, sweep=None, keys_first=False, bounds=None, broken=False):
    CASES.append(Case(group, name, n, C, sweep, keys_first, build, tuple(args), bounds, broken))


def case_id(c):
    return c.name


def seed_of(c):
    return zlib.crc32(c.name.encode())


# -- generators: (case, rng) -> (ids int32 [n], lags int64 [n]) ------------------------------------------------------------------
def _u40_ties(n, rng):
    lag = rng.integers(0, 1 << 40, n).astype(np.int64)
    tie = rng.random(n) < 0.1
    lag[tie] = lag[rng.integers(0, n, int(tie.sum()))]
    return lag


def _seven(n, rng):
    return (rng.integers(0, 7, n) * 1000).astype(np.int64)


def b_geometry(c, rng):
    """Lags u40 with about 10 % ties, ids shuffled."""
    return rng.permutation(c.n).astype(np.int32), _u40_ties(c.n, rng)


def b_key_digit(c, rng):
    """Byte d of the lag varies, the other seven are the same in every record; ids shuffled."""
    d, = c.args
    base = np.uint64(0x0123456789ABCDEF) & ~(np.uint64(0xFF) << np.uint64(8 * d))
    byte = rng.integers(0, 256, c.n).astype(np.uint64)
    byte[:256] = np.arange(256, dtype=np.uint64)                         # every value of the byte is there (n > 256)
    lag = (base | (rng.permutation(byte) << np.uint64(8 * d))).view(np.int64)
    return rng.permutation(c.n).astype(np.int32), lag


def b_extreme_lags(c, rng):
    lag = rng.integers(INT64_MIN, INT64_MAX, c.n, dtype=np.int64)
    special = np.array([INT64_MIN, -1, 0, 1, INT64_MAX] * 3, np.int64)   # each three times: ties at the extremes too
    lag[rng.choice(c.n, special.size, replace=False)] = special
    return rng.permutation(c.n).astype(np.int32), lag


def _by_id_rank(ids, per_rank):
    """lags such that the record with the r-th smallest id carries per_rank[r]: what a key pass meets at position r, the id
    passes having run before it."""
    lag = np.empty(ids.size, np.int64)
    lag[np.argsort(ids, kind="stable")] = per_rank
    return lag


def b_tile_one_bin_key(c, rng):
    """At the one key pass, every element of a tile has the same digit and the tiles differ."""
    tile, = c.args
    ids = rng.permutation(c.n).astype(np.int32)
    return ids, _by_id_rank(ids, np.arange(c.n, dtype=np.int64) // tile)


def b_tile_one_bin_id(c, rng):
    """At the one id pass (byte 2 of the id, lags all equal), every element of a tile has the same digit; tiles descend."""
    tile, = c.args
    t = np.arange(c.n, dtype=np.int64) // tile
    return ((t.max() - t) << 16).astype(np.int32), np.full(c.n, 77, np.int64)


def b_all_bins(c, rng):
    """At the one key pass every tile holds all 256 digits."""
    ids = rng.permutation(c.n).astype(np.int32)
    return ids, _by_id_rank(ids, np.arange(c.n, dtype=np.int64) % 256)


def b_255_single(c, rng):
    """At the one key pass 255 bins of a tile hold one element each and the rest of the tile is in one bin."""
    tile, = c.args
    r = np.arange(c.n, dtype=np.int64) % tile
    ids = rng.permutation(c.n).astype(np.int32)
    return ids, _by_id_rank(ids, np.where(r < 255, r + 1, 0))


def b_id_digit(c, rng):
    """Byte d of the id varies, the other three are the same in every record; lags all equal or seven-valued."""
    d, lag_kind = c.args
    base = np.uint32(0x01234567) & ~(np.uint32(0xFF) << np.uint32(8 * d))
    byte = rng.integers(0, 256, c.n).astype(np.uint32)
    byte[:256] = np.arange(256, dtype=np.uint32)
    ids = (base | (rng.permutation(byte) << np.uint32(8 * d))).view(np.int32)
    return ids, (np.full(c.n, -5, np.int64) if lag_kind == "equal" else _seven(c.n, rng))


def b_extreme_ids(c, rng):
    ids = rng.choice(np.arange(INT32_MIN, INT32_MAX, 4099, dtype=np.int64), c.n, replace=False).astype(np.int32)
    ids[rng.choice(c.n, 4, replace=False)] = np.array([INT32_MIN, -1, 0, INT32_MAX], np.int32)
    return ids, _u40_ties(c.n, rng)


def b_duplicate_ids(c, rng):
    return rng.integers(-50, 50, c.n).astype(np.int32), _seven(c.n, rng)


def b_one_descent(c, rng):
    """Ids ascending but for ids[j + 1] < ids[j]."""
    j, lag_kind = c.args
    ids = 3 * np.arange(c.n, dtype=np.int64) + 5
    ids[j + 1] = ids[j] - 1
    return ids.astype(np.int32), (np.full(c.n, 9, np.int64) if lag_kind == "equal" else _seven(c.n, rng))


def b_no_descent(c, rng):
    dup, lag_kind = c.args
    ids = np.arange(c.n, dtype=np.int64) // 2 - 100 if dup else 3 * np.arange(c.n, dtype=np.int64) - 100
    return ids.astype(np.int32), (np.full(c.n, 9, np.int64) if lag_kind == "equal" else _seven(c.n, rng))


def b_runs(c, rng):
    """Run geometry by construction: runs = ((start, length), ...) in SORTED positions, every other position a lag of its own.
    A run of value v starts at sorted position s when exactly s lags are larger; the values straddle zero."""
    runs, dup = c.args
    starts = np.ones(c.n, bool)
    for s, length in runs:
        assert 0 <= s and s + length <= c.n and starts[s:s + length].all(), (c.name, s, length)   # (runs do not touch)
        starts[s + 1:s + length] = False
    sorted_desc = np.int64(int(starts.sum()) // 2) - np.cumsum(starts).astype(np.int64)
    ids = rng.permutation(c.n)
    return (ids // 3 if dup else ids).astype(np.int32), rng.permutation(sorted_desc)


def b_bounded(c, rng):
    """Largest lag and largest id exactly as given, both present, ids shuffled with duplicates; broken: one partition one above."""
    max_lag, max_id, which = c.args
    lag = rng.integers(0, max_lag + 1, c.n).astype(np.int64)
    ids = rng.integers(0, max_id + 1, c.n).astype(np.int64)
    at = rng.choice(c.n, 3, replace=False)
    lag[at[0]], ids[at[1]] = max_lag, max_id
    if which == "lag":
        lag[at[2]] = max_lag + 1
    elif which == "id":
        ids[at[2]] = max_id + 1
    return ids.astype(np.int32), lag


BUILDERS = {f.__name__[2:]: f for f in (b_geometry, b_key_digit, b_extreme_lags, b_tile_one_bin_key, b_tile_one_bin_id, b_all_bins,
                                        b_255_single, b_id_digit, b_extreme_ids, b_duplicate_ids, b_one_descent, b_no_descent,
                                        b_runs, b_bounded)}


def data_of(c):
    """(ids, lags) of a case: a function of the case alone."""
    ids, lags = BUILDERS[c.build](c, np.random.default_rng(seed_of(c)))
    assert ids.dtype == np.int32 and lags.dtype == np.int64 and ids.size == c.n and lags.size == c.n, c.name
    return ids, lags


def bounds_of(c, ids, lags):
    """(max_lag, max_id) the call is given, or None."""
    if c.bounds == "tight":
        return int(lags.max()), int(ids.max())
    return c.bounds


# -- a. tile geometry ----------------------------------------------------------------------------------------------------------
for _w in WIDTHS:
    _T = ITEMS * _w
    for _n in (1, 2, 63, 64, 65, 1023, 1024, 1025, _T - 1, _T, _T + 1, 2 * _T, 3 * _T + 1):
        _add("a", "a-w%d-n%d" % (_w, _n), _n, "geometry", sweep=_w)
for _n in (131071, 131072, 131073):                                      # the natural switch 256 -> 512; 32 x 4096 -+ 1
    _add("a", "a-natural-n%d" % _n, _n, "geometry")
_add("a", "a-natural-n%d" % (64 * 4096 + 1), 64 * 4096 + 1, "geometry")  # two full scan groups of the four-kernel form and a tile
for _n in (3 * (1 << 20) - 1, 3 * (1 << 20)):                            # the natural switch 512 -> 1024, sort only
    _add("a", "a-natural-sortonly-n%d" % _n, _n, "geometry", C=0)

# -- b. digit geometry and c. one descent, at 3 tiles + 1 of every width ----------------------------------------------------------
for _w in WIDTHS:
    _T = ITEMS * _w
    _n = 3 * _T + 1
    _p = "w%d" % _w
    for _d in range(8):
        _add("b", "b-%s-keydigit%d" % (_p, _d), _n, "key_digit", (_d,), sweep=_w)
    _add("b", "b-%s-extreme-lags" % _p, _n, "extreme_lags", sweep=_w)
    _add("b", "b-%s-tile-one-bin-key" % _p, _n, "tile_one_bin_key", (_T,), sweep=_w)
    _add("b", "b-%s-tile-one-bin-id" % _p, _n, "tile_one_bin_id", (_T,), sweep=_w)
    _add("b", "b-%s-all-bins" % _p, _n, "all_bins", sweep=_w)
    _add("b", "b-%s-255-single" % _p, _n, "255_single", (_T,), sweep=_w)
    for _d in range(4):
        for _k in ("equal", "seven"):
            _add("b", "b-%s-iddigit%d-%s" % (_p, _d, _k), _n, "id_digit", (_d, _k), sweep=_w)
    _add("b", "b-%s-extreme-ids" % _p, _n, "extreme_ids", sweep=_w)
    _add("b", "b-%s-duplicate-ids" % _p, _n, "duplicate_ids", sweep=_w)
    for _j in (0, _n - 2, 255, 1023, _T - 1, _n // 2):
        for _k in ("equal", "seven"):
            _add("c", "c-%s-descent%d-%s" % (_p, _j, _k), _n, "one_descent", (_j, _k), sweep=_w)
    for _dup in (0, 1):
        for _k in ("equal", "seven"):
            _add("c", "c-%s-ascending-%s-%s" % (_p, "dups" if _dup else "strict", _k), _n, "no_descent", (_dup, _k), sweep=_w)

# -- d. keys first forced: run geometry ------------------------------------------------------------------------------------------
_ND = 12400                                                              # 4 tiles of 4 096; three windows and a short fourth


def _d(name, runs, n=_ND, dup=0):
    _add("d", "d-" + name, n, "runs", (tuple(runs), dup), keys_first=True)


for _L in (2, 3, 4, 5):                                                  # 5 is the first length that is flagged
    _d("len%d" % _L, [(100, _L), (4094, _L), (9000, _L)])
for _o in (4091, 4092, 4093, 4094, 4095):                                # a run of five up to and across the first window border
    _d("five-at-%d" % _o, [(_o, 5)])
for _L in (4096, 4097, 4098):                                            # window 1 begins with a run start: first = 4096, the limit is 4 097
    _d("w1-start-off4095-len%d" % _L, [(WINDOW + 4095, _L)])
for _L in (4096, 4097, 4098, 4099):                                      # window 1 begins inside a run of 7: first = 4097, the limit is 4 098
    _d("w1-inside-off4095-len%d" % _L, [(4090, 7), (WINDOW + 4095, _L)])
_d("short-run-ends-at-n", [(_ND - 6, 6)])
_d("long-run-ends-at-n-fits", [(8000, 4288)], n=WINDOW + CAP)              # first = 4096, the run ends at n = first + CAP
_d("long-run-ends-at-n-redo", [(8000, 4289)], n=WINDOW + CAP + 1)
_d("two-flagged-neighbours", [(100, 6), (4000, 200), (4300, 9), (8100, 50)])
_d("two-flagged-neighbours-dup-ids", [(100, 6), (4000, 200), (4300, 9), (8100, 50)], dup=1)
_d("window-inside-a-run", [(10, 9000)])                                  # window 1 lies wholly inside it: window 0 asks for the redo
_d("window-inside-a-run-fits", [(4090, 4102), (8300, 5)])                # ... a run that ends at 8 192 = 0 + CAP: window 0 takes it whole

# -- e. bounds on a digit border --------------------------------------------------------------------------------------------------
_NE = MULTI_TILE + 1
LAG_BORDERS = (0, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32)
ID_BORDERS = (0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)
for _m in LAG_BORDERS:
    _add("e", "e-maxlag%d" % _m, _NE, "bounded", (_m, 70000, ""), bounds="tight")
for _m in ID_BORDERS:
    _add("e", "e-maxid%d" % _m, _NE, "bounded", ((1 << 40) - 1, _m, ""), bounds="tight")
for _m in LAG_BORDERS:
    if _m & (_m + 1) == 0:                                               # 2^(8 d) - 1: one lag of 2^(8 d) breaks it
        _add("e", "e-broken-lag%d" % (_m + 1), _NE, "bounded", (_m, 70000, "lag"), bounds=(_m, 70000), broken=True)
for _m in ID_BORDERS:
    if _m & (_m + 1) == 0:
        _add("e", "e-broken-id%d" % (_m + 1), _NE, "bounded", ((1 << 40) - 1, _m, "id"), bounds=((1 << 40) - 1, _m), broken=True)

assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}


# ---- workloads -----------------------------------------------------------------------------------------------------------------
def ranks_of(C):
    return (2 * np.arange(C, dtype=np.int64) + 1).astype(np.int32)


def workload(topics, name="sort case"):
    """topics: [(ids, lags, C), ...] -> one batch."""
    ps, cs = [t[0].size for t in topics], [t[2] for t in topics]
    part_off = np.concatenate([[0], np.cumsum(ps)]).astype(np.int64)
    cons_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    ids = np.concatenate([t[0] for t in topics]).astype(np.int32)
    lag = np.concatenate([t[1] for t in topics]).astype(np.int64)
    ranks = np.concatenate([ranks_of(C) for C in cs] + [np.empty(0, np.int32)]).astype(np.int32)
    n = int(part_off[-1])
    return synth.Workload(name, len(topics), part_off, ids, np.zeros(n, np.int64), lag.copy(), np.zeros(n, np.int64), lag,
                          cons_off, ranks, max(ps), max(cs))


def companion_shape(c):
    """(n, C) of the second large topic of the side-by-side form: one tile more than the case (so the launch's grid is wider than
    the case's own tile count); next to the two 3 M-element sorts a small one, so that theirs is the wider."""
    if c.n > 1 << 20:
        return 20000, 0
    n2 = (n_tiles(c.n, c.sweep) + 1) * tile_size(c.n, c.sweep) + 77
    return (n2, C_LARGE) if c.C else (max(n2, SORT_ONLY_MIN), 0)


def companion_of(c, bounds):
    """(ids, lags, C): shuffled ids, u40 lags with ties -- inside the call's bounds where it has some."""
    n2, C2 = companion_shape(c)
    rng = np.random.default_rng(seed_of(c) + 1)
    if bounds is None:
        return rng.permutation(n2).astype(np.int32), _u40_ties(n2, rng), C2
    return rng.integers(0, bounds[1] + 1, n2).astype(np.int32), rng.integers(0, bounds[0] + 1, n2).astype(np.int64), C2


# ---- f. la_group_by_member, radix form --------------------------------------------------------------------------------------------
GROUP_N = 65537                                                          # one past the mid form's 32 x 2 048 entries
GROUP_MEMBERS = (255, 256, 257, 511, 65535, 65536, 65537)


def group_case(n_members):
    """(part_off, out_partition, out_member_rank): rank -1 and the highest rank present, member 3 crowded (a tenth of the
    entries), every member whose rank is 5 mod 7 empty."""
    rng = np.random.default_rng(n_members)
    m = rng.integers(-1, n_members, GROUP_N).astype(np.int64)
    m[rng.random(GROUP_N) < 0.1] = 3
    m[(m % 7 == 5) & (m != n_members - 1)] = 4
    at = rng.choice(GROUP_N, 4, replace=False)
    m[at[0]], m[at[1]], m[at[2]], m[at[3]] = -1, n_members - 1, n_members - 1, 0
    out_p = rng.integers(0, 1 << 20, GROUP_N).astype(np.int32)
    part_off = np.array([0, 1000, 1000, 40000, GROUP_N], np.int64)
    return part_off, out_p, m.astype(np.int32)


def expected_groups(part_off, out_p, out_m, n_members):
    """(member_off, grouped_topic, grouped_partition): the stable sort by member rank (_expected_groups of test_gpu_parity.py)."""
    order = np.argsort(out_m, kind="stable")
    topic_of = np.searchsorted(part_off, np.arange(out_p.size), side="right") - 1
    counts = np.bincount(out_m + 1, minlength=n_members + 1)
    return np.cumsum(counts)[: n_members + 1].astype(np.int64), topic_of[order].astype(np.int32), out_p[order]


# ---- g. bins in HBM: more consumers than one workgroup holds, a device sort of the totals per round -------------------------------
HUGE_SHAPES = ((5000, 9000), (8193 * 2 + 1, 8193))
HUGE_CASES = [(p, c, w) for p, c in HUGE_SHAPES for w in WIDTHS]


def huge_topic(p, c):
    rng = np.random.default_rng(p + c)
    return rng.permutation(p).astype(np.int32), _u40_ties(p, rng), c
