"""The case table of sort_cases.py holds what it was built to hold (no GPU): test_large_sort_gpu.py runs exactly these cases
through the large path's radix sort, and a case that does not reach the edge it is named after proves nothing about it.  Every
class is asserted from the model on the case's own data, never from the case's label; the model itself is held against
examples worked by hand."""
import numpy as np
import pytest

import sort_cases as sc
from oracle import oracle
from oracle.round_form import round_form

# Sum of P x C over the cases that the literal oracle walks (P x C <= PC_MAX each, about 1.5 ns a step): some five seconds here.
TABLE_PC_CAP = 4_000_000_000


@pytest.fixture(scope="module")
def table():
    """case name -> (ids, lags, plan, plan of the four-kernel form); read-only."""
    out = {}
    for c in sc.CASES:
        ids, lags = sc.data_of(c)
        b = sc.bounds_of(c, ids, lags)
        out[c.name] = (ids, lags, sc.plan(ids, lags, c.sweep, c.keys_first, b), sc.plan(ids, lags, c.sweep, c.keys_first, b, True))
    return out


def _of(table, group):
    return [(c,) + table[c.name] for c in sc.CASES if c.group == group]


# ---- the model against examples worked by hand ---------------------------------------------------------------------------------
def test_route_in_words():
    assert sc.route(1, 2049) == "large" and sc.route(1, 2048) == "block" and sc.route(1024, 64) == "tile"
    assert sc.route(16385, 0) == "large" and sc.route(16384, 0) == "block" and sc.route(8193, 1025) == "large"
    assert sc.route(8192, 2048) == "block" and sc.route(16384, 1024) == "block" and sc.route(1025, 1) == "block"


def test_layout_in_words():
    assert [sc.sweep_threads(n) for n in (1, 131071, 131072, 3145727, 3145728)] == [256, 256, 512, 512, 1024]
    assert [sc.sweep_threads(5, e) for e in ("256", "512", "1024", "300", "0")] == [256, 512, 1024, 512, 512]
    assert sc.tile_size(5, 1024) == 16384 and sc.tile_size(5, 1024, multi_kernel=True) == 4096
    assert [sc.n_tiles(n, 256) for n in (1, 4095, 4096, 4097, 8192, 12289)] == [1, 1, 1, 2, 2, 4]
    assert sc.n_tiles(131073) == 17 and sc.n_tiles(131071) == 32 and sc.n_tiles(131073, None, True) == 33


def test_bounds_pass_mask_in_words():
    # a largest lag of 255 needs one key pass, 256 needs two; 0 needs none; the id digits likewise
    assert sc.bounds_pass_mask(255, 0) == 0b0000_0001_0000 and sc.bounds_pass_mask(256, 0) == 0b0000_0011_0000
    assert sc.bounds_pass_mask(0, 0) == 0 and sc.bounds_pass_mask(0, 255) == 0b0001 and sc.bounds_pass_mask(0, 256) == 0b0011
    assert sc.bounds_pass_mask(65535, 65535) == 0b0000_0011_0011 and sc.bounds_pass_mask(65536, 65536) == 0b0000_0111_0111
    assert sc.bounds_pass_mask((1 << 32) - 1, (1 << 24) - 1) == 0b0000_1111_0111
    assert sc.bounds_pass_mask(1 << 32, 1 << 24) == 0b0001_1111_1111
    assert sc.bounds_pass_mask((1 << 63) - 1, (1 << 31) - 1) == 0xFFF
    assert [sc.group_key_passes(m) for m in (1, 255, 256, 257, 65535, 65536, 65537)] == [1, 1, 2, 2, 2, 3, 3]


def test_plan_on_hand_worked_topics():
    # lags 0 .. 255 under ids 0 .. 255 in order: id digit 0 and key digit 0 vary, the ids ascend -> one key pass, no id pass
    p = sc.plan(np.arange(256), np.arange(256), None, False, None)
    assert p.constant == (False, True, True, True, False) + (True,) * 7 and not p.unsorted_ids
    assert (p.id_passes, p.key_passes, p.keys_first, p.redone) == (0, 1, False, 0) and (p.threads, p.tiles) == (256, 1)
    # the same ids turned round: one id pass before it; forced keys first: no id pass, nothing to redo
    p = sc.plan(np.arange(256)[::-1], np.arange(256), None, False, None)
    assert p.unsorted_ids and (p.id_passes, p.key_passes, p.keys_first) == (1, 1, False)
    p = sc.plan(np.arange(256)[::-1], np.arange(256), None, True, None)
    assert (p.id_passes, p.key_passes, p.keys_first, p.redone) == (0, 1, True, 0)
    assert not sc.plan(np.arange(256)[::-1], np.arange(256), None, True, None, multi_kernel=True).keys_first
    # equal lags never go keys first (no key digit is active); ascending ids neither
    assert not sc.plan(np.arange(256)[::-1], np.zeros(256, np.int64), None, True, None).keys_first
    assert not sc.plan(np.arange(256), np.arange(256), None, True, None).keys_first
    # -1 and 0 differ in every byte of the key, so do the ids -1 and 0 (the id order is signed: -1 before 0 ascends)
    p = sc.plan(np.array([-1, 0]), np.array([0, -1]), None, False, None)
    assert p.constant == (False,) * 12 and not p.unsorted_ids and (p.id_passes, p.key_passes) == (0, 8)
    assert sc.plan(np.array([0, -1]), np.array([0, -1]), None, False, None).id_passes == 4
    # equal neighbours are no descent
    assert not sc.plan(np.array([1, 1, 2, 2]), np.zeros(4, np.int64), None, False, None).unsorted_ids
    # a run of 9 000 among 20 000 shuffled ids: keys first has to be redone -- 2 id passes (ids below 2^16), key passes twice
    lags = np.concatenate([np.full(9000, 5), np.arange(10, 11010)])
    p = sc.plan(np.arange(20000)[::-1], lags, None, True, None)
    assert (p.id_passes, p.key_passes, p.keys_first, p.redone) == (2, 4, True, 1)
    # the order itself: lag descending, then id ascending, signed
    assert sc.expected_order(np.array([3, -1, 2, 7], np.int32), np.array([5, 5, -9, 1 << 40])).tolist() == [7, -1, 3, 2]


def test_repair_on_hand_worked_runs():
    def keys(*runs):                                                    # (value, length), ...
        return np.concatenate([np.full(n, v) for v, n in runs])
    singles = lambda v0, n: [(v0 + i, 1) for i in range(n)]             # noqa: E731
    # runs of up to four are settled by the scan: nothing is flagged
    r = sc.repair(keys((9, 4), (8, 1), (7, 3), (6, 2)))
    assert r.flagged == () and r.redone == 0
    # five is flagged; the window's first start is position 0, the last start is the single key behind the run
    r = sc.repair(keys((9, 5), (8, 1)))
    assert r.flagged == (0,) and r.windows == (sc.RepairWindow(0, 0, 5, 6, True),) and r.redone == 0
    # a run is flagged where it STARTS: five keys from position 4 094 on belong to window 0, and window 1 is not flagged
    r = sc.repair(keys(*singles(100, 4094), (1, 5), *singles(5000, 200)))
    assert r.flagged == (0,) and r.windows[0][1:] == (0, 4094, 4099, True)
    # one run over everything: 8 192 keys fit (end == first + CAP), 8 193 do not
    assert sc.repair(np.zeros(8192)).windows == (sc.RepairWindow(0, 0, 0, 8192, True),)
    assert sc.repair(np.zeros(8193)).redone == 1
    # a window that begins inside a run counts from its own first start: 4 096 singles, a run of 10 across the border at 4 090 ..
    # 4 099, singles up to 8 190, then a run of 4 098 ending at 12 288 <= 4 100 + 8 192
    r = sc.repair(keys(*singles(0, 4090), (-1, 10), *singles(9000, 4091), (-2, 4098), (-3, 1)))
    assert r.flagged == (0, 1) and r.windows[1] == sc.RepairWindow(1, 4100, 8191, 12289, True) and r.redone == 0


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_large_path(table):
    for c in sc.CASES:
        assert sc.route(c.n, c.C) == "large", c.name
        n2, c2 = sc.companion_shape(c)
        assert sc.route(n2, c2) == "large" and sc.n_tiles(n2, c.sweep) != sc.n_tiles(c.n, c.sweep), c.name
        if c.sweep:                                                      # one tile class: the launch's grid is the companion's
            assert sc.n_tiles(n2, c.sweep) > sc.n_tiles(c.n, c.sweep), c.name
    for p, c, _ in sc.HUGE_CASES:
        assert sc.route(p, c) == "large" and c > 8192
    assert sc.GROUP_N == 32 * 2048 + 1


def test_every_width_at_its_tile_edges(table):
    for w in sc.WIDTHS:
        forced = {c.n for c in sc.CASES if c.group == "a" and table[c.name][2].threads == w and c.sweep is not None}
        tile = 16 * w
        assert {1, 2, 63, 64, 65, 1023, 1024, 1025, tile - 1, tile, tile + 1, 2 * tile, 3 * tile + 1} <= forced, w
        assert {table[c.name][2].tiles for c in sc.CASES if c.group == "a" and c.sweep == w} >= {1, 2, 4}
    natural = {(c.n, table[c.name][2].threads) for c in sc.CASES if c.sweep is None and c.group == "a"}
    assert {(131071, 256), (131072, 512), (131073, 512), (3 * 2**20 - 1, 512), (3 * 2**20, 1024)} <= natural
    # the four-kernel form's scan groups: 32 tiles (one group, the last tile one short), 33 and 65 tiles (a group of one tile)
    multi = {table[c.name][3].tiles for c in sc.CASES if c.sweep is None and c.group == "a"}
    assert {32, 33, 65} <= multi
    for c, ids, lags, p, _ in _of(table, "a"):
        assert 0 <= lags.min() and lags.max() < 1 << 40 and len(np.unique(ids)) == c.n
        if c.n >= 1023:                                                  # shuffled ids; about a tenth of the lags tie
            assert p.unsorted_ids and int(0.85 * c.n) <= len(np.unique(lags)) <= int(0.97 * c.n), c.name


def test_every_digit_is_the_only_active_one(table):
    for w in sc.WIDTHS:
        mine = [x for x in _of(table, "b") if x[0].sweep == w]
        assert all(x[0].n == 3 * 16 * w + 1 and x[3].tiles == 4 for x in mine)
        key_only = {tuple(d for d in range(4, 12) if not p.constant[d]) for _, _, _, p, _ in mine}
        assert {(d,) for d in range(4, 12)} <= key_only, w                                   # one active key pass, each digit
        only = {(tuple(d for d in range(12) if not p.constant[d]), p.unsorted_ids) for _, _, _, p, _ in mine}
        assert {((d,), True) for d in range(4)} <= only, w                                   # one active pass in all: an id digit
        with_keys = {tuple(d for d in range(4) if not p.constant[d]) for _, _, _, p, _ in mine
                     if p.unsorted_ids and p.key_passes > 0}
        assert {(d,) for d in range(4)} <= with_keys, w                                      # ... and with key passes behind it


def test_digit_cases_hold_their_bins(table):
    for c, ids, lags, p, _ in _of(table, "b"):
        tile = 16 * c.sweep
        by_id = np.argsort(ids, kind="stable")                           # what the first key pass reads, after the id passes
        key0 = ((sc.keys_of(lags)[by_id]) & np.uint64(0xFF)).astype(np.int64)
        tiles = [key0[t:t + tile] for t in range(0, c.n, tile)]
        if c.build == "tile_one_bin_key":
            assert p.key_passes == 1 and not p.constant[4] and all(len(set(t.tolist())) == 1 for t in tiles)
            assert len({int(t[0]) for t in tiles}) == len(tiles) == 4
        elif c.build == "tile_one_bin_id":
            d2 = ((sc.vals_of(ids) >> np.uint32(16)) & np.uint32(0xFF)).astype(np.int64)
            per = [d2[t:t + tile] for t in range(0, c.n, tile)]
            assert (p.id_passes, p.key_passes) == (1, 0) and all(len(set(t.tolist())) == 1 for t in per)
            assert len({int(t[0]) for t in per}) == 4
        elif c.build == "all_bins":
            assert p.key_passes == 1 and all(len(set(t.tolist())) == 256 for t in tiles[:3])
        elif c.build == "255_single":
            for t in tiles[:3]:
                cnt = np.bincount(t, minlength=256)
                assert p.key_passes == 1 and sorted(cnt.tolist()) == [1] * 255 + [tile - 255]
        elif c.build == "extreme_lags":
            assert {sc.INT64_MIN, -1, 0, 1, sc.INT64_MAX} <= set(lags.tolist()) and p.key_passes == 8
        elif c.build == "extreme_ids":
            assert {sc.INT32_MIN, -1, 0, sc.INT32_MAX} <= set(ids.tolist()) and p.id_passes == 4
        elif c.build == "duplicate_ids":
            assert len(np.unique(ids)) < c.n // 100 and p.unsorted_ids
        elif c.build == "key_digit":
            d = c.args[0]
            assert len(np.unique((sc.keys_of(lags) >> np.uint64(8 * d)) & np.uint64(0xFF))) == 256
            assert (lags < 0).any() == (d == 7) and (d != 7 or (lags >= 0).any())           # digit 7 carries the sign


def test_descents_are_where_the_names_say(table):
    for w in sc.WIDTHS:
        tile, n = 16 * w, 3 * 16 * w + 1
        for kind_equal in (True, False):
            at = set()
            plain = set()
            for c, ids, lags, p, _ in _of(table, "c"):
                if c.sweep != w or (len(np.unique(lags)) == 1) != kind_equal:
                    continue
                assert c.n == n and (kind_equal or len(np.unique(lags)) == 7)
                down = np.flatnonzero(ids[1:] < ids[:-1])
                if down.size:
                    assert down.size == 1 and p.unsorted_ids and p.id_passes > 0 and not p.keys_first
                    at.add(int(down[0]))
                else:
                    assert not p.unsorted_ids and p.id_passes == 0
                    plain.add(bool((ids[1:] == ids[:-1]).any()))
                    # ... and the input order stands: a stable sort by the lag alone gives the comparator's order
                    np.testing.assert_array_equal(sc.expected_order(ids, lags), ids[np.argsort(~lags, kind="stable")])
            assert at == {0, n - 2, 255, 1023, tile - 1, n // 2}, (w, kind_equal, at)
            assert plain == {True, False}, (w, kind_equal)                # with and without equal neighbours


def _run_lengths(lags):
    s = np.sort(lags)
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return np.diff(np.append(start, s.size))


def test_runs_on_both_sides_of_every_limit(table):
    d = {c.name: (c, ids, lags, p, sc.repair(np.sort(lags)[::-1])) for c, ids, lags, p, _ in _of(table, "d")}
    for c, ids, lags, p, r in d.values():
        assert p.keys_first and p.unsorted_ids and (lags < 0).any() and (lags > 0).any(), c.name
        assert p.redone == r.redone and sc.n_tiles(c.n) >= 3
        # (lags on both sides of zero differ in all 8 bytes of the key; 12 400 ids differ in 2; a redo runs the key passes twice)
        assert (p.id_passes, p.key_passes) == ((2, 16) if r.redone else (0, 8)), c.name
    assert any(len(np.unique(ids)) < c.n for c, ids, _, _, _ in d.values())                  # duplicate ids once
    # settled by the scan up to four, flagged from five on
    for L in (2, 3, 4):
        c, _, lags, _, r = d["d-len%d" % L]
        assert _run_lengths(lags).max() == L and r.flagged == ()
    c, _, lags, _, r = d["d-len5"]
    assert _run_lengths(lags).max() == 5 and r.flagged == (0, 2) and r.redone == 0          # (the run at 4 094 is window 0's)
    # a run of five up to and across the window border is flagged in the window where it starts
    for o in (4091, 4092, 4093, 4094, 4095):
        r = d["d-five-at-%d" % o][4]
        assert r.flagged == (0,) and r.windows[0][1:] == (0, o, o + 5, True), o          # (nothing starts behind it in window 0)
    # the capacity, met from both sides, with the first start at the window's first position and one position in
    for names, first, limit in ((["d-w1-start-off4095-len%d" % L for L in (4096, 4097, 4098)], 4096, 4097),
                                (["d-w1-inside-off4095-len%d" % L for L in (4096, 4097, 4098, 4099)], 4097, 4098)):
        seen = set()
        for name in names:
            c, _, lags, _, r = d[name]
            w = [x for x in r.windows if x.window == 1][0]
            L = w.end - w.last
            assert (w.first, w.last) == (first, 8191) and _run_lengths(lags).max() == L, name
            assert w.fits == (L <= limit) and r.redone == (0 if L <= limit else 1), name
            seen.add(L - limit)
        assert {-1, 0, 1} <= seen
    # a run that ends exactly at n: short; long at the capacity exactly; one more
    c, _, _, _, r = d["d-short-run-ends-at-n"]
    assert r.windows[-1].end == c.n and r.redone == 0
    c, _, _, _, r = d["d-long-run-ends-at-n-fits"]
    assert r.windows == (sc.RepairWindow(1, 4096, 8000, c.n, True),) and c.n == 4096 + sc.CAP
    c, _, _, _, r = d["d-long-run-ends-at-n-redo"]
    assert r.windows == (sc.RepairWindow(1, 4096, 8000, c.n, False),) and r.redone == 1
    for name in ("d-two-flagged-neighbours", "d-two-flagged-neighbours-dup-ids"):
        assert d[name][4].flagged == (0, 1) and d[name][4].redone == 0
    # a window wholly inside a run starts nothing and is not flagged: the window before it decides
    r = d["d-window-inside-a-run"][4]
    assert r.flagged == (0,) and r.windows[0][1:] == (0, 10, 9010, False) and r.redone == 1
    r = d["d-window-inside-a-run-fits"][4]
    assert r.flagged == (0, 2) and r.windows[0][1:] == (0, 4090, 8192, True) and r.windows[1].first == 8192 and r.redone == 0
    assert {x[4].redone for x in d.values()} == {0, 1}


def test_bounds_sit_on_the_digit_borders(table):
    lag_side, id_side, broken = {}, {}, set()
    for c, ids, lags, p, _ in _of(table, "e"):
        b = sc.bounds_of(c, ids, lags)
        assert lags.min() >= 0 and ids.min() >= 0 and sc.n_tiles(c.n) == 2 and p.mask == sc.bounds_pass_mask(*b), c.name
        if c.broken:
            over_lag, over_id = np.flatnonzero(lags > b[0]), np.flatnonzero(ids > b[1])
            assert over_lag.size + over_id.size == 1, c.name
            top, bound = (int(lags.max()), b[0]) if over_lag.size else (int(ids.max()), b[1])
            assert top == bound + 1 and top & (top - 1) == 0 and top.bit_length() % 8 == 1, c.name      # 2^(8 d), one above the bound
            assert sc.bounds_pass_mask(*b) != sc.bounds_pass_mask(int(lags.max()), int(ids.max()))     # a pass would be missing
            broken.add(("lag" if over_lag.size else "id", top))
        else:
            assert b == (int(lags.max()), int(ids.max()))                                    # tight
            # every pass the mask keeps is one the data needs, every one it drops is constant: the mask is exact on this data
            for dgt in range(12):
                assert ((p.mask >> dgt) & 1) == (0 if p.constant[dgt] else 1), (c.name, dgt)
            lag_side[b[0]] = bin(p.mask >> 4).count("1")
            id_side[b[1]] = bin(p.mask & 15).count("1")
    want_l = {0: 0, 255: 1, 256: 2, 65535: 2, 65536: 3, 2**32 - 1: 4, 2**32: 5}
    want_i = {0: 0, 255: 1, 256: 2, 65535: 2, 65536: 3, 2**24 - 1: 3, 2**24: 4}
    assert {k: lag_side[k] for k in want_l} == want_l and {k: id_side[k] for k in want_i} == want_i
    assert broken == {("lag", 1), ("lag", 256), ("lag", 65536), ("lag", 2**32), ("id", 1), ("id", 256), ("id", 65536), ("id", 2**24)}


def test_group_cases_reach_the_pass_borders():
    assert [sc.group_key_passes(m) for m in sc.GROUP_MEMBERS] == [1, 2, 2, 2, 2, 3, 3]
    for m in sc.GROUP_MEMBERS:
        part_off, out_p, out_m = sc.group_case(m)
        assert out_m.size == sc.GROUP_N == part_off[-1] and out_m.min() == -1 and out_m.max() == m - 1
        cnt = np.bincount(out_m + 1, minlength=m + 1)
        assert cnt[4] > sc.GROUP_N // 20 and (cnt[1:] == 0).sum() >= m // 8                  # member 3 crowded; empty members
        # the highest key, rank + 1 = n_members, needs every pass: its top byte differs from every other key's where a pass is new
        assert (m >> (8 * (sc.group_key_passes(m) - 1))) > 0
        off, g_t, g_p = sc.expected_groups(part_off, out_p, out_m, m)
        assert off[0] == cnt[0] and off[-1] == sc.GROUP_N and (np.diff(off) >= 0).all()
        assert (np.diff(out_m[np.argsort(out_m, kind="stable")]) >= 0).all() and set(g_t.tolist()) == {0, 2, 3}


def test_references_agree_and_the_oracle_work_is_capped(table):
    """Ranks and totals of the GPU test come from the round form: here it is held against the literal oracle on the same topics
    wherever that is affordable, and the partition order of both against the comparator written out."""
    work = 0
    for c in sc.CASES:
        ids, lags = table[c.name][:2]
        w = sc.workload([(ids, lags, c.C)])
        exp = round_form(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
        np.testing.assert_array_equal(exp[0], sc.expected_order(ids, lags), err_msg=c.name)
        if c.C == 0:
            assert (exp[1] == -1).all()
        if 0 < c.n * c.C <= sc.PC_MAX:
            work += c.n * c.C
            lit = oracle.assign_flat(w.part_off, w.partition_id, w.lag, w.cons_off, w.cons_rank)
            for g, e, what in zip(exp, lit, ("partition order", "member", "totals")):
                np.testing.assert_array_equal(g, e, err_msg="round form vs literal, %s: %s" % (what, c.name))
    assert 0 < work <= TABLE_PC_CAP, work
    for p, c, _ in sc.HUGE_CASES:
        assert p * c > sc.PC_MAX                                         # (the round form alone; test_large_gpu.py holds it at such shapes)


def test_no_case_is_lost():
    groups = {g: sum(1 for c in sc.CASES if c.group == g) for g in "abcde"}
    assert groups == {"a": 45, "b": 69, "c": 48, "d": 23, "e": 22}, groups
    assert all(c.build in sc.BUILDERS for c in sc.CASES) and len(sc.HUGE_CASES) == 6 and len(sc.GROUP_MEMBERS) == 7
