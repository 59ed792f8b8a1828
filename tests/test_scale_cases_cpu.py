"""scale_cases.py holds what it says, without a GPU: every case crosses the threshold it names -- by the arithmetic of the sources,
for 256 and for 304 compute units -- with large-topic positions within 1.7 x what the threshold needs; the vectorised pinned
builder yields valid owned lists and sharding.assign_pinned_numpy agrees with the dictionary model on them; the sticky yardstick
agrees with the independent model where digit 10 is in use; the sticky `past one grid` case holds the runs it promises."""
import numpy as np
import pytest

import pinned_large_cases as PL
import scale_cases as X
import sticky_cases as S
import sticky_large_cases as SL

CUS = (256, 304)


def _within_cap(positions, need):
    assert need <= positions <= X.CAP * need, (positions, need)


# ---- pinned ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_pinned_cases_cross_their_thresholds(cus):
    grid, groups = X.grid_of(cus), X.LEVEL_GROUPS_PER_CU * cus
    # classes out of order
    shapes = X.PINNED_SHAPES["classes out of order"](cus)
    big = X.pinned_large(shapes)
    classes = [X.tile_class(p) for p in big]
    assert sorted(set(classes)) == [256, 512] and classes != sorted(classes), "the item order is the topic order"
    assert [X.tile_class(n) for n in (131071, 131072, 131073)] == [256, 512, 512] and {131071, 131072, 131073} <= set(big)
    assert any(p <= X.LIMIT for p, _ in shapes), "no small neighbour"
    _within_cap(sum(big), X.pinned_need("classes out of order", cus))
    # three classes
    shapes = X.PINNED_SHAPES["three classes"](cus)
    big = X.pinned_large(shapes)
    assert [X.tile_class(p) for p in big[:3]] == [1024, 256, 512] and len(big) == len(shapes)
    assert X.tile_class(3 * 2**20 - 1) == 512
    steps = X.steps_of(big)
    assert steps > grid and steps == 3073 + 5 + 128 + 5 * (len(big) - 3)
    assert X.scan_per(steps) == 4 and X.idle_scan_threads(steps) > 0
    assert len(big) <= groups
    _within_cap(sum(big), X.pinned_need("three classes", cus))
    # more topics than level workgroups
    shapes = X.PINNED_SHAPES["more topics than level workgroups"](cus)
    big = X.pinned_large(shapes)
    assert len(big) == len(shapes) == groups + 1 and X.steps_of(big) == 10 * cus + 5 > grid
    assert {X.tile_class(p) for p in big} == {256}
    # topic 2 x CUs is the one a workgroup (the first) meets second: consumers, free partitions, another C than topic 0's
    held = X.more_topics_held(cus)
    second, owned = shapes[groups], X.more_topics_owned(cus)
    assert second == X.SECOND_TOPIC and second[1] > 0 and second[1] != shapes[0][1] > 0 and groups not in held
    assert len(owned) == len(shapes) and owned[groups] == 0.5 and second[0] * (1 - owned[groups]) > 100 * second[1]
    assert all(shapes[t][1] != shapes[t + 1][1] for t in range(groups - 1))
    assert sorted(held) == [t for t, (_, c) in enumerate(shapes) if t % 5 == 0 and c > 0 and t < groups]
    assert all(len(h) == shapes[t][1] and h[0] == 0 and min(h[1:] or [1]) > 0 for t, h in held.items())
    _within_cap(sum(big), X.pinned_need("more topics than level workgroups", cus))


@pytest.mark.parametrize("name", list(X.PINNED))
def test_the_vectorised_builder_yields_valid_owned_lists(name):
    c = X.PINNED[name](256)
    assert c.shapes() == [tuple(s) for s in X.PINNED_SHAPES[name](256)]
    assert c.owned_off.size == c.m + 1 and c.owned_off[0] == 0 and c.owned_off[-1] == c.n_owned and (np.diff(c.owned_off) >= 0).all()
    assert ((c.owned_topic >= 0) & (c.owned_topic < c.t)).all()
    key = c.owned_topic.astype(np.int64) << 32 | c.owned_pid.astype(np.int64) & 0xFFFFFFFF
    assert np.unique(key).size == key.size, "a (topic, id) is claimed twice"
    for t in range(c.t):
        r = c.cons_rank[int(c.cons_off[t]):int(c.cons_off[t + 1])]
        assert (np.diff(r) > 0).all() and (r.size == 0 or (0 <= r[0] and r[-1] < c.m))
        ids = c.pid[int(c.part_off[t]):int(c.part_off[t + 1])]
        assert np.array_equal(np.sort(ids), np.arange(ids.size))
    member = np.repeat(np.arange(c.m), np.diff(c.owned_off))
    n_of = np.diff(c.part_off)
    stale = c.owned_pid >= n_of[c.owned_topic]
    consumes = np.zeros(c.n_owned, bool)
    for t in np.unique(c.owned_topic):
        at = c.owned_topic == t
        consumes[at] = np.isin(member[at], c.cons_rank[int(c.cons_off[t]):int(c.cons_off[t + 1])])
    assert stale.sum() > 0 and (~consumes & ~stale).sum() > 0, "no stale or no foreign claim"
    share = (~stale).sum() / c.n
    assert 0.3 < share < 0.7, share
    if name == "more topics than level workgroups":
        per_topic = np.bincount(c.owned_topic[~stale], minlength=c.t) / n_of
        plain = [t for t in range(c.t) if t not in X.more_topics_held(256)]
        np.testing.assert_allclose(per_topic[plain], np.array(X.more_topics_owned(256))[plain], atol=0.05)
        assert 0.45 < per_topic[c.t - 1] < 0.55, "the topic met second has no free partitions"


def test_assign_pinned_numpy_is_the_dictionary_model_on_classes_out_of_order():
    c, exp = X.pinned_case("classes out of order", 256)
    for k, g, e in zip(PL.pinned_cases.OUTPUTS, exp, PL.model(c)):
        np.testing.assert_array_equal(g, e, err_msg=k)
    assert exp[4][0] > 0 and exp[4][2] > 0 and exp[4][3] >= 6, "pinned, foreign and stale claims: %s" % exp[4]


# ---- sticky ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_sticky_cases_cross_their_thresholds(cus):
    digit10 = 1 << 10
    facts = {}
    for name in X.STICKY:
        w = X.STICKY[name](cus)
        ps = [int(w.part_off[t + 1] - w.part_off[t]) for t in SL.big_topics(w)]
        n_pos = sum(ps)
        facts[name] = (w, ps, n_pos)
        if name != "digit 10, below":
            _within_cap(n_pos, X.sticky_need(name, cus))
    assert [facts["digit 10, " + k][2] for k in ("below", "at", "above")] == [65535, 65536, 65537]
    assert not X.sticky_pass_mask(65535) & digit10 and X.sticky_pass_mask(65536) & digit10 and X.sticky_pass_mask(65537) & digit10
    assert not X.sticky_pass_mask((1 << 24) - 1) & (1 << 11)
    assert [X.tile_class(2 * n) for n in (65535, 65536)] == [256, 512]
    # digit 10 in use
    w, ps, n_pos = facts["digit 10 in use"]
    assert X.sticky_pass_mask(n_pos) & digit10 and X.tile_class(2 * n_pos) == 512 and 2 * n_pos <= X.MATCH_ELEMENTS
    assert ps == [150000, 4097, 60000] and w.n_topics == 4
    assert ps[0] > 65536, "no topic of the list starts past position 65 536"
    a, b = X.DIGIT10_RUNS
    assert a != b and (a ^ b) & ~0xFF0000 == 0 and b + 9 <= ps[0]      # the two run starts differ in the third byte only
    # match strides
    w, ps, n_pos = facts["match strides"]
    assert len(ps) == 3 and 2 * n_pos > X.MATCH_ELEMENTS and 2 * (n_pos - 9) <= X.MATCH_ELEMENTS
    # past one grid
    w, ps, n_pos = facts["past one grid"]
    steps = X.steps_of(ps)
    assert n_pos > X.STEP * X.grid_of(cus) and steps > X.grid_of(cus)
    assert n_pos > 3 * 2**19 and X.tile_class(2 * n_pos) == 1024 and X.scan_per(steps) >= 3
    assert ps[:2] == [1600000, 300000] and all(X.LIMIT < p <= 9000 for p in ps[2:]) and len(ps) > 3
    assert max(int(c) for c in np.diff(w.cons_off)) <= 7
    assert n_pos < 1 << 24, "digit 11 is left out"


def test_run_bounds_is_groups_of_on_a_small_case():
    w, res = SL.case("straddle")
    starts, ends = X.run_bounds(w, res)
    runs = SL.groups_of(w, res, SL.prev_of("straddle"))
    assert [(a, z) for a, z, _ in runs] == list(zip(starts.tolist(), ends.tolist()))


def test_the_sticky_past_one_grid_case_holds_the_runs_it_promises():
    cus = 256
    w, res = X.sticky_case("past one grid", cus)
    starts, ends = X.run_bounds(w, res)
    bounds = set(zip(starts.tolist(), ends.tolist()))
    big = SL.big_topics(w)
    assert big[0] == 0, "positions of the first topic are positions of the list"
    share = X.scan_per(X.steps_of(int(w.part_off[t + 1] - w.part_off[t]) for t in big)) * X.STEP
    (a, n), (b, k) = X.past_one_grid_runs(cus)
    assert (a, a + n) in bounds and (b, b + k) in bounds
    assert n > 3 * X.STEP and n > share and a < -(-a // share) * share and (-(-a // share) + 1) * share < a + n, "no whole share of K3 inside"
    assert (b + k) % X.STEP == 0 and b % X.STEP != 0
    q0 = np.cumsum([0] + [int(w.part_off[t + 1] - w.part_off[t]) for t in big])[:-1]
    first = dict(zip(starts.tolist(), ends.tolist()))
    assert all(first[int(q)] == int(q) + 1 for q in q0), "a large topic does not begin with a run of one"
    length = ends - starts
    assert (length == 1).sum() > 1000 and ((length > 7) & (length < 200)).sum() > 1000


def test_the_sticky_model_is_the_yardstick_where_digit_10_is_in_use():
    w, res = X.sticky_case("digit 10 in use", 256)
    starts, ends = X.run_bounds(w, res)
    bounds = set(zip(starts.tolist(), ends.tolist()))
    assert all((s, s + 9) in bounds for s in X.DIGIT10_RUNS)
    prev = X.sticky_prev("digit 10 in use", 256, "shifted")
    exp = X.sticky_expected("digit 10 in use", 256, "shifted")
    sticky, before, after = S.model(w, res, prev)
    np.testing.assert_array_equal(exp[0], sticky)
    np.testing.assert_array_equal(exp[1], after)
    np.testing.assert_array_equal(exp[2], after - before)
    assert exp[3][3] == 0 and exp[3][1] > exp[3][0]


# ---- verify ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_the_verify_case_crosses_its_thresholds(cus):
    shapes = X.verify_shapes(cus)
    grid, base = X.grid_of(cus), X.verify_partition_topics(cus)
    assert base == 2 * cus + 2 and all(p > X.LIMIT for p, _ in shapes[:base])
    assert all(s == X.CONSUMER_LARGE and s[0] <= X.LIMIT < s[1] for s in shapes[base:])
    assert X.domain_steps((X.LIMIT + 1, 64)) == (5, 1, 2) and X.domain_steps(shapes[X.VERIFY_WIDE]) == (5, 5, 17)
    assert X.domain_steps(X.CONSUMER_LARGE) == (1, 5, 17)
    first, (part, cons, pair) = X.first_steps(shapes)
    # every phase has more steps than one grid; phase 2 reaches each of its pair steps on a later trip only
    assert part > grid and cons > grid and pair > grid and part == 10 * cus + 10 + len(shapes) - base
    assert cons - X.domain_steps(X.CONSUMER_LARGE)[1] < grid + X.domain_steps(X.CONSUMER_LARGE)[1], "more consumer-large topics than needed"
    faults = X.verify_faults(cus)
    assert sorted(faults) == list(range(base - 5, base)) + [len(shapes) - 2, len(shapes) - 1]
    classes = 0
    for t, name in faults.items():
        classes |= X.FAULT_CLASS[name]
        p0, c0, q0 = first[t]
        if t < base:                                                     # found in a partition step of phases 1, 2 or 5
            assert shapes[t] == (X.LIMIT + 1, 64) and p0 >= grid, (name, p0)
        elif name == "total + 1":                                        # found in a consumer step of phase 3
            assert X.FAULT_CLASS[name] == X.V.TOTALS and c0 >= grid, (name, c0)
        else:                                                            # phase 4 leaves it in a pair step, phase 5 finds it behind the partition steps
            assert name == X.LEFT_OUT and q0 >= grid and part + c0 >= grid, (name, q0)
    assert classes == 31
    assert (X.LIMIT + 1 - 1) // X.STEP == 4 == X.domain_steps((X.LIMIT + 1, 64))[0] - 1      # the last position is alone in the last block
    _within_cap(sum(p for p, _ in shapes), X.verify_need(cus))
