"""The case table of packing_cases.py holds what it was built to hold (no GPU): test_packing_limit_gpu.py compares every greedy
form with the literal oracle on exactly these cases, and the conditions here are what keeps that comparison from passing for
the wrong reason -- checked on the oracle's totals, never asserted from the formulas."""
import numpy as np
import pytest

import packing_cases as pc
from oracle import oracle
from oracle.round_form import round_form

# Sum of P x C over the expanded table: the literal oracle walks C bins per partition (about 1.5 ns a step), and both this file
# and the GPU file run it once per case.  Under this cap each of them spends about seven seconds in the oracle; the large path's
# shapes (more than 8 192 partitions on more than 1 024 consumers: 17 M steps a case) make up most of it.
TABLE_PC_CAP = 4_500_000_000


def _topic(c):
    """(part_off, ids, lags, cons_off, ranks) of a case; ids in order, so the result is a function of the lags alone."""
    return (np.array([0, c.P], np.int64), np.arange(c.P, dtype=np.int32), pc.lags_of(c), np.array([0, c.C], np.int64),
            np.arange(c.C, dtype=np.int32))


@pytest.fixture(scope="module")
def totals():
    """case -> the literal oracle's totals (read-only); the round form has to agree on order, member and totals on the way."""
    out = {}
    for c in pc.CASES:
        t = _topic(c)
        lit = oracle.assign_flat(*t)
        for g, e, what in zip(round_form(*t), lit, ("partition order", "member", "totals")):
            np.testing.assert_array_equal(g, e, err_msg="round form vs literal, %s: %s" % (what, pc.case_id(c)))
        out[c] = lit[2]
    return out


def test_decision_in_words():
    assert pc.decision(16385, 3, 64) == (13, 6)                         # 5 462 rounds; three consumers still index 64 bins
    assert pc.decision(127, 128, 128) == (1, 7)                         # one partial round
    assert pc.decision(4127, 129, 256) == (6, 8) and pc.decision(4096, 129, 256) == (6, 8) and pc.decision(3999, 129, 256) == (5, 8)
    assert pc.block_bins(65) == 128 and pc.block_bins(128) == 128 and pc.block_bins(2047) == 2048
    assert pc.large_bins(3) == 64 and pc.large_bins(1025) == 2048 and pc.large_bins(8192) == 8192


def form_in_words(P, C, mode):
    """The greedy form that a call of ONE packing topic of P partitions and C consumers reaches, from the dispatch in words
    (la_kernels.h block_fits / block_class, block_launch's workgroup sizes, block_topic_kernel's branches, rounds_class); `mode`
    is LA_BLOCK_KEY32, 1 where it is not set.  A dispatch constant that moves makes a label of the table wrong: this says so."""
    if not ((P <= 8192 and C <= 2048) or (P <= 16384 and C <= 1024)):   # too big for one workgroup's LDS: the large path
        bins = pc.large_bins(C)                                         # 1 024 threads at most, so 1, 2, 4, 8 bins each
        assert bins <= 8192
        return {64: pc.ROUNDS_1_64, 1024: pc.ROUNDS_1, 2048: pc.ROUNDS_2, 4096: pc.ROUNDS_4, 8192: pc.ROUNDS_8}[bins]
    assert C > 64, "up to 64 consumers: the tile and the one-wavefront rounds, whose limit tests are in test_gpu_parity.py"
    threads = 64 if P <= 512 and C <= 256 else 256 if P <= 2048 and C <= 256 else 512 if P <= 4096 and C <= 1024 else 1024
    bins = pc.block_bins(C)
    if bins > 256:
        return pc.MULTI_1 if bins <= threads else pc.MULTI_2
    if bins == 128:
        # (one bin per lane on two wavefronts only in launches of up to 512 topics: these are launches of one)
        return pc.KEY32_2 if mode >= 1 else pc.MULTI_2W if bins <= threads else pc.ONE_WAVE_2
    return pc.KEY32_4 if mode >= 2 else pc.MULTI_4W if bins <= threads else pc.ONE_WAVE_4


def test_every_label_names_the_form_its_shape_reaches():
    for form, P, C, bins, env in pc.SHAPES:
        assert form_in_words(P, C, int(env or 1)) == form, (form, P, C, env)
        assert bins == (pc.large_bins(C) if form in pc.LARGE_FORMS else pc.block_bins(C))
    # the class arithmetic behind three of the labels, spelled out
    assert all(P <= 512 for f, P, C, _, _ in pc.SHAPES if f in (pc.ONE_WAVE_2, pc.ONE_WAVE_4))        # the 64-thread class
    assert all(bins > (512 if P <= 4096 and C <= 1024 else 1024) for f, P, C, bins, _ in pc.SHAPES if f == pc.MULTI_2)   # n_c > nt
    assert all((P > 8192 or C > 2048) and (P > 16384 or C > 1024) for f, P, C, _, _ in pc.SHAPES if f in pc.LARGE_FORMS)


def test_every_form_has_both_sides_of_the_limit_at_the_brim():
    for form in pc.FORMS:
        for S in (61, 62, 63):
            assert any(c.form == form and c.S == S and c.kind == "brim" for c in pc.CASES), (form, S)
        for S in (65, 66):
            assert any(c.form == form and c.S == S and c.kind == "brim" for c in pc.CASES), (form, S)
        # block path: S = 64 on a shape with idle bins whose totals have their top bit set before the last round's sort -- where
        # the form's shapes allow one (packing_cases.SUMS): the first sum at which a decision that packs too much shows
        if form not in pc.LARGE_FORMS and form != pc.ONE_WAVE_4:
            assert any(c.form == form and c.S == 64 and c.kind == "brim" and c.C < c.bins and
                       -(-c.P // c.C) - 1 > 1 << (pc.decision(c.P, c.C, c.bins)[0] - 1) for c in pc.CASES), form
        for kind in pc.KINDS:
            assert any(c.form == form and c.kind == kind for c in pc.CASES), (form, kind)
        for kind in ("spread", "cliff"):
            assert any(c.form == form and c.kind == kind and c.S == 64 for c in pc.CASES), (form, kind)
    assert len(set(pc.CASES)) == len(pc.CASES)
    for form in pc.KEY32_FORMS:                                         # drop == 0 and drop == 1 with the lags at the edge
        ib = {pc.KEY32_2: 7, pc.KEY32_4: 8}[form]
        for lb in (31 - ib, 32 - ib):
            for kind in ("brim", "cliff"):
                assert any(c.form == form and c.kind == kind and pc.lag_bits_of(c) == lb for c in pc.CASES), (form, lb, kind)


def test_generators_hold_what_they_promise():
    for c in pc.CASES:
        lag = pc.lags_of(c)
        lb = pc.lag_bits_of(c)
        top = (1 << lb) - 1
        assert int(lag.max()) == top, pc.case_id(c)
        if c.kind == "brim":
            assert int(lag.min()) >= top - (pc.BRIM_SPAN - 1)
            assert np.unique(lag).size == min(c.P, pc.BRIM_SPAN), pc.case_id(c)
        elif c.kind == "spread":
            assert int(lag.min()) > 0
        elif c.kind == "cliff":
            s = np.sort(lag)[::-1]
            n = min(c.P, c.C)
            np.testing.assert_array_equal(s[:n], top - np.arange(n))
            assert int(s[0] - s[-1]).bit_length() == lb or c.P <= c.C, pc.case_id(c)
            assert c.P <= c.C or (int(s[n]) < 1 << (lb // 2) and int(s[-1]) > 0)
        elif c.kind == "one negative":
            assert c.S == pc.LIMIT and int((lag < 0).sum()) == 1 and int(lag.min()) == -1
        else:
            assert int((lag == 0).sum()) == 1 and int(lag.min()) == 0


def test_brim_totals_fill_the_field(totals):
    for c in pc.CASES:
        if c.kind != "brim":
            continue
        rb, _ = pc.decision(c.P, c.C, c.bins)
        lb = pc.lag_bits_of(c)
        rounds = -(-c.P // c.C)
        biggest = int(totals[c].max())
        assert biggest >= (rounds - 1) * ((1 << lb) - pc.BRIM_SPAN), pc.case_id(c)
        if rounds & (rounds - 1):
            assert biggest >= 1 << (lb + rb - 1), pc.case_id(c)          # the field's top bit is set


def test_every_form_reaches_a_sum_that_cannot_pack(totals):
    """Some "brim" case of every form has a total that (total << idx_bits) cannot hold, on the oracle's totals -- at S = 65 where
    the form has a shape whose rounds are no power of two, else at S = 66 (at most 4 rounds on a 64-thread workgroup with 129+
    consumers, at most 2 with 4 097+ consumers under PC_MAX): a decision that packed it would show in the totals."""
    for form in pc.FORMS:
        first = min((c.S for c in pc.CASES if c.form == form and c.kind == "brim" and
                     int(totals[c].max()) >= 1 << (64 - pc.decision(c.P, c.C, c.bins)[1])), default=None)
        assert first == (66 if form in (pc.ONE_WAVE_4, pc.ROUNDS_8) else 65), (form, first)


def test_packed_sums_really_fit(totals):
    """S <= 62 and no negative lag: no total reaches 2^(64 - idx_bits) (nor 2^(62 - idx_bits), which is what the rule promises),
    so the packed word is exact there and a mismatch on the GPU is the kernel's."""
    for c in pc.CASES:
        if c.S > pc.LIMIT:
            continue
        _, ib = pc.decision(c.P, c.C, c.bins)
        t = totals[c]
        if c.kind == "one negative":
            continue                                                     # does not pack: the smallest lag rules it out
        assert int(t.min()) >= 0 and int(t.max()) < 1 << (62 - ib), pc.case_id(c)
        assert int(t.max()) < 1 << (64 - ib)


def test_the_table_stays_cheap():
    total = sum(c.P * c.C for c in pc.CASES)
    assert total <= TABLE_PC_CAP, total
    assert all(c.P * c.C <= pc.PC_MAX for c in pc.CASES)
