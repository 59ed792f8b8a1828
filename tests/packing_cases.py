"""Topics at the exact limit where a greedy form's bins stop packing.  Not a test module: test_packing_cases_cpu.py (the
conditions that keep the GPU test honest, on the oracle's totals) and test_packing_limit_gpu.py (every form against the
literal oracle) import it by name, so both run the same cases.

The rule, in words: a consumer's running total and its index share one 64-bit word, (total << idx_bits) | index, when no lag
is negative and S = lag_bits + round_bits + idx_bits <= 62, where lag_bits is the bit length of the largest lag, round_bits
the bit length of the number of rounds ceil(P / C) (a consumer takes one partition per round, so its total stays below
2^(lag_bits + round_bits)), and idx_bits = log2 of the PADDED bin count: C rounded up to a power of two in the block path,
the same with a floor of 64 in the large path.  la_block.hip writes that rule out three times and la_large.hip (rounds_io)
once; SHAPES names, for every greedy form behind one of the four, the smallest topics that reach it."""
from collections import namedtuple

import numpy as np

LIMIT = 62                      # the largest S that packs
BRIM_SPAN = 4096                # "brim" lags lie in [2^lag_bits - BRIM_SPAN, 2^lag_bits - 1]
MIN_LAG_BITS = 13               # so that BRIM_SPAN distinct values exist
PC_MAX = 30_000_000             # per case: the literal oracle's P x C steps stay well below a second


def pow2ceil(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def block_bins(C):
    return pow2ceil(C)


def large_bins(C):
    return max(64, pow2ceil(C))


def decision(P, C, bins):
    """(round_bits, idx_bits) of a topic of P partitions and C consumers whose bins are padded to `bins`."""
    assert bins >= C and bins & (bins - 1) == 0, (C, bins)
    rounds = -(-P // C)
    return rounds.bit_length(), bins.bit_length() - 1


# ---- the case table: (form label, P, C, padded bins, environment) ----------------------------------------------------------
# environment: "" or the value of LA_BLOCK_KEY32 (read once per process: such cases run in a fresh child process).
# Block path (block_class / block_launch): a topic of up to 512 partitions and 256 consumers runs on ONE wavefront (64 threads),
# up to 2 048 x 256 on 256 threads, up to 4 096 x 1 024 on 512, everything else on 1 024.  65 .. 256 consumers: the 32-bit-key
# form for 128 bins (256 too with LA_BLOCK_KEY32=2); otherwise one bin per lane on 2 / 4 wavefronts where the workgroup has
# that many threads, else 2 / 4 bins per lane on one wavefront.  More than 256 consumers: one bin per thread where the
# workgroup has a thread per bin, else two.
KEY32_2 = "block key32<2>"
KEY32_4 = "block key32<4>"
MULTI_2W = "block multi_wave<1> 2 wavefronts"
MULTI_4W = "block multi_wave<1> 4 wavefronts"
ONE_WAVE_2 = "block one_wave_packed<2,64>"
ONE_WAVE_4 = "block one_wave_packed<4,64>"
MULTI_1 = "block multi_wave<1> 512+ bins"
MULTI_2 = "block multi_wave<2>"
ROUNDS_1_64 = "large rounds_packed<1> 64 bins"
ROUNDS_1 = "large rounds_packed<1> 1024 bins"
ROUNDS_2 = "large rounds_packed<2>"
ROUNDS_4 = "large rounds_packed<4>"
ROUNDS_8 = "large rounds_packed<8>"

_BLOCK = [
    # 65 .. 128 consumers, default: greedy_one_wave_key32<2> (17 rounds; 17 rounds with every bin live; one wavefront; one partial round)
    (KEY32_2, 1100, 65, ""), (KEY32_2, 2049, 128, ""), (KEY32_2, 300, 70, ""), (KEY32_2, 127, 128, ""),
    (KEY32_2, 1500, 70, ""),                                            # 22 rounds, idle bins (see SUMS)
    (KEY32_2, 1039, 65, ""), (KEY32_2, 1040, 65, ""), (KEY32_2, 1041, 65, ""),      # P = 16 C - 1, 16 C (every bin takes exactly 16 lags), 16 C + 1
    # ... LA_BLOCK_KEY32=0: one bin per lane on two wavefronts (256+ threads) / two bins per lane on one (64 threads)
    (MULTI_2W, 1100, 65, "0"), (MULTI_2W, 2049, 128, "0"), (MULTI_2W, 1900, 128, "0"), (MULTI_2W, 1500, 70, "0"),
    (ONE_WAVE_2, 300, 70, "0"), (ONE_WAVE_2, 127, 128, "0"), (ONE_WAVE_2, 512, 65, "0"), (ONE_WAVE_2, 450, 70, "0"),
    # 129 .. 256 consumers, default: one bin per lane on four wavefronts (32, 41, 64 = 2^6 and 63 = 2^6 - 1 rounds)
    (MULTI_4W, 4097, 129, ""), (MULTI_4W, 8193, 200, ""), (MULTI_4W, 16384, 256, ""), (MULTI_4W, 16128, 256, ""),
    (MULTI_4W, 4127, 129, ""), (MULTI_4W, 4128, 129, ""), (MULTI_4W, 4129, 129, ""),        # P = 32 C - 1, 32 C, 32 C + 1
    # ... on a 64-thread workgroup: four bins per lane on one wavefront
    (ONE_WAVE_4, 500, 129, ""), (ONE_WAVE_4, 512, 256, ""), (ONE_WAVE_4, 300, 200, ""),
    # ... LA_BLOCK_KEY32=2: greedy_one_wave_key32<4>
    (KEY32_4, 4097, 129, "2"), (KEY32_4, 8193, 200, "2"), (KEY32_4, 16384, 256, "2"), (KEY32_4, 16128, 256, "2"), (KEY32_4, 300, 200, "2"),
    # 257 .. 2 048 consumers, a thread per bin: 512 bins on 512 threads, 1 024 bins on 1 024 (both classes of 1 024 threads)
    (MULTI_1, 1500, 257, ""), (MULTI_1, 4097, 1024, ""), (MULTI_1, 16384, 1024, ""),
    # ... two bins per thread: 2 048 bins on 1 024 threads, 1 024 bins on 512 threads
    (MULTI_2, 8192, 2048, ""), (MULTI_2, 6100, 2047, ""), (MULTI_2, 64, 2048, ""), (MULTI_2, 3000, 1000, ""), (MULTI_2, 6000, 1100, ""),
]
_LARGE = [
    (ROUNDS_1_64, 16385, 3), (ROUNDS_1_64, 20000, 64),                  # 5 462 rounds on 3 of 64 bins; every bin live
    (ROUNDS_1, 16385, 1000), (ROUNDS_1, 17000, 600),
    (ROUNDS_2, 16385, 1025), (ROUNDS_2, 9000, 2048), (ROUNDS_2, 8300, 1300),                   # 16 rounds + 1 partition; 5 rounds, every bin live; 7 rounds
    (ROUNDS_4, 6148, 2049), (ROUNDS_4, 10600, 2100),                    # 3 rounds + 1 partition; 6 rounds
    (ROUNDS_4, 8195, 2049), (ROUNDS_4, 8196, 2049), (ROUNDS_4, 8197, 2049),                    # P = 4 C - 1, 4 C, 4 C + 1
    (ROUNDS_8, 4098, 4097), (ROUNDS_8, 4096, 4097), (ROUNDS_8, 4097, 4097),                     # P = C + 1 (2 rounds), C - 1, C
    (ROUNDS_8, 2000, 8192),                                             # one partial round, every bin's slot live
]
SHAPES = [(f, p, c, block_bins(c), env) for f, p, c, env in _BLOCK] + [(f, p, c, large_bins(c), "") for f, p, c in _LARGE]
FORMS = tuple(dict.fromkeys(s[0] for s in SHAPES))
KEY32_FORMS = (KEY32_2, KEY32_4)
LARGE_FORMS = (ROUNDS_1_64, ROUNDS_1, ROUNDS_2, ROUNDS_4, ROUNDS_8)

# ---- target sums per lag kind ------------------------------------------------------------------------------------------------
# Why 64, 65 and 66: the rule's 62 leaves margin, and a decision that packed S = 63 would still give the oracle's answer, so the
# table goes on to the sums at which a decision that packs too much shows.  Seen on scratch builds whose three block decisions
# behind these forms and rounds_io were relaxed to <= 63, 64, 65 and 66, run on these cases (outputs padded, see below):
#   <= 63  every case still matches, in every form.
#   <= 64  the block forms compare bins through the sign of a 64-bit difference and pad the bins with the sentinel 2^63 - 1
#          (la_sort64.h): a bin of 2^63 or more sorts behind an idle bin's sentinel, the idle bin takes a lag, and members and
#          totals differ (a total is even written at an index past C).  It takes idle bins (C < bins) AND a total whose top bit
#          is set before the last round's sort, rounds - 1 > 2^(round_bits - 1): "brim" at S = 64 failed on 1500x70 (key32<2>,
#          multi_wave<1> on 2 wavefronts), 450x70 (one_wave_packed<2,64>), 8193x200 (multi_wave<1> on 4, key32<4>), 1500x257
#          (multi_wave<1> 512+ bins) and 6000x1100 (multi_wave<2>).  Without idle bins nothing can show at 64: the bins of a round
#          lie within one lag of each other, and the sign of a difference stays right after both have wrapped -- "spread" and
#          "cliff" at 64 (one shape per form, below) are there for the forms the sum falls back to, not to catch this.  129 .. 256
#          consumers on one wavefront run at most 4 rounds, so one_wave_packed<4,64> has no such shape: its 500x129 meets the
#          sentinel a sum later, at 65.  The large path pads with all-ones totals and compares unsigned: exact to the last bit of
#          the word, every case still matches at <= 64.
#   <= 65  (total << idx_bits) loses the top bit of a total of 2^(lag_bits + round_bits - 1) or more, which "brim" reaches where
#          the number of rounds is no power of two: "brim" at S = 65 failed in every form but rounds_packed<8> (totals; members too
#          where the order changed), e.g. 500x129 (one_wave_packed<4,64>), 16385x3, 17000x600, 8300x1300, 8197x2049.
#   <= 66  more than 4 096 consumers stay at 1 or 2 rounds under PC_MAX, both powers of two, so rounds_packed<8> first differs
#          at S = 66 (4098x4097, the bin that takes two lags), as do the other shapes of 2^k rounds.
# A relaxed block form writes that one total past the topic's C consumers: such a build runs with output arrays padded by a
# bin count, never through the tests as they are.
KINDS = ("brim", "spread", "cliff", "one negative", "one zero")
SUMS = {"brim": (61, 62, 63, 64, 65, 66), "spread": (62, 63), "cliff": (62, 63), "one negative": (62,), "one zero": (62, 63)}

Case = namedtuple("Case", "form P C bins env S kind")


def lag_bits_of(case):
    rb, ib = decision(case.P, case.C, case.bins)
    return case.S - rb - ib


def _expand():
    out = []
    for form, P, C, bins, env in SHAPES:
        assert P * C <= PC_MAX, (form, P, C)
        rb, ib = decision(P, C, bins)
        for kind in KINDS:
            for S in SUMS[kind]:
                out.append(Case(form, P, C, bins, env, S, kind))
        if form in KEY32_FORMS:
            # drop = lag_bits - (31 - idx_bits) of 0 and of 1: the key keeps every bit of a total / loses exactly one
            for lb in (31 - ib, 32 - ib):
                for kind in ("brim", "cliff"):
                    out.append(Case(form, P, C, bins, env, lb + rb + ib, kind))
        if form == ROUNDS_8:
            # the narrow form's own border (32-bit lags in, 16-bit indices out) with the lags at the brim
            for lb in (32, 33):
                out.append(Case(form, P, C, bins, env, lb + rb + ib, "brim"))
    # S = 64 with the other two distributions too, on one shape per form: the one without idle bins that runs the most rounds
    # (no "brim" case at 64 can tell there: see above), else the form's first shape
    for form in FORMS:
        mine = [s for s in SHAPES if s[0] == form]
        full = [s for s in mine if s[2] == s[3]]
        _, P, C, bins, env = max(full, key=lambda s: -(-s[1] // s[2])) if full else mine[0]
        for kind in ("spread", "cliff"):
            out.append(Case(form, P, C, bins, env, 64, kind))
    for c in out:                                                       # a shape that cannot carry a generator is not listed
        assert MIN_LAG_BITS <= lag_bits_of(c) <= 62, c
    return out


CASES = _expand()


def case_id(c):
    return ("%s-%dx%d-S%d-%s" % (c.form, c.P, c.C, c.S, c.kind)).replace(" ", "_")


def seed_of(c):
    return (c.P * 1_000_003 + c.C * 101 + c.S) * 7 + KINDS.index(c.kind)


# ---- lag generators: (P, C, bins, S, seed) -> int64 [P], the largest lag exactly 2^lag_bits - 1 -----------------------------
def _lag_bits(P, C, bins, S):
    rb, ib = decision(P, C, bins)
    lb = S - rb - ib
    assert MIN_LAG_BITS <= lb <= 62, (P, C, bins, S, lb)
    return lb


def brim(P, C, bins, S, seed):
    """Every lag within BRIM_SPAN of the top, distinct where P allows: a consumer's total after q rounds exceeds
    q (2^lag_bits - 4096), so the total field fills to its last usable bit, and the order of the bins is not trivial."""
    lb = _lag_bits(P, C, bins, S)
    rng = np.random.default_rng(seed)
    if P <= BRIM_SPAN:
        off = rng.choice(BRIM_SPAN, P, replace=False)
    else:
        off = rng.permutation(np.concatenate([np.arange(BRIM_SPAN), rng.integers(0, BRIM_SPAN, P - BRIM_SPAN)]))
    if not (off == 0).any():
        off[rng.integers(0, P)] = 0
    return (np.int64((1 << lb) - 1) - off).astype(np.int64)


def spread(P, C, bins, S, seed):
    """One lag of 2^lag_bits - 1, the rest uniform below it (and above zero)."""
    lb = _lag_bits(P, C, bins, S)
    rng = np.random.default_rng(seed)
    lag = rng.integers(1, (1 << lb) - 1, P).astype(np.int64)
    lag[rng.integers(0, P)] = (1 << lb) - 1
    return lag


def cliff(P, C, bins, S, seed):
    """The first round's lags are 2^lag_bits - 1 - i, all others lie below 2^(lag_bits / 2): first lag - last lag uses every
    one of lag_bits bits, and the rounds after the first differ in low bits only."""
    lb = _lag_bits(P, C, bins, S)
    rng = np.random.default_rng(seed)
    n = min(C, P)
    lag = np.concatenate([np.int64((1 << lb) - 1) - np.arange(n, dtype=np.int64), rng.integers(1, 1 << (lb // 2), P - n).astype(np.int64)])
    return rng.permutation(lag)


def _brim_with_one(value, P, C, bins, S, seed):
    lag = brim(P, C, bins, S, seed)
    rng = np.random.default_rng(seed + 1)
    j = int(rng.integers(0, P))
    if lag[j] == lag.max():                                             # the top lag stays: lag_bits is what S says
        j = (j + 1) % P
    lag[j] = value
    return lag


def one_negative(P, C, bins, S, seed):
    """ "brim" with a single lag of -1: the smallest lag alone rules packing out, and that consumer's total takes a step down."""
    return _brim_with_one(-1, P, C, bins, S, seed)


def one_zero(P, C, bins, S, seed):
    """ "brim" with a single lag of 0: the smallest lag arms the zero-tail shortcuts of both paths, with one zero only."""
    return _brim_with_one(0, P, C, bins, S, seed)


GENERATORS = {"brim": brim, "spread": spread, "cliff": cliff, "one negative": one_negative, "one zero": one_zero}


def lags_of(c):
    lag = GENERATORS[c.kind](c.P, c.C, c.bins, c.S, seed_of(c))
    assert lag.dtype == np.int64 and lag.size == c.P and int(lag.max()) == (1 << lag_bits_of(c)) - 1
    return lag
