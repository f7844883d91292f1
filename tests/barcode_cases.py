"""Constructed inputs of the demultiplexer (SPEC.md §16): hand-made barcode sets
and reads at the smallest shapes where the kernel can go wrong.  CASES =
[(name, set index, ccs, expect)], SETS = [(barcodes, window)]; expect holds
what the case was built to reach, as fields of the reference's result
(tests/test_barcode_host.py asserts them on barcode_ref, so a case that no
longer reaches its situation fails there): e0 / e1 = the leading values of that
end's (pattern, score, end, second, second_pattern), check = a predicate on the
whole result.  Shared by the host and the GPU tests; reference() computes
barcode_ref once per case.  REJECTED = sets that are none; CALLS = inputs of
ccsx_barcode_call at its thresholds' edges.
"""
from __future__ import annotations

import random

from . import barcode_ref as R

NONE = R.NONE
rc = R.revcomp


def rnd(seed: int, n: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


BC = [rnd(1000 + i, 16) for i in range(8)]
PAL = b"ACGTACGTACGTACGT"          # its own reverse complement
NEARPAL = b"ACGTACGTACGTACGA"      # one base off its reverse complement
BIG = [rnd(2000 + i, 16) for i in range(96)]
BIG_TIE = BIG[:70] + [BIG[3]] + BIG[71:]   # barcode 70 = barcode 3: patterns 6 (chunk 0) and 140 (chunk 2)
MIXED = [b"g", rnd(31, 8), rnd(32, 16).lower(), rnd(33, 25), rnd(34, 64), rnd(35, 40).lower()]

SETS = [
    (BC, 96),                              # 0
    (BC, 40),                              # 1
    (BC, 1),                               # 2
    (BC, 256),                             # 3
    ([BC[0], PAL, BC[1]], 96),             # 4
    ([BC[0], BC[2], BC[1], BC[2]], 96),    # 5: two identical barcodes
    ([BC[0], NEARPAL, BC[1]], 96),         # 6
    ([BC[0], BC[2], BC[1], BC[1]], 96),    # 7
    ([BC[2]], 96),                         # 8: B = 1
    (BIG[:32], 96),                        # 9: exactly one chunk
    (BIG[:33], 96),                        # 10: two patterns in a second chunk
    (BIG, 96),                             # 11: three full chunks
    (BIG_TIE, 96),                         # 12
    (MIXED, 96),                           # 13: 64 rows, lengths mixed in one wave
    ([MIXED[3], BC[0]], 96),               # 14: 32 rows
    ([MIXED[5], BC[0], MIXED[1]], 96),     # 15: 48 rows
    (BIG[:33], 50),                        # 16
]


def cases():
    out = []

    def add(name, si, ccs, **expect):
        out.append((name, si, bytes(ccs), expect))

    f = lambda k, n: rnd(5000 + k, n)  # noqa: E731  (filler)
    b2, b5 = BC[2], BC[5]
    # where the copy lies
    add("copy_at_0", 0, b2 + f(1, 300) + rc(b5), e0=(4, 16, 16), e1=(10, 16, 16))
    add("copy_at_7", 0, f(2, 7) + b2 + f(3, 300) + rc(b5) + f(4, 11), e0=(4, 16, 23), e1=(10, 16, 27))
    add("ends_at_w", 1, f(5, 24) + b2 + f(6, 300), e0=(4, 16, 40))
    add("beyond_window", 1, f(7, 41) + b2 + f(8, 300), check=lambda r: r[0][1] < 10)
    # read lengths
    add("n0", 0, b"", e0=(0, -32, 0, -32, 2), e1=(0, -32, 0, -32, 2))
    add("n1", 0, b"A", check=lambda r: r[0][1] == -29 and r[0][2] == 1 and r[1][1] == -29)
    add("n_lt_L", 0, b2[:10], e0=(4, -2, 10))
    # (each window holds the whole read: the far end's barcode ties, and the smaller p wins)
    add("n_lt_wn", 0, b2 + f(9, 30) + rc(b5), e0=(4, 16, 16, 16, 11), e1=(5, 16, 62, 16, 10))
    add("overlapping_windows", 0, b2 + f(10, 118) + rc(b5), e0=(4, 16, 16), e1=(10, 16, 16))
    add("wn1", 2, b2 + f(11, 100), check=lambda r: r[0][1] == -29 and r[0][2] == 1)
    add("wn256", 3, f(12, 200) + b2 + f(13, 500), e0=(4, 16, 216))
    # one error of each kind: L - 3, L - 2, L - 3
    sub = b2[:8] + bytes([b"ACGT"[(b"ACGT".index(b2[8]) + 1) % 4]]) + b2[9:]
    add("one_substitution", 0, f(14, 5) + sub + f(15, 300), e0=(4, 13, 21))
    add("one_inserted_base", 0, f(16, 5) + b2[:8] + bytes([b"ACGT"[(b"ACGT".index(b2[8]) + 2) % 4]]) + b2[8:] + f(17, 300),
        e0=(4, 14, 22))
    add("one_deleted_base", 0, f(18, 5) + b2[:8] + b2[9:] + f(19, 300), e0=(4, 13, 20))
    # column 0's -2 i on the best path
    add("starts_mid_barcode", 0, b2[2:] + f(20, 300), e0=(4, 10, 14))
    # orientations, palindromes, duplicates
    add("o1_at_end0", 0, rc(BC[3]) + f(21, 300) + BC[6], e0=(7, 16, 16), e1=(13, 16, 16))
    add("palindrome", 4, f(22, 2) + PAL + f(23, 300), e0=(2, 16, 18))
    add("identical_barcodes", 5, b2 + f(24, 300), e0=(2, 16, 16, 16, 6))
    add("twice_in_window", 0, f(25, 3) + b2 + f(26, 10) + b2 + f(27, 300), e0=(4, 16, 19))
    add("second_skips_other_orientation", 6, NEARPAL + f(28, 300),
        check=lambda r: r[0][:3] == (2, 16, 16) and r[0][4] >> 1 != 1 and r[0][3] < 10
        and R.align(R.patterns([NEARPAL])[1], R.ends(NEARPAL + f(28, 300), 96)[0])[0] > r[0][3])
    add("second_pattern_tie", 7, b2 + f(29, 4) + BC[1] + f(30, 300), e0=(2, 16, 16, 16, 4))
    add("one_barcode", 8, b2 + f(31, 300) + rc(b2), e0=(0, 16, 16, NONE, -1), e1=(0, 16, 16, NONE, -1))
    # chunks
    add("b32_last", 9, rc(BIG[31]) + f(32, 300), e0=(63, 16, 16))
    add("b33_second_chunk", 10, BIG[32] + f(33, 300) + BIG[32], e0=(64, 16, 16), e1=(65, 16, 16))
    add("b33_first_chunk", 10, BIG[0] + f(34, 300), e0=(0, 16, 16))
    add("b96_last_lane", 11, rc(BIG[95]) + f(35, 300) + rc(BIG[40]), e0=(191, 16, 16), e1=(80, 16, 16))
    add("b96_chunk0_and_chunk2", 12, BIG[3] + f(36, 300), e0=(6, 16, 16, 16, 140))
    add("b96_second_in_other_chunk", 11, BIG[90] + f(37, 3) + BIG[5] + f(38, 300), e0=(10, 16, 35, 16, 180))
    add("b33_short_window", 16, f(39, 30) + BIG[32] + f(40, 300), e0=(64, 16, 46))
    # lengths 1, 8, 16, 25, 40 and 64 in one set, lower case letters
    add("mixed_64", 13, f(41, 9) + MIXED[4] + f(42, 300) + rc(MIXED[3]).lower(), e0=(8, 64, 73), e1=(6, 25, 25))
    add("mixed_8_and_16", 13, MIXED[1] + f(43, 300) + MIXED[2].upper(), e0=(2, 8, 8), e1=(5, 16, 16))
    add("mixed_40", 13, rc(MIXED[5]) + f(44, 300), e0=(11, 40, 40))
    add("mixed_1", 13, b"A" * 50, e0=(0, -2, 0), e1=(0, -2, 0))
    add("mixed_1_found", 13, b"AAAC" + b"A" * 50, e0=(1, 1, 4))
    add("rows32", 14, f(45, 3) + MIXED[3] + f(46, 300) + rc(BC[0]), e0=(0, 25, 28), e1=(2, 16, 16))
    add("rows48", 15, f(47, 56) +MIXED[5].upper() + f(48, 300) + rc(MIXED[1]), e0=(0, 40, 96), e1=(4, 8, 8))
    add("letters_n", 0, b"NNNN" + b2 + f(49, 300), e0=(4, 16, 20))
    return out


CASES = cases()
NAMES = [c[0] for c in CASES]
_ref: dict = {}


def reference(i: int):
    if i not in _ref:
        _, si, ccs, _ = CASES[i]
        _ref[i] = R.score(SETS[si][0], ccs, SETS[si][1])
    return _ref[i]


def by_set():
    """{set index: [case indices]} in case order."""
    d: dict = {}
    for i, c in enumerate(CASES):
        d.setdefault(c[1], []).append(i)
    return d


REJECTED = {
    "letter_n": [BC[0], b"ACGTNACGT"],
    "length_0": [BC[0], b""],
    "length_65": [rnd(1, 65)],
    "empty_set": [],
    "b_2049": [BC[0]] * 2049,
}

# (name, result, lens, n, T, D, expect = (cl, cr, called, assigned, reason)) for ccsx_barcode_call
_E = lambda p, s, e, s2, p2: (p, s, e, s2, p2)  # noqa: E731
CALLS = [
    # 100 score = T L: 100 x 12 = 75 x 16
    ("score_at_T", (_E(0, 12, 20, 3, 2), _E(2, 16, 16, 3, 0)), [16, 16], 500, 75, 3, (20, 16, (True, True), True, 0)),
    ("score_below_T", (_E(0, 11, 20, 3, 2), _E(2, 16, 16, 3, 0)), [16, 16], 500, 75, 3, (0, 16, (False, True), False, 1)),
    ("lead_at_D", (_E(0, 16, 16, 13, 2), _E(2, 16, 18, 13, 0)), [16, 16], 500, 60, 3, (16, 18, (True, True), True, 0)),
    ("lead_below_D", (_E(0, 16, 16, 13, 2), _E(2, 16, 18, 14, 0)), [16, 16], 500, 60, 3, (16, 0, (True, False), False, 2)),
    ("neither", (_E(0, 5, 16, 4, 2), _E(2, 5, 18, 4, 0)), [16, 16], 500, 60, 3, (0, 0, (False, False), False, 3)),
    ("clips_meet", (_E(0, 16, 16, 3, 2), _E(2, 16, 18, 3, 0)), [16, 16], 34, 60, 3, (16, 18, (True, True), False, 4)),
    ("one_base_left", (_E(0, 16, 16, 3, 2), _E(2, 16, 18, 3, 0)), [16, 16], 35, 60, 3, (16, 18, (True, True), True, 0)),
    ("one_barcode", (_E(1, 16, 16, NONE, -1), _E(0, 16, 16, NONE, -1)), [16], 100, 60, 3, (16, 16, (True, True), True, 0)),
    ("length_of_the_winner", (_E(2, 5, 8, 0, 0), _E(0, 5, 16, 0, 2)), [16, 8], 100, 60, 3, (8, 0, (True, False), False, 2)),
    ("negative_score", (_E(0, -32, 0, -32, 2), _E(0, -32, 0, -32, 2)), [16, 16], 0, 60, 3, (0, 0, (False, False), False, 3)),
]


def accuracy_case(seed: int = 7):
    """SPEC.md §16's end-to-end case: 12 barcodes of 16 bases, pairwise (and
    against every reverse complement, their own included) at edit distance >= 7;
    12 ZMWs of bc[i0] + 600 random bases + rc(bc[i1]), each with 8 subreads at
    2 / 4 / 4 % errors, the odd ones reverse-complemented.  Returns (barcodes,
    [(i0, i1)], [subreads])."""
    from .polish_ref import mutate
    rng = random.Random(seed)
    bcs: list = []
    while len(bcs) < 12:
        c = bytes(rng.choice(b"ACGT") for _ in range(16))
        if R.edit_distance(c, rc(c)) >= 7 and all(R.edit_distance(c, b) >= 7 and R.edit_distance(c, rc(b)) >= 7 for b in bcs):
            bcs.append(c)
    pairs, zmws = [], []
    for _ in range(12):
        i0, i1 = rng.randrange(12), rng.randrange(12)
        t = bcs[i0] + bytes(rng.choice(b"ACGT") for _ in range(600)) + rc(bcs[i1])
        subs = [mutate(rng, t, .02, .04, .04) for _ in range(8)]
        pairs.append((i0, i1))
        zmws.append([s if k % 2 == 0 else rc(s) for k, s in enumerate(subs)])
    return bcs, pairs, zmws
