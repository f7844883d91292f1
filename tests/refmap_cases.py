"""Constructed inputs of the reference mapper (SPEC.md §18): hand-made
reference sets and reads at the smallest shapes where the seed, the band or the
path can go wrong.  CASES = [(name, set index, read, expect)], SETS = [targets];
expect holds what the case was built to reach, as values of the reference's
record (field name -> value, or -> a predicate on the whole record as a dict),
which tests/test_refmap_host.py asserts on refmap_ref, so a case that no longer
reaches its situation fails there.  Shared by the host and the GPU tests;
reference() computes refmap_ref once per case and keeps it.  REJECTED = sets
that are none.
"""
from __future__ import annotations

import random

from . import refmap_ref as R

rc = R.revcomp


def rnd(seed: int, n: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other(ch: int, by: int = 1) -> int:
    return b"ACGT"[(b"ACGT".index(ch) + by) % 4]


def subs(s: bytes, every: int, first: int = 6) -> bytes:
    """s with a substitution at first, first + every, ..."""
    b = bytearray(s)
    for k in range(first, len(b), every):
        b[k] = other(b[k])
    return bytes(b)


T0, T1, T2 = rnd(1, 1500), rnd(2, 1500), rnd(3, 900)
T13 = rnd(4, 13)
U, V = rnd(5, 20), rnd(6, 20)
_X = T0[300:400]
PAL = _X + rc(_X)                      # its own reverse complement (200)
TP = rnd(7, 150) + PAL + rnd(8, 150)
T0N = T0[:500] + b"N" + T0[501:520] + b"n" + T0[521:]
LONG = rnd(9, 20600)

SETS = [
    [T0, T1, T2],               # 0: the general set
    [T13, T1],                  # 1: a target of exactly 13 bases
    [T0, T0],                   # 2: two identical targets
    [TP, TP],                   # 3: ... that hold a palindrome
    [U * 64],                   # 4: the k-mers at offsets 0..7 of the unit occur 64 times: kept
    [U * 65],                   # 5: ... 65 times: dropped (offsets 8..19: 64 times, kept)
    [V * 40 + rnd(10, 30), rnd(11, 30) + V * 40],  # 6: 40 occurrences in each of two targets
    [T0N, T1.lower()],          # 7: N and n in a target; a lower-case target
    [T0, subs(T0, 50)],         # 8: a near copy
    [LONG],                     # 9
]


def _long_read() -> bytes:
    """LONG[100:20100] with a substitution every 97 bases, a deleted base every
    1000 and an inserted one every 1000, 500 apart."""
    b = bytearray()
    for k, ch in enumerate(LONG[100:20100]):
        if k % 1000 == 250:
            continue
        b.append(other(ch) if k % 97 == 13 else ch)
        if k % 1000 == 750:
            b.append(other(ch, 2))
    return bytes(b)


def cases():
    out = []

    def add(name, si, read, **expect):
        out.append((name, si, bytes(read), expect))

    mapped = lambda r: r["g"] >= 0    # noqa: E731
    # --- seed
    add("n0", 0, b"", g=-1)
    add("n12", 0, T0[100:112], g=-1)
    add("n13", 0, T0[100:113], g=0, o=0, votes=1, d0=112, mat=13)
    add("target_13", 1, rnd(12, 10) + T13 + rnd(13, 17), g=0, votes=1, qb=10, qe=23, tb=0, te=13)
    add("diag_m1", 0, rnd(14, 1) + T0[0:100], g=0, d0=-16)
    add("diag_m32", 0, rnd(15, 32) + T0[0:100], g=0, d0=-16)
    add("diag_m33", 0, rnd(16, 33) + T0[0:100], g=0, d0=-48)
    add("diag_31", 0, T0[31:131], g=0, d0=16)
    add("diag_32", 0, T0[32:132], g=0, d0=48)
    # 18 k-mers at diagonal 100 (bin 3) and 18 at 140 (bin 4): the smaller bin
    add("two_bins_tie", 0, T0[100:130] + T0[170:200], g=0, d0=112, votes=18)
    add("identical_targets", 2, T0[200:600], g=0, o=0, check=lambda r: r["votes2"] == r["votes"] == 388)
    add("palindrome", 3, PAL, g=0, o=0, check=lambda r: r["votes2"] == r["votes"])
    add("occ_64", 4, U * 3, check=lambda r: mapped(r) and r["votes"] > 0)
    add("occ_65", 5, U * 3, check=mapped)
    add("occ_40_two_targets", 6, V * 3, check=lambda r: mapped(r) and r["votes2"] > 0)
    add("target_N", 7, T0[400:700], g=0, o=0, mis=2, mat=298)
    add("lower_case_target", 7, T1[100:400].lower(), g=1, mat=300)
    add("revcomp_read", 0, rc(T0[300:700]), g=0, o=1, tb=300, te=700, mat=400)
    add("revcomp_read_other_target", 0, rc(T2[100:500]), g=2, o=1, tb=100, te=500)
    add("near_copy", 8, T0[100:500], g=0, check=lambda r: 0 < r["votes2"] < r["votes"])
    add("no_hit", 0, rnd(17, 300), g=-1)
    # --- band and path
    add("exact", 0, T1[100:600], g=1, o=0, qb=0, qe=500, tb=100, te=600, mat=500, aln=500)
    add("substitutions", 0, subs(T1[100:600], 40), g=1, mis=13, mat=487)
    add("insertions", 0, T1[100:300] + b"A" + T1[300:450] + b"C" + T1[450:600], g=1, check=lambda r: r["ins"] + r["mis"] >= 1 and r["aln"] >= 500)
    add("deletions", 0, T1[100:300] + T1[301:450] + T1[451:600], g=1, check=lambda r: r["del"] >= 1 and r["te"] == 600)
    # (one side of the indel is aligned, the other clipped: 256 gaps cost more than 400 matches gain)
    add("deletion_300", 0, T0[0:400] + T0[700:1100], g=0, check=lambda r: 400 <= r["aln"] <= 410 and r["del"] == 0)
    add("insertion_300", 0, T0[0:400] + rnd(18, 300) + T0[400:800], g=0, check=lambda r: 400 <= r["aln"] <= 410 and r["ins"] == 0)
    # the votes come from 100 exact bases at diagonal 368; the best alignment
    # is 300 bases with a substitution every 12 (no 13-mer left) at the band's edge
    add("band_first_cells", 0, subs(T0[112:412], 12) + T0[668:768], g=0, d0=368,
        check=lambda r: r["tb"] - r["qb"] == 368 - 256 and r["aln"] > 250)
    add("band_last_cells", 0, subs(T0[624:924], 12) + T0[668:768], g=0, d0=368,
        check=lambda r: r["tb"] - r["qb"] == 368 + 256 and r["aln"] > 250)
    add("junk_ends", 0, rnd(19, 50) + T0[200:600] + rnd(20, 70), g=0, check=lambda r: 45 <= r["qb"] <= 50 and 450 <= r["qe"] <= 455)
    add("over_right_end", 0, T0[1400:1500] + rnd(21, 100), g=0, te=1500)
    add("over_left_end", 0, rnd(22, 100) + T0[0:100], g=0, tb=0)
    for n in (31, 32, 33, 63, 64, 65, 127, 128, 129):
        add(f"n_{n}", 0, T2[500:500 + n], g=2, qb=0, qe=n, mat=n)
    add("long_20000", 9, _long_read(), g=0, o=0, check=lambda r: r["qe"] - r["qb"] > 19900)
    return out


CASES = cases()
NAMES = [c[0] for c in CASES]
_REF: dict = {}


def reference(i: int):
    """(record, words) of case i by refmap_ref, computed once."""
    if i not in _REF:
        _, si, read, _ = CASES[i]
        _REF[i] = R.record(SETS[si], read)
    return _REF[i]


def check_expect(rec, expect) -> None:
    from ccsx_amd import REF_FIELDS
    r = dict(zip(REF_FIELDS, rec))
    for k, v in expect.items():
        if k == "check":
            assert v(r), r
        else:
            assert r[k] == v, (k, v, r)


REJECTED = {
    "empty": [],
    "65_targets": [rnd(400 + k, 13) for k in range(65)],
    "a_target_of_12": [T0, rnd(30, 12)],
    "letters_over_2_20": [b"A" * ((1 << 19) + 1)] * 2,
    "digit": [T0[:50] + b"1" + T0[51:100]],
    "dash": [T0[:50] + b"-" + T0[51:100]],
    "space": [T0[:50] + b" " + T0[51:100]],
}


def accuracy_case(seed: int):
    """SPEC.md §18's end-to-end case: three random 600-base targets; 12 ZMWs
    whose template is a 400-base stretch of one of them in either strand, each
    with 8 subreads at 2 / 4 / 4 % errors (scan_cases.accuracy_case's rates),
    the odd ones reverse-complemented.  Returns (targets, [(g, strand, start)],
    [subreads])."""
    from .polish_ref import mutate
    rng = random.Random(seed)
    targets = [bytes(rng.choice(b"ACGT") for _ in range(600)) for _ in range(3)]
    planted, zmws = [], []
    for _ in range(12):
        g, o, b = rng.randrange(3), rng.randrange(2), rng.randrange(201)
        t = targets[g][b:b + 400]
        if o:
            t = rc(t)
        ss = [mutate(rng, t, .02, .04, .04) for _ in range(8)]
        planted.append((g, o, b))
        zmws.append([s if k % 2 == 0 else rc(s) for k, s in enumerate(ss)])
    return targets, planted, zmws


ACCURACY_SEED = 0  # the first seed tried: the reference meets §18's condition on it (test_refmap_host.py checks that)
