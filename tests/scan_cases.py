"""Constructed inputs of the adapter scanner (SPEC.md §17): hand-made adapter
sets and reads at the smallest shapes where the kernel can go wrong.  CASES =
[(name, set index, ccs, expect)], SETS = [(adapters, T)]; expect holds what the
case was built to reach, as properties of the reference's hits
(tests/test_scan_host.py asserts them on scan_ref, so a case that no longer
reaches its situation fails there): hits = the hits' (adapter, orient, start,
end) exactly, n_hits = their number, has = hits that must be among them, check
= a predicate on the hit list.  Shared by the host and the GPU tests;
reference() computes scan_ref once per case.  The tile cases are placed by TC /
WU, which mirror ccsx_scan.h (the GPU tests check them against Scanner.tile).
TRACKED = the cases whose bottom rows the GPU test compares cell for cell.
REJECTED = sets that are none; CUTS = inputs of ccsx_scan_cut.
"""
from __future__ import annotations

import random

from . import scan_ref as R

rc = R.revcomp
TC = 512
WU = {16: 40, 32: 80, 48: 120, 64: 160}  # ceil(2.5 rows)


def rnd(seed: int, n: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def put(read: bytes, at: int, what: bytes) -> bytes:
    """read with `what` written over its bases [at, at + len(what))."""
    assert 0 <= at and at + len(what) <= len(read)
    return read[:at] + what + read[at + len(what):]


def other(ch: int) -> int:
    return b"ACGT"[(b"ACGT".index(ch) + 1) % 4]


def sub(s: bytes, k: int) -> bytes:
    return s[:k] + bytes([other(s[k])]) + s[k + 1:]


# one adapter per row class: 16, 32, 48 and 64 rows
AD = {16: rnd(101, 16), 32: rnd(102, 25), 48: rnd(103, 45), 64: rnd(104, 64)}
A25 = AD[32]
PAL = b"ACGGTCATGCATGACCGT"            # its own reverse complement (18)
_X, _Z = rnd(105, 13), rnd(106, 6)
HALF = _X + _Z + rc(_Z)                # rc(HALF) = _Z rc(_Z) rc(_X): its last 12 bases start its reverse complement
KINNEX = [rnd(200 + i, 25) for i in range(16)]
A64 = [rnd(300 + i, 20) for i in range(64)]
MIXED = [b"g", rnd(31, 8), rnd(32, 16).lower(), rnd(33, 25), rnd(34, 64), rnd(35, 40).lower()]

SETS = [
    ([A25], 75),                 # 0: A = 1, 32 rows
    ([AD[16]], 75),              # 1: 16 rows
    ([AD[48], rnd(107, 45)], 75),  # 2: 48 rows, an adapter-filter set
    ([AD[64]], 75),              # 3: 64 rows, every pattern as long as the rows
    ([A25], 20),                 # 4: a low threshold, for long degraded copies
    ([A25], 76),                 # 5: 100 x 19 = 76 x 25
    ([PAL, A25], 75),            # 6
    ([A25, AD[16], A25], 75),    # 7: two identical adapters
    ([HALF], 75),                # 8
    (KINNEX, 75),                # 9
    (A64, 75),                   # 10: A = 64
    (MIXED, 75),                 # 11: lengths 1, 8, 16, 25, 64, 40 in 64 rows
    ([A25.lower()], 75),         # 12
    ([b"A" * 20], 75),           # 13: poly-A
]
ROWS_SET = {32: 0, 16: 1, 48: 2, 64: 3}
TRACKED: list = []


def cases():
    out = []

    def add(name, si, ccs, tracked=False, **expect):
        out.append((name, si, bytes(ccs), expect))
        if tracked:
            TRACKED.append(name)

    # ---- tile edges, per row class
    for rows, si in ROWS_SET.items():
        ad, L, wu = AD[rows], len(AD[rows]), WU[rows]
        n = 3 * TC + 200
        r = rnd(400 + rows, n)
        # hits ending at t0 - 1, t0 and t0 + 1 of three tiles
        ends = [TC - 1, 2 * TC, 3 * TC + 1]
        for e in ends:
            r = put(r, e - L, ad)
        add(f"tile_ends_r{rows}", si, r, tracked=True, hits=[(0, 0, e - L, e) for e in ends])
        # inside the first WU columns, straddling a tile start, ending at column n
        r = rnd(500 + rows, n)
        r = put(put(put(r, 5, ad), TC - L // 2, rc(ad)), n - L, ad)
        assert 5 + L < wu
        add(f"tile_misc_r{rows}", si, r, tracked=True,
            hits=[(0, 0, 5, 5 + L), (0, 1, TC - L // 2, TC - L // 2 + L), (0, 0, n - L, n)])
        # a copy that starts exactly at the warm-up's first column and one that starts one before it
        r = rnd(600 + rows, n)
        r = put(put(r, TC - wu, ad), 2 * TC - wu - 1, ad)
        add(f"tile_warmup_edge_r{rows}", si, r, tracked=True,
            hits=[(0, 0, TC - wu, TC - wu + L), (0, 0, 2 * TC - wu - 1, 2 * TC - wu - 1 + L)])
    # a degraded copy with ten inserted read bases (span 35 = 1.4 L, score 25 - 20 = 5 = the threshold at T = 20),
    # ending two columns after a tile start
    ins = bytearray()
    for k, ch in enumerate(A25):
        ins.append(ch)
        if 7 <= k < 17:
            ins.append(other(A25[k + 1]))
    r = put(rnd(700, 2 * TC), TC + 2 - len(ins), bytes(ins))
    add("tile_long_span", 4, r, tracked=True, has=[(0, 0, TC + 2 - 35, TC + 2)])

    # ---- read lengths (set 0)
    add("n1", 0, b"A", tracked=True, hits=[])
    add("n_lt_L", 0, A25[:10], tracked=True, hits=[])
    add("n0", 0, b"", tracked=True, hits=[])   # (an empty read between two others)
    for n in (TC - 1, TC, TC + 1):
        add(f"n_{n}", 0, put(rnd(800 + n, n), n - 25, A25), tracked=True, hits=[(0, 0, n - 25, n)])
    n = 64 * TC + 5
    r = rnd(900, n)
    ends = [TC, 17 * TC - 1, 40 * TC + 1, 63 * TC + 12, n]
    for e in ends:
        r = put(r, e - 25, A25)
    add("n_64_tiles", 0, r, tracked=True, hits=[(0, 0, e - 25, e) for e in ends])
    for k in range(3):  # three short reads that share one wave
        add(f"short_{k}", 0, put(rnd(950 + k, 90 + k), 20 + k, rc(A25)), tracked=True, hits=[(0, 1, 20 + k, 45 + k)])

    # ---- the hit rule (set 0 unless said)
    bg = rnd(1000, 300)
    add("ends_L_apart", 0, put(bg, 100, A25 + A25), hits=[(0, 0, 100, 125)])
    add("ends_L_plus_1_apart", 0, put(bg, 100, A25 + bytes([other(A25[0])]) + A25), hits=[(0, 0, 100, 125), (0, 0, 126, 151)])
    add("higher_within_radius", 0, put(bg, 100, sub(A25, 12) + A25 + sub(A25, 12)), hits=[(0, 0, 125, 150)])
    # the copy without its last base, then a base that is not it: columns 124 and 125 both score 22
    add("plateau", 0, put(bg, 100, A25[:-1] + bytes([other(A25[-1])])),
        check=lambda h: len(h) == 1 and h[0][3] == 124 and h[0][4] == 22)
    add("tandem", 0, put(bg, 50, A25 * 6), hits=[(0, 0, 50, 75)])
    add("palindrome", 6, put(bg, 100, PAL), hits=[(0, 0, 100, 118)])
    add("identical_adapters", 7, put(bg, 100, A25), hits=[(0, 0, 100, 125), (2, 0, 100, 125)])
    add("orientations_half_L_apart", 8, put(bg, 100, _X + _Z + rc(_Z) + rc(_X)), hits=[(0, 0, 100, 125)])

    # ---- sets
    r = rnd(1100, 2000)
    for k in range(16):
        r = put(r, 60 + 120 * k, KINNEX[k] if k % 3 else rc(KINNEX[k]))
    add("kinnex_array", 9, r, hits=[(k, 0 if k % 3 else 1, 60 + 120 * k, 85 + 120 * k) for k in range(16)])
    add("last_of_64_reversed", 10, put(rnd(1101, 700), TC - 5, rc(A64[63])), hits=[(63, 1, TC - 5, TC + 15)])
    r = put(put(put(rnd(1102, 400), 20, MIXED[4]), 150, rc(MIXED[5])), 250, MIXED[3])
    add("mixed_lengths", 11, r,
        has=[(4, 0, 20, 84), (5, 1, 150, 190), (3, 0, 250, 275)], check=lambda h: any(x[0] == 0 for x in h))
    add("rows48_second_adapter", 2, put(rnd(1103, 700), 300, rc(SETS[2][0][1])), hits=[(1, 1, 300, 345)])
    # lower-case adapters; N in the read reads as A (code 0)
    ia, ic = A25.index(b"A", 8), A25.index(b"C", 8)
    add("n_for_a", 12, put(bg, 100, A25[:ia] + b"N" + A25[ia + 1:]), check=lambda h: len(h) == 1 and h[0][4] == 25)
    add("n_for_c", 12, put(bg, 100, (A25[:ic] + b"n" + A25[ic + 1:]).lower()), check=lambda h: len(h) == 1 and h[0][4] == 22)

    # ---- start
    add("start_exact", 0, put(bg, 100, A25), hits=[(0, 0, 100, 125)])
    add("start_substitution", 0, put(bg, 100, sub(A25, 3)), check=lambda h: [x[2:] for x in h] == [(100, 125, 22)])
    add("start_insertion", 0, put(bg, 100, A25[:9] + bytes([other(A25[9])]) + A25[9:]),
        check=lambda h: [x[2:] for x in h] == [(100, 126, 23)])
    add("start_deletion", 0, put(bg, 100, A25[:9] + A25[10:]), check=lambda h: [x[2:] for x in h] == [(100, 124, 22)])
    add("start_at_first_base", 0, A25 + bg, hits=[(0, 0, 0, 25)])

    # ---- threshold (T = 76: 19 is a candidate, 18 is not)
    add("score_at_T", 5, put(bg, 100, sub(sub(A25, 5), 15)), check=lambda h: [x[2:] for x in h] == [(100, 125, 19)])
    two_ins = A25[:8] + bytes([other(A25[8])]) + A25[8:16] + bytes([other(A25[16])]) + A25[16:]
    add("score_below_T", 5, put(bg, 100, sub(two_ins, 3)), hits=[])

    # ---- a missed adapter: t + adapter + rc(t)
    t = rnd(1200, 400)
    add("missed_adapter", 2, t + AD[48] + rc(t), hits=[(0, 0, 400, 445)])

    # ---- many candidates
    add("tandem_40", 0, A25 * 40, n_hits=1)
    # every column from 19 on is a candidate; each is suppressed by the one before it but column 20
    add("poly_a", 13, b"A" * 2000, hits=[(0, 0, 0, 20)])
    return out


CASES = cases()
NAMES = [c[0] for c in CASES]
_REF: dict = {}


def reference(i: int) -> list:
    """scan_ref.hits of case i as (adapter, orient, start, end, score), computed once."""
    if i not in _REF:
        _, si, ccs, _ = CASES[i]
        _REF[i] = R.hits(SETS[si][0], ccs, SETS[si][1])
    return _REF[i]


def by_set() -> dict:
    d: dict = {}
    for i, c in enumerate(CASES):
        d.setdefault(c[1], []).append(i)
    return d


def check_expect(hits, expect) -> None:
    coords = [h[:4] for h in hits]
    if "hits" in expect:
        assert coords == sorted(expect["hits"], key=lambda h: (h[3], h[0])), coords
    if "n_hits" in expect:
        assert len(hits) == expect["n_hits"], hits
    for h in expect.get("has", []):
        assert h in coords, (h, coords)
    if "check" in expect:
        assert expect["check"](hits), hits


REJECTED = {
    "bad_letter": [A25, b"ACGTNACGT"],
    "length_0": [A25, b""],
    "length_65": [rnd(1, 65)],
    "empty_set": [],
    "a_65": [A25] * 65,
}
REJECTED_T = (0, 101)

# (name, hits, n, lmin, pieces) for ccsx_scan_cut; a hit is (adapter, orient, start, end, score)
CUTS = [
    ("no_hit", [], 100, 50, [(0, 100, -1, -1)]),
    ("no_hit_short_read", [], 10, 50, [(0, 10, -1, -1)]),
    ("hit_at_0", [(0, 0, 0, 25, 25)], 200, 50, [(25, 200, 0, -1)]),
    ("hit_ending_at_n", [(0, 1, 175, 200, 25)], 200, 50, [(0, 175, -1, 0)]),
    ("overlapping_hits_merged", [(0, 0, 100, 125, 25), (1, 0, 110, 135, 25)], 300, 50, [(0, 100, -1, 0), (135, 300, 1, -1)]),
    ("touching_hits_merged", [(0, 0, 100, 125, 25), (1, 1, 125, 150, 25)], 300, 50, [(0, 100, -1, 0), (150, 300, 1, -1)]),
    ("pieces_lmin_minus_1_and_lmin", [(0, 0, 49, 74, 25), (0, 0, 124, 149, 25)], 300, 50, [(74, 124, 0, 1), (149, 300, 1, -1)]),
    # a long hit that ends after a later one: the left flank is the hit with the largest end
    ("flank_largest_end", [(1, 0, 120, 140, 20), (0, 0, 100, 160, 40)], 300, 50, [(0, 100, -1, 1), (160, 300, 1, -1)]),
    # two hits of different adapters at the same place: the first in list order flanks
    ("flank_first_in_list", [(0, 0, 100, 125, 25), (2, 0, 100, 125, 25)], 300, 50, [(0, 100, -1, 0), (125, 300, 0, -1)]),
    ("everything_covered", [(0, 0, 0, 30, 25)], 30, 1, []),
]


def accuracy_case(seed: int = 7):
    """SPEC.md §17's end-to-end case: three adapters of 25 bases, every pair,
    every adapter against every other's reverse complement and against its own
    at edit distance >= 9; 12 ZMWs of f(300) + ad[i] + f(300) + rc(ad[j]) +
    f(300), each with 8 subreads at 2 / 4 / 4 % errors, the odd ones
    reverse-complemented.  Returns (adapters, [(i, j)], [subreads])."""
    from .polish_ref import mutate
    rng = random.Random(seed)
    ads: list = []
    while len(ads) < 3:
        c = bytes(rng.choice(b"ACGT") for _ in range(25))
        if R.edit_distance(c, rc(c)) >= 9 and all(R.edit_distance(c, b) >= 9 and R.edit_distance(c, rc(b)) >= 9 for b in ads):
            ads.append(c)
    pairs, zmws = [], []
    f = lambda: bytes(rng.choice(b"ACGT") for _ in range(300))  # noqa: E731
    for _ in range(12):
        i, j = rng.randrange(3), rng.randrange(3)
        t = f() + ads[i] + f() + rc(ads[j]) + f()
        subs = [mutate(rng, t, .02, .04, .04) for _ in range(8)]
        pairs.append((i, j))
        zmws.append([s if k % 2 == 0 else rc(s) for k, s in enumerate(subs)])
    return ads, pairs, zmws
