"""Synthetic ZMW inputs shared by the CPU and GPU tests (seeded, deterministic)."""
from __future__ import annotations

import random

import numpy as np

import ccsx_amd as cx

SEED = 20201104


def synth(hole: int, L: int, passes: int, seed: int = SEED) -> cx.Prepared:
    subs, _ = cx.synth_zmw(seed, hole, L, passes)
    return cx.prepare(subs)


def raw(segs: list[bytes]) -> cx.Prepared:
    """Segments given directly (already strand-normalised), push order as listed."""
    offs, o = [], 0
    for s in segs:
        offs.append(o)
        o += len(s)
    return cx.Prepared(b"".join(segs), np.array(offs, np.uint32), np.array([len(s) for s in segs], np.uint32))


def mutate(rng: random.Random, s: bytes, p_ins=0.06, p_del=0.03, p_sub=0.01) -> bytes:
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < p_del:
            pass
        elif u < p_del + p_sub:
            out.append(rng.choice([b for b in b"ACGT" if b != c]))
        else:
            out.append(c)
        if rng.random() < p_ins:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def edge_cases() -> dict[str, cx.Prepared]:
    rng = random.Random(7)
    ins = bytes(rng.choice(b"ACGT") for _ in range(3500))
    cases = {}
    cases["one_segment"] = raw([mutate(rng, ins)])
    cases["two_segments"] = raw([mutate(rng, ins), mutate(rng, ins)])
    cases["short_reads_60bp"] = raw([mutate(rng, ins[:60]) for _ in range(6)])
    cases["shorter_than_band"] = raw([mutate(rng, ins[:100]) for _ in range(5)])
    cases["with_empty_segment"] = raw([mutate(rng, ins), b"", mutate(rng, ins), mutate(rng, ins), mutate(rng, ins)])
    cases["identical_reads"] = raw([ins] * 5)
    cases["unrelated_reads"] = raw([bytes(rng.choice(b"ACGT") for _ in range(3100)) for _ in range(5)])
    hp = b"".join(bytes([rng.choice(b"ACGT")]) * rng.randint(1, 9) for _ in range(700))
    cases["homopolymers"] = raw([mutate(rng, hp) for _ in range(7)])
    lc = bytes(rng.choice(b"ACGTacgtN") for _ in range(3200))
    cases["lowercase_and_N"] = raw([mutate(rng, lc) for _ in range(5)])
    cases["noisy_no_breakpoint"] = raw([mutate(rng, ins, 0.15, 0.10, 0.05) for _ in range(6)])
    cases["ragged_lengths"] = raw([mutate(rng, ins[rng.randint(0, 300):3500 - rng.randint(0, 300)]) for _ in range(8)])
    cases["many_passes_short"] = raw([mutate(rng, ins[:1200]) for _ in range(40)])
    cases["over_64_reads"] = raw([mutate(rng, ins[:700]) for _ in range(70)])
    return cases


# ---------------------------------------------------------------------------
# Constructed cases for the traceback records, the band edges and the tie
# rules (tests/test_record_cases.py states what each family must reach, from
# the oracle's debug counters; tests/test_gpu_records.py compares every kernel
# object with the oracle on them).  Each family returns {name: list of reads}.
# Exact reads, no random errors: what a case reaches is decided by its
# construction, and the seeds are chosen so that no accidental equal-score
# alternative moves a junction.
# ---------------------------------------------------------------------------
LADDER_DIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)
# Nested ladders: (skips, extra rows).  A read that deletes the last d - 1
# bases of Mid makes its own edge only while no existing edge plus a short
# deletion or insertion is cheaper (O + E per base), i.e. while every existing
# skip is longer than 2 d - 1: the skips are listed longest first, each more
# than twice the next.  An extra row is a substitution of Mid's last base: one
# more predecessor of S[0], and every skip edge one row longer.  The junction
# row S[0] then has the predecessor distances given beside each nest.
LADDER_NESTS = {
    "np3_4": (((33, 16), 0), ((17, 8), 0), ((9, 4), 0), ((5, 2), 0), ((8, 3), 0)),  # {1, a, b}
    "np5+": (((33, 16, 8, 4, 2), 0),      # {1, 2, 4, 8, 16, 33}
             ((16, 8, 4, 2), 1),          # {1, 2, 3, 5, 9, 17}
             ((33, 16, 8, 4), 0)),        # {1, 4, 8, 16, 33}: five, the smallest far row
}


def _rb(rng: random.Random, n: int) -> bytes:
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _pms(seed: int, lp: int = 300, lm: int = 40, ls: int = 300):
    """P, Mid, S of a deletion ladder, such that a deleted suffix of Mid and a
    deleted S[0] or S[0..1] have one best placement: Mid's last base and S[0]
    are the two letters the rest of Mid does not use (the deleted block cannot
    slide left or right), and S[1], S[2] differ from S[0]."""
    rng = random.Random(seed)
    x, y, w, v = rng.sample(list(b"ACGT"), 4)
    P, S = _rb(rng, lp), bytearray(_rb(rng, ls))
    M = bytes(rng.choice((x, y)) for _ in range(lm - 1)) + bytes([w])
    S[0] = v
    for i in (1, 2):
        if S[i] == v:
            S[i] = w
    return P, M, bytes(S)


def _nest_reads(P: bytes, M: bytes, S: bytes, skips, what: str, fulls: int = 2, extra: int = 0) -> list[bytes]:
    """A nested deletion ladder: `fulls` reads P + Mid + S, `extra` reads with
    Mid's last base substituted, then per skip d a read that deletes the last
    d - 1 bases of Mid (it creates an edge into S[0]), then the reads that use
    the edges: what = "M": the same reads again (M moves over each edge) and a
    full read; what = "D": reads that also delete S[0] (a D move over each
    edge), S[0] alone after a full Mid, and S[0..1] (D-ext chains)."""
    full = P + M + S
    skip = {d: P + M[:len(M) - (d - 1)] for d in skips}
    subs = [b for b in b"ACGT" if b not in (M[-1], S[0])][:extra]
    reads = [full] * fulls + [P + M[:-1] + bytes([b]) + S for b in subs] + [skip[d] + S for d in skips]
    if what == "M":
        reads += [skip[d] + S for d in skips] + [full]
    else:
        reads += [skip[d] + S[1:] for d in skips] + [P + M + S[1:], skip[skips[-1]] + S[2:]]
    return reads


def ladder_cases() -> dict[str, list[bytes]]:
    """Deletion ladders: a later read retraces a skip edge of row distance d in
    M state, another crosses it in D state and in a D-ext chain, for d in
    LADDER_DIST and junction rows of 1, 2, 3, 5 and 6 predecessors (up to 13
    reads in the six-predecessor cases)."""
    cases = {}
    for d in LADDER_DIST[1:]:
        # one predecessor, d rows back: X is inserted after P, then Y (d - 1
        # bases) between P and X, so X[0] keeps P[-1] as its only predecessor.
        # X and Y use different letters (Y never aligns to X); an inserted
        # block slides left when its last base equals P[-1] and right when its
        # first equals S[0], a deleted X[0] or X[0..1] when it equals the base
        # after it
        rng = random.Random(1000 + d)
        a, b, c, e = rng.sample(list(b"ACGT"), 4)
        P, S = _rb(rng, 299) + bytes([c]), bytes([b]) + _rb(rng, 299)
        X = bytes([a, b, b]) + bytes(rng.choice((a, b)) for _ in range(9))
        Y = bytes(rng.choice((c, e)) for _ in range(d - 2)) + bytes([e])
        cases[f"np1_d{d}"] = [P + S, P + X + S, P + Y + S, P + X + S, P + X[1:] + S, P + X[2:] + S, P + X + S]
        # two predecessors: the plain ladder
        cases[f"np2_d{d}_M"] = _nest_reads(*_pms(2000 + d), (d,), "M")
        cases[f"np2_d{d}_D"] = _nest_reads(*_pms(2000 + d), (d,), "D")
    for cls, nests in LADDER_NESTS.items():
        for skips, extra in nests:
            tag = "_".join(str(d) for d in skips) + (f"_x{extra}" if extra else "")
            P, M, S = _pms(3000 + 10 * skips[0] + extra)
            fulls = 1 if len(skips) + extra > 4 else 2
            cases[f"{cls}_s{tag}_M"] = _nest_reads(P, M, S, skips, "M", fulls, extra)
            cases[f"{cls}_s{tag}_D"] = _nest_reads(P, M, S, skips, "D", fulls, extra)
    # The rows a skip edge jumps over descend from its origin: a traceback that
    # decodes too short a distance lands among them and their D chain leads it
    # back to the origin at the same read base -- the same events.  Here a
    # read Z + S first puts |Z| rows with no way back in front of S[0] (LEAD
    # columns: Z[0] has no predecessor), so Mid's last row and the skip
    # origins lie |Z| rows further back and a shorter move ends in Z.
    for lz in (3, 4, 5, 7, 8, 15):
        P, M, S = _pms(3500 + lz)
        Z = bytes(([S[0], M[-1]] * lz)[:lz])  # (the two letters the rest of Mid does not use)
        full, skip = P + M + S, P + M[:-3]
        cases[f"lead_block_{lz}"] = [full, full, Z + S, skip + S, full, skip + S, full[:len(P) + len(M)] + S[1:],
                                     skip + S[1:], skip + S[2:]]
    return cases


BLOCK_D17_RESIDUES = (0, 1, 31)


def block_edge_cases() -> dict[str, list[bytes]]:
    """The distance-5 ladder with |P| = 300 .. 331: the junction row P + Mid
    lands on every residue of a 32-row traceback block (the move leaves the
    block for residues 0 .. 3); a distance-17 ladder at residues 0, 1, 31."""
    cases = {}
    for lp in range(300, 332):
        P, M, S = _pms(4000 + lp, lp=lp)
        res = (lp + len(M)) % 32
        cases[f"d5_res{res:02d}"] = _nest_reads(P, M, S, (5,), "M") + _nest_reads(P, M, S, (5,), "D")[3:]
    for res in BLOCK_D17_RESIDUES:
        lp = 300 + (res - 340) % 32
        P, M, S = _pms(4100 + res, lp=lp)
        cases[f"d17_res{res:02d}"] = _nest_reads(P, M, S, (17,), "M") + _nest_reads(P, M, S, (17,), "D")[3:]
    return cases


BAND_INS = (60, 61, 62, 63, 64, 65, 126, 127, 128, 129, 130, 200)
BAND_DEL = (60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 128, 129, 130)
BAND_M = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
BAND_OFFSETS = (1, 2, 63, 64, 65, 127, 128, 200)


def band_cases() -> dict[str, list[bytes]]:
    """The band (W = 128) at its edges: long insertions and deletions in later
    reads, read lengths around the 64-lane multiples against longer and
    shorter graphs, reads that start and stop inside the graph, graphs that
    start inside the read, and bubbles of two unrelated branches (bands that
    jump between consecutive rows)."""
    rng = random.Random(5000)
    T = _rb(rng, 500)
    cases = {}
    for n in BAND_INS:
        ins = _rb(rng, n)
        cases[f"ins{n}"] = [T, T, T[:250] + ins + T[250:], T[:250] + ins + T[250:], T]
    for n in BAND_DEL:
        cases[f"del{n}"] = [T, T, T[:200] + T[200 + n:], T[:200] + T[200 + n:], T]
    for m in BAND_M:
        # (a read of m bases out of the middle of a 400-base graph, and a graph
        # of about half the read out of the read's middle)
        cases[f"m{m}_long_graph"] = [T[:400], T[:400], T[100:100 + m], T[:m]]
        h = max(1, m // 2)
        a = (m - h) // 2
        cases[f"m{m}_short_graph"] = [T[a:a + h], T[a:a + h], T[:m], T[:m]]
    for a in BAND_OFFSETS:
        cases[f"inner_{a}"] = [T, T, T[a:500 - a], T[a:], T[:500 - a], T]
        cases[f"outer_{a}"] = [T[a:500 - a], T[a:500 - a], T, T[a:], T]
    # (different letters: neither branch aligns to the other as mismatches)
    A, B = bytes(rng.choice(b"AC") for _ in range(100)), bytes(rng.choice(b"GT") for _ in range(100))
    # (the band cannot follow a 100-base branch swap: the path is lost and the
    # rest of the read becomes trailing INS; a 40-base one is followed)
    cases["bubble_100_lost"] = [T[:200] + A + T[200:400], T[:200] + B + T[200:400]] * 2 + [T[:400]]
    cases["bubble_40"] = [T[:200] + A[:40] + T[200:400], T[:200] + B[:40] + T[200:400]] * 2 + [T[:400]]
    return cases


def tie_cases() -> dict[str, list[bytes]]:
    """Inputs where equal scores are the rule (SPEC.md §3.1, §3.2, §3.4, §3.5,
    §6): every alignment here has many equally good placements."""
    rng = random.Random(6000)
    cases = {}
    for b in b"AT":
        cases[f"homopolymer_{chr(b)}"] = [bytes([b]) * n for n in (200, 190, 210, 200, 1, 130, 260)]
    cases["dinucleotide"] = [b"AC" * n for n in (100, 95, 105, 100, 64)] + [b"CA" * 100]
    cases["trinucleotide"] = [b"ACG" * n for n in (70, 66, 74, 70)] + [b"CGA" * 70, b"ACG" * 43 + b"A"]
    for period, copies in ((5, (40, 36, 44, 40, 39)), (17, (12, 10, 14, 12, 11)), (64, (5, 4, 6, 5, 3)),
                           (130, (4, 3, 5, 4, 2))):
        unit = _rb(rng, period)
        flank = _rb(rng, 40), _rb(rng, 40)
        cases[f"tandem_{period}"] = [flank[0] + unit * c + flank[1] for c in copies]
    cases["two_letter"] = [bytes(rng.choice(b"AC") for _ in range(n)) for n in (300, 300, 280, 320, 300, 150)]
    base = bytes(rng.choice(b"AC") for _ in range(300))
    cases["two_letter_related"] = [base, base[:100] + base[104:], base[:200] + b"AC" + base[200:], base, base[3:-3]]
    cases["only_N"] = [b"N" * n for n in (150, 140, 160, 150)]
    cases["N_and_A"] = [b"N" * 150, b"A" * 150, b"n" * 145, b"NANA" * 40]
    T = _rb(rng, 300)

    def sub(c: int, b: bytes) -> bytes:
        return T[:c] + b + T[c + 1:]
    # the same column split 2 / 2 and 2 / 2 / 2 (ties go to the smallest base), at three columns
    cases["split_2_2"] = [sub(150, b"G"), sub(150, b"C"), sub(150, b"G"), sub(150, b"C")]
    cases["split_2_2_2"] = [sub(90, b"T"), sub(90, b"G"), sub(90, b"C"), sub(90, b"T"), sub(90, b"G"), sub(90, b"C")]
    cases["split_first_last_column"] = [b"T" + T[1:-1] + b"G", b"A" + T[1:-1] + b"C", b"T" + T[1:-1] + b"C",
                                        b"A" + T[1:-1] + b"G"]
    # columns where cnt[best] == gap: an insertion / a deletion carried by exactly half the reads
    ins = T[:120] + b"GATTACA" + T[120:]
    dele = T[:180] + T[190:]
    cases["gap_equals_best_ins"] = [T, ins, T, ins]
    cases["gap_equals_best_del"] = [T, dele, dele, T]
    cases["gap_equals_best_3_3"] = [T, ins, T, ins, ins, T]
    return cases


# ---------------------------------------------------------------------------
# Constructed cases for the shredding loop around the POA call (SPEC.md §7:
# the breakpoint scan, the window growth, the cursors, the emission over
# several rounds).  tests/test_shred_cases.py states which class each case
# must reach, from the oracle's opoa_shred_hist; tests/test_gpu_shred.py
# compares every kernel object with the oracle on them.  Exact reads again.
# Three constructions:
#   copies     n exact copies of T[:L], with single substituted bases: an
#              isolated substitution stays a mismatch (X = -6 against two gaps,
#              2 (O + E) = -10), so column c of the first 2,000-base window is
#              T's base c and the number of reads carrying it is chosen freely.
#              A "dirty" column (n = 5: two reads keep the base, two carry a
#              second, one a third; 2 * 100 < 60 * 5) rejects every candidate
#              window that holds it; dirty columns every 9 bases from c to the
#              window's end make c - 10 the first accepted candidate, at depth
#              (ncols - 10) - i = 2000 - c.
#   zone       reads 0 and 1 carry a random string over {A, C}, read 2 one
#              over {G, T}: nothing aligns, read 2's bases are gap-consensus
#              columns, the others' base columns read 2 never matches.  After a
#              shared prefix of p bases the scan accepts i = p - 5 (five base
#              columns, then five skipped gap columns).
#   lengths    which read makes a round final, and when.
# ---------------------------------------------------------------------------
SHRED_DEPTHS = (63, 64, 65, 100, 127, 128, 129)
SHRED_NS = (63, 64, 65, 128, 129)


def _other(b: int, j: int = 1) -> int:
    return b"ACGT"[(b"ACGT".index(b) + j) % 4]


def _copies(T: bytes, n: int, L: int, subs=(), dirty=()) -> list[bytes]:
    """n copies of T[:L]; subs: (read, column, j) substitutes T's base by the
    j-th next letter; dirty: columns made dirty (n = 5, see above)."""
    reads = [bytearray(T[:L]) for _ in range(n)]
    subs = list(subs) + [(k, c, j) for c in dirty for k, j in ((2, 1), (3, 1), (4, 2))]
    for k, c, j in subs:
        reads[k][c] = _other(T[c], j)
    return [bytes(r) for r in reads]


def _dirty_from(c: int) -> list[int]:
    """Dirty columns from c to the end of the first 2,000-base window, at most
    9 apart, the last one in 1990 .. 1995 (no candidate window above c - 10 is
    clean, none of them at the window's last bases)."""
    cols = list(range(c, 1996, 9))
    return cols if cols[-1] >= 1990 else cols + [1992]


def shred_cases() -> dict[str, list[bytes]]:
    rng = random.Random(7000)
    T = _rb(rng, 14000)
    L = 4200  # two rounds: 2,000 bases pushed, then the final push
    cases = {}
    # ---- lengths: rounds and termination
    cases["copies_3000"] = [T[:3000]] * 3          # pos + 2000 + 1000 == len: one final round
    cases["copies_3001"] = [T[:3001]] * 3          # one base longer: (1990, 2000) then the final round
    cases["copies_4990"] = [T[:4990]] * 3          # the first breakpoint leaves every cursor at len - 3000
    cases["copies_14000"] = [T[:14000]] * 3        # seven rounds
    for Lf in (2943, 2944, 2945):                  # final rounds of 64 m - 1, 64 m, 64 m + 1 columns
        cases[f"final_{Lf}"] = [T[:Lf]] * 3
    cases["two_reads"] = [T[:5000]] * 2
    cases["empty_segment"] = [T[:5000], b"", T[:5000], T[:5000]]
    cases["read0_short"] = [T[:3000], T[:4000], T[:4000]]
    cases["last_short"] = [T[:4000], T[:4000], T[:3000]]
    cases["ragged_1001"] = [T[:5000], T[:5200], T[:1001]]
    cases["span_end_edge"] = [T[:3000], T[:3000], T[:2944]]   # read 2's span ends at column 46 * 64
    cases["span_begin_edge"] = [T[:3000], T[:3000], T[64:3000]]  # ... begins at column 64
    # ---- zone: depths by the zone's length, small i, growth
    for k in (34, 35, 66):                         # depth 2 k - 5 = 63, 65, 127
        A, B, p, s = _rb2(rng, k, b"AC"), _rb2(rng, k, b"GT"), T[:2000 - k], T[2000:5200]
        cases[f"zone_{k}"] = [p + A + s, p + A + s, p + B + s]
    s = T[2000:6000]
    for pre in (6, 7, 10, 20):                     # i = pre - 5
        A, B = _rb2(rng, 2000 - pre, b"AC"), _rb2(rng, 2000 - pre, b"GT")
        cases[f"prefix_{pre}"] = [T[:pre] + A + s, T[:pre] + A + s, T[:pre] + B + s]
    A, B = _rb2(rng, 1990, b"AC"), _rb2(rng, 1990, b"GT")
    cases["prefix_10_read2_from_5"] = [T[:10] + A + s, T[:10] + A + s, T[5:10] + B + s]  # i = 5: no base of read 2 before it
    A, B, s = _rb2(rng, 2000, b"AC"), _rb2(rng, 2000, b"GT"), T[2000:8000]
    cases["dirty_2000_then_shared"] = [A + s, A + s, B + s]   # grows to 4,000, then finds a breakpoint
    for Ld in (3100, 5100, 7100):                  # 1, 2, 3 growths, then the final push
        A, B = _rb2(rng, Ld, b"AC"), _rb2(rng, Ld, b"GT")
        cases[f"dirty_{Ld}"] = [A, A, B]
    # read 1 lacks 44 single bases of the first window: its 2,000 bases reach
    # further into A, the MSA has 4,042 columns: ncols - 10 = 63 * 64, nothing found
    A, B = _rb2(rng, 3200, b"AC"), _rb2(rng, 3100, b"GT")
    a1 = bytearray(A)
    for x in range(44):
        del a1[1993 - 40 * x]
    cases["dirty_4042_columns"] = [A, bytes(a1), B]
    # ---- copies: the scan's steps of 64 candidates, bp_ok's thresholds
    for d in SHRED_DEPTHS:
        cases[f"depth_{d}"] = _copies(T, 5, L, dirty=_dirty_from(2000 - d))
    for c in (1993, 1994, 1995):                   # i = c - 10 = 1983, 1984 = 31 * 64, 1985
        cases[f"i_mod64_{(c - 10) % 64}"] = _copies(T, 5, L, dirty=[c])
    cases["col_n5_below"] = _copies(T, 5, L, dirty=[1990])    # 2 of 5: offsets 0 .. 9 of candidates 1990 .. 1981
    cases["col_n5_equal"] = _copies(T, 5, L, [(3, 1995, 1), (4, 1995, 1)])      # 3 of 5 at 60 %
    cases["col_n10_equal"] = _copies(T, 10, L, [(8, 1995, 1), (9, 1995, 1)])    # 8 of 10 at 80 %
    for n, c in ((9, 7), (10, 7), (9, 6), (10, 6)):           # 7 and 6 reads agree: 60 % of 9, not 80 % of 10
        cases[f"col_n{n}_c{c}"] = _copies(T, n, L, [(k, 1995, 1) for k in range(c, n)])
    # read 4 mismatches at 3 of the top window's 10 columns (7 < 8), then at 2 of candidate 1987's
    cases["row_below_then_equal"] = _copies(T, 5, L, [(4, 1991, 1), (4, 1994, 1), (4, 1997, 1)])
    cases["rows_at_i"] = _copies(T, 5, L, [(4, 1990, 1), (3, 1989, 1)])         # two rows in columns i and i - 1
    for g in (1, 2, 3, 4):
        # g bases inserted in read 1 six columns under a dirty column: the
        # first clean candidate's window holds g gap columns, nogwin = 10 - g
        # (g = 4: candidate 1950 is clean but for its leading gap column)
        reads = _copies(T, 5, L, dirty=_dirty_from(1956))
        ins = bytes(_other(T[1950], 1 + x % 2) for x in range(g))
        reads[1] = reads[1][:1950] + ins + reads[1][1950:]
        cases[f"nogwin_{10 - g}"] = reads
    # ---- cursors: an insertion in one read and a deletion in another before the breakpoint
    cases["indel"] = [T[:L], T[:500] + b"GAT" + T[500:L], T[:900] + T[904:L]]
    for n in SHRED_NS:
        # read counts around the 64-read mask words; the reads at the words'
        # edges carry an insertion, the last one a deletion
        reads = [T[:3001]] * n
        for k in {0, 62, 63, 64, 127, 128} & set(range(n - 1)):
            reads[k] = T[:700] + bytes([_other(T[700]), _other(T[700], 2)]) + T[700:3001]
        reads[n - 1] = T[:1200] + T[1203:3004]
        cases[f"n{n}"] = reads
    return cases


def _rb2(rng: random.Random, n: int, letters: bytes) -> bytes:
    return bytes(rng.choice(letters) for _ in range(n))


def shred_golden_entry(poa, reads: list[bytes]) -> dict:
    """What tests/golden/shred_cases.json keeps per case (tools/make_golden.py):
    the SHA-256 of the oracle's shredded CCS and its whole breakpoint log."""
    import hashlib
    z = raw(reads)
    ccs, log = poa.zmw_breakpoints(z.seqs, z.offs, z.lens)
    return {"sha256": hashlib.sha256(ccs).hexdigest(), "len": len(ccs), "log": [[int(a), int(b)] for a, b in log]}


def hbm_cursor_zmw(seed: int = 7100):
    """3 reads: a 4,100-base disjoint-alphabet zone (two growths: the pushed
    6,000-base window exceeds the tight read cap), then 3 exact copies of a
    100,200-base random string (segments beyond the LDS read buffer: the re-run
    with full caps takes the HBM-read instance, whose cursors then advance over
    about 55 rounds)."""
    rng = random.Random(seed)
    A, B, S = _rb2(rng, 4100, b"AC"), _rb2(rng, 4100, b"GT"), _rb(rng, 100200)
    return [A + S, A + S, B + S]


RECORD_FAMILIES = {"ladder": ladder_cases, "block_edge": block_edge_cases, "band": band_cases, "tie": tie_cases}


def record_digest(cns, msa) -> str:
    """SHA-256 of the consensus codes, then the MSA's shape and bytes."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(cns, np.uint8).tobytes())
    h.update(np.asarray(msa.shape, np.uint32).tobytes())
    h.update(np.ascontiguousarray(msa, np.uint8).tobytes())
    return h.hexdigest()


def record_golden_entry(poa, reads: list[bytes]) -> dict:
    """What tests/golden/record_cases.json keeps per case (tools/make_golden.py):
    the oracle's CCS in both modes and the digest of poa()'s consensus codes
    and MSA (hashes, not MSAs, keep the file small)."""
    z = raw(reads)
    cns, msa = poa.poa(reads)
    return {"ccs_shred": poa.zmw(z.seqs, z.offs, z.lens, 0).decode(),
            "ccs_primitive": poa.zmw(z.seqs, z.offs, z.lens, 1).decode(), "sha256": record_digest(cns, msa)}


def high_indegree(seed: int = 7):
    """91 reads P + M[:k] + S (k = 100 .. 10): each deletes a different suffix
    of M, so S's first node gets one in-edge per read -- a far row with more
    than 63 predecessors (more than a 6-bit slot tag holds)."""
    import random
    rnd = random.Random(seed)

    def rb(n):
        return bytes(rnd.choice(b"ACGT") for _ in range(n))
    P, M, S = rb(300), rb(100), rb(300)
    return [P + M[:k] + S for k in range(100, 9, -1)]
