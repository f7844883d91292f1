"""The constructed family shred_cases() of tests/zmw_cases.py on the oracle
alone: the shredding loop around the POA call (SPEC.md §7; main.c:541-641) --
the breakpoint scan, the window growth, the per-read cursors, the emission over
several rounds.

MUST below is the contract of the generator: per class of the oracle's
opoa_shred_hist the case that has to reach it, so a change that silently stops
reaching a class fails here, on any machine.  TRY lists classes that were
searched for; what was found is asserted like a MUST class, what was not is
recorded in DESIGN.md §1.  The oracle's results on the family are pinned by
tests/golden/shred_cases.json (tools/make_golden.py), and the two other
restatements of the loop (tests/quality_ref.py, tests/pass_ref.py) must agree
with the oracle on every case.

test_mutant_is_caught shows that the family discriminates: a third, parametric
restatement of the loop equals the oracle on every case as it stands, and each
single wrong rule (a `<=` for a `<`, a skipped candidate, a cursor advanced one
column too far ...) changes the CCS or the breakpoint log of the case named
beside it.  tests/test_gpu_shred.py compares every kernel object with the
oracle on the same cases.  Everything is an integer equality.

What the classes mean for the kernel (ccsx_kernel.hip): find_breakpoint tests
64 candidates per ballot from ncols - 10 downwards, so the accepted candidate's
depth (ncols - 10) - i decides the ballot and the lane; bp_ok evaluates the four
integer thresholds from popcounts of the column masks; emit advances cursor k by
a ballot-popcount over the rows [0, colrow[i]) in chunks of 64 rows, per 64-read
mask word, and writes the consensus in chunks of 64 columns; pass_stats takes
each read's span ends relative to those 64-column chunks.
"""
import json
import os
import time

import numpy as np
import pytest

from oracle import oracle as o
from tests import pass_ref as pr
from tests import quality_ref as qr
from tests.quality_ref import ADDLEN, INITLEN, MINLEN, MINWIN, ROWRATE, WINDOW, column_quals
from tests.zmw_cases import SHRED_DEPTHS, SHRED_NS, raw, shred_cases, shred_golden_entry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shred_cases.json")

# class of opoa_shred_hist -> the case that must reach it
MUST = [
    # rounds and termination
    ("rounds_1", "copies_3000"), ("rounds_2", "copies_3001"), ("rounds_3_5", "zone_34"), ("rounds_ge6", "copies_14000"),
    ("fin_n_lt3", "two_reads"), ("fin_empty", "empty_segment"), ("fin_nobase", "empty_segment"),
    ("fin_exact", "copies_3000"),      # pos + ws + 1000 == len
    ("notfin_by1", "copies_3001"),     # one base longer: not final
    ("fin_read0_only", "read0_short"), ("fin_last_only", "last_short"),
    ("fin_ragged", "ragged_1001"),     # remaining lengths 1,001 against >= 5,000
    # growth
    ("grow_0", "copies_3001"), ("grow_1", "dirty_3100"), ("grow_2", "dirty_5100"), ("grow_ge3", "dirty_7100"),
    ("grow_found", "dirty_2000_then_shared"), ("grow_final", "dirty_5100"),
    ("push_gt4096", "dirty_2000_then_shared"), ("push_gt4096", "dirty_5100"), ("push_gt4096", "ragged_1001"),
    # the accepted candidate
    ("d0", "copies_3001"), ("d1_62", "col_n5_below"), ("d63", "depth_63"), ("d63", "zone_34"), ("d64", "depth_64"),
    ("d65", "depth_65"), ("d65", "zone_35"), ("d66_126", "depth_100"), ("d127", "depth_127"), ("d127", "zone_66"),
    ("d128", "depth_128"), ("d_ge129", "depth_129"), ("d_gt1000", "prefix_10"),
    ("i_le16", "prefix_10"), ("i_le16", "prefix_20"),
    ("none_mult64", "dirty_4042_columns"),
    # bp_ok
    ("rej_leadgap", "zone_34"), ("gap_skip", "zone_34"), ("rej_nog_lt5", "zone_34"), ("acc_nog5", "zone_34"),
    ("acc_nog6_9", "nogwin_6"), ("acc_nog6_9", "nogwin_7"), ("acc_nog6_9", "nogwin_8"), ("acc_nog6_9", "nogwin_9"),
    ("acc_nog10", "copies_3001"),
    ("rej_col_by1", "col_n5_below"), ("acc_col_eq_n5", "col_n5_equal"), ("acc_col_eq_n10", "col_n10_equal"),
    ("acc_n9_c7", "col_n9_c7"), ("rej_n10_c7", "col_n10_c7"), ("acc_n9_c6", "col_n9_c6"), ("rej_n10_c6", "col_n10_c6"),
    ("rej_row_by1", "row_below_then_equal"), ("acc_row_eq_nog10", "row_below_then_equal"),
    ("acc_row_eq_nog5", "prefix_10"),
] + [(f"rej_col_off{x}", "col_n5_below") for x in range(10)] + [
    # cursors and emission
    ("adv_differ", "indel"), ("gapcol_base", "indel"), ("gapcol_base", "zone_34"),
    ("rows_i_ge2", "rows_at_i"), ("rows_im1_ge2", "rows_at_i"),
    ("colrow_mod0", "i_mod64_0"), ("colrow_mod1", "i_mod64_1"), ("colrow_mod63", "i_mod64_63"),
    ("i_mod0", "i_mod64_0"), ("i_mod1", "i_mod64_1"), ("i_mod63", "i_mod64_63"),
    ("fin_i_mod0", "final_2944"), ("fin_i_mod1", "final_2945"), ("fin_i_mod63", "final_2943"),
    ("n3", "copies_3001"), ("n9", "col_n9_c7"), ("n10", "col_n10_equal"),
] + [(f"n{n}", f"n{n}") for n in SHRED_NS] + [(b, f"n{n}") for n in SHRED_NS for b in ("adv_differ", "gapcol_base")] + [
    ("ccs_cross64", "copies_3001"),
    ("span_end_edge", "span_end_edge"), ("span_beg_edge", "span_begin_edge"),
]
# searched for (ISSUE: "try"); found ones are asserted, the others are in DESIGN.md §1
TRY_FOUND = [
    ("i_1", "prefix_6"), ("i_2", "prefix_7"),
    ("nobase", "prefix_10_read2_from_5"),   # a read with no base among a non-final round's emitted columns
    ("next_exact", "copies_4990"),          # a breakpoint that leaves a cursor exactly at len - 3000
]
TRY_NOT_FOUND = ["none_lt64"]  # a scan of an MSA of fewer than 74 columns: a pushed window has >= 2,000


@pytest.fixture(scope="module")
def runs():
    """Per case: (prepared ZMW, CCS, breakpoint log, shred_hist), one Poa, single-threaded."""
    p = o.Poa()
    out = {}
    t0 = time.perf_counter()
    for name, reads in shred_cases().items():
        z = raw(reads)
        with o.counting():
            ccs, log = p.zmw_breakpoints(z.seqs, z.offs, z.lens)
        out[name] = (z, ccs, [(int(a), int(b)) for a, b in log], o.shred_hist(True))
    print(f"\nshred_cases(): {len(out)} cases, oracle {time.perf_counter() - t0:.2f} s")
    return out


def test_case_limits():
    """Seeded and deterministic; at most 14,000 bases a read; 3 reads, or 5 /
    9 / 10 where a threshold needs them, but for one case per read-count class."""
    a, b = shred_cases(), shred_cases()
    assert a == b
    big = [name for name, reads in a.items() if len(reads) > 10]
    assert big == [f"n{n}" for n in SHRED_NS]
    for name, reads in a.items():
        assert 2 <= len(reads) <= 129 and max(len(r) for r in reads) <= 14000, name
    assert SHRED_DEPTHS == (63, 64, 65, 100, 127, 128, 129) and SHRED_NS == (63, 64, 65, 128, 129)


def test_counters_off_outside_counting():
    z = raw(shred_cases()["copies_3001"])
    o.reset_counters()
    o.Poa().zmw_breakpoints(z.seqs, z.offs, z.lens)
    assert not any(o.shred_hist().values())


@pytest.mark.parametrize("cls,case", MUST + TRY_FOUND, ids=[f"{c}-{k}" for c, k in MUST + TRY_FOUND])
def test_family_reaches(runs, cls, case):
    assert runs[case][3][cls] >= 1, f"shred_cases()[{case!r}] no longer reaches {cls}: log {runs[case][2][:6]}"


def test_try_list_outcome(runs):
    """What no input found reaches stays unreached (DESIGN.md §1 says why); the
    day a case reaches it, it moves to TRY_FOUND."""
    for cls in TRY_NOT_FOUND:
        assert not [k for k, r in runs.items() if r[3][cls]], cls
    assert set(c for c, _ in MUST + TRY_FOUND) | set(TRY_NOT_FOUND) == set(o.SHRED_BINS)


def test_depths_and_logs_by_construction(runs):
    """The copies cases' first breakpoint is where the construction puts it."""
    for d in SHRED_DEPTHS:
        assert runs[f"depth_{d}"][2][0] == (1990 - d, 2000), d
    assert runs["copies_3000"][2] == [(3000, 3000)]
    assert runs["copies_3001"][2] == [(1990, 2000), (1011, 1011)]
    assert runs["copies_4990"][2] == [(1990, 2000), (3000, 3000)]
    assert runs["col_n5_below"][2][0] == (1980, 2000) and runs["col_n5_equal"][2][0] == (1990, 2000)
    assert runs["col_n9_c7"][2][0] == (1990, 2000) and runs["col_n10_c7"][2][0] == (1985, 2000)
    assert runs["row_below_then_equal"][2][0] == (1987, 2000)
    for g in (1, 2, 3, 4):  # g gap columns in the accepted window
        i, ncols = runs[f"nogwin_{10 - g}"][2][0]
        assert ncols == 2000 + g and i <= 1949 < i + WINDOW
    assert [len(runs[f"dirty_{L}"][2]) for L in (3100, 5100, 7100)] == [1, 1, 1]
    assert len(runs["copies_14000"][2]) == 7
    for k, depth in ((34, 63), (35, 65), (66, 127)):
        i, ncols = runs[f"zone_{k}"][2][0]
        assert (i, ncols) == (1995 - k, 2000 + k) and ncols - WINDOW - i == depth
    assert [runs[f"prefix_{p}"][2][0][0] for p in (6, 7, 10, 20)] == [1, 2, 5, 15]
    assert (runs["dirty_4042_columns"][3]["none_mult64"], runs["dirty_4042_columns"][3]["grow_1"]) == (1, 1)


def test_oracle_reproduces_golden(runs):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(want) == sorted(runs)
    p = o.Poa()
    for name, reads in shred_cases().items():
        assert shred_golden_entry(p, reads) == want[name], f"{name}: the oracle moved"


def test_three_restatements_agree(runs):
    """quality_ref and pass_ref restate the loop from Poa.poa's MSA; each
    asserts its own CCS and breakpoint log against the oracle's."""
    for name, (z, ccs, log, _) in runs.items():
        qccs, qual, qlog = qr.reference(z, 0)
        pccs, rec, plog = pr.reference(z, 0)
        assert qccs == ccs and pccs == ccs and qlog == log and plog == log, name
        assert len(qual) == len(ccs) and rec.shape == (len(z.lens), 6), name


# --------------------------------------------------------------------------
# A parametric restatement of the loop (after tests/quality_ref.py _run and
# _breakpoint), every rule an argument.
# --------------------------------------------------------------------------
class Stuck(Exception):
    """A mutant that can neither find a breakpoint nor grow the window."""


RULES = dict(
    col_rejects=lambda colcnt, colrate, n: colcnt * 100 < colrate * n,
    row_rejects=lambda rc, nogwin: rc * 100 < ROWRATE * nogwin,
    few_columns=lambda nogwin: nogwin < MINWIN,
    colrate=lambda n: 60 if n < 10 else 80,
    lead_gap_rejects=True,
    gaps_count=False,
    skip_depth=lambda d: False,
    over=lambda lim, ln: lim >= ln,
    final_reads=lambda n: range(n),
    advance=lambda has, base, i: has[:i].sum(0),
    max_growths=None,
    cand_min=1,
)


def _scan(cons, eq, n, r) -> int:
    ncols = len(cons)
    if ncols <= WINDOW:
        return 0
    base = cons < 4
    colcnt = eq.sum(1)
    colrate = r["colrate"](n)
    top = ncols - WINDOW
    for i in range(top, r["cand_min"] - 1, -1):
        if r["skip_depth"](top - i):
            continue
        nogwin, ok = 0, True
        rowcnt = np.zeros(n, np.int64)
        for j in range(i, i + WINDOW):
            if not base[j]:
                nogwin += 1 if r["gaps_count"] and nogwin else 0
                if nogwin or not r["lead_gap_rejects"]:
                    continue
                ok = False
                break
            nogwin += 1
            rowcnt += eq[j]
            if r["col_rejects"](int(colcnt[j]), colrate, n):
                ok = False
                break
        if not ok or r["few_columns"](nogwin):
            continue
        if not any(r["row_rejects"](int(rc), nogwin) for rc in rowcnt):
            return i
    return 0


def restated(z, **mutation):
    """(ccs, breakpoint log) of the shredded mode under RULES + mutation."""
    r = dict(RULES, **mutation)
    poa = o.Poa()
    n = len(z.lens)
    offs, lens = [int(x) for x in z.offs], [int(x) for x in z.lens]
    ccs, log, pos, flag = bytearray(), [], [0] * n, True
    while flag:
        ws, grown = INITLEN, 0
        while True:
            fin = n < 3 or any(r["over"](pos[k] + ws + MINLEN, lens[k]) for k in r["final_reads"](n))
            if fin:
                flag = False
            reads = [z.seqs[offs[k] + pos[k]:offs[k] + (lens[k] if fin else min(pos[k] + ws, lens[k]))] for k in range(n)]
            _, msa = poa.poa(reads)
            cons, _, _, _, eq, has = column_quals(msa, n)
            if fin:
                i = len(cons)
                break
            i = _scan(cons, eq, n, r)
            if i >= 1:
                break
            if r["max_growths"] is not None and grown >= r["max_growths"]:
                raise Stuck
            ws, grown = ws + ADDLEN, grown + 1
        log.append((i, len(cons)))
        if flag:
            adv = r["advance"](has, cons < 4, i)
            pos = [pos[k] + int(adv[k]) for k in range(n)]
        ccs.extend(b"ACGT"[c] for c in cons[:i][cons[:i] < 4])
    return bytes(ccs), log


def test_restatement_equals_oracle(runs):
    for name, (z, ccs, log, _) in runs.items():
        assert restated(z) == (ccs, log), name


# mutant -> (the rule it gets wrong, the case that must show it)
MUTANTS = {
    "column rule <=": (dict(col_rejects=lambda c, rate, n: c * 100 <= rate * n), "col_n5_equal"),
    "column rule <= (n = 10)": (dict(col_rejects=lambda c, rate, n: c * 100 <= rate * n), "col_n10_equal"),
    "row rule <=": (dict(row_rejects=lambda rc, nog: rc * 100 <= ROWRATE * nog), "row_below_then_equal"),
    "row rule <= (nogwin = 5)": (dict(row_rejects=lambda rc, nog: rc * 100 <= ROWRATE * nog), "prefix_10"),
    "nogwin <= 5": (dict(few_columns=lambda nog: nog <= MINWIN), "zone_34"),
    "colrate switches at n <= 10": (dict(colrate=lambda n: 60 if n <= 10 else 80), "col_n10_c7"),
    "leading gap column skipped": (dict(lead_gap_rejects=False), "nogwin_6"),
    "gap columns counted into nogwin": (dict(gaps_count=True), "zone_34"),
    "depth a positive multiple of 64 skipped": (dict(skip_depth=lambda d: d > 0 and d % 64 == 0), "depth_64"),
    "depth a positive multiple of 64 skipped (128)": (dict(skip_depth=lambda d: d > 0 and d % 64 == 0), "depth_128"),
    "depth 63 mod 64 skipped": (dict(skip_depth=lambda d: d % 64 == 63), "depth_63"),
    "depth 63 mod 64 skipped (127)": (dict(skip_depth=lambda d: d % 64 == 63), "depth_127"),
    "depth 1 mod 64 skipped": (dict(skip_depth=lambda d: d % 64 == 1), "depth_65"),
    "final test >": (dict(over=lambda lim, ln: lim > ln), "copies_3000"),
    "final test on read 0 only": (dict(final_reads=lambda n: range(1)), "last_short"),
    "final test on all reads but the last": (dict(final_reads=lambda n: range(n - 1)), "ragged_1001"),
    "pos advanced over base columns only": (dict(advance=lambda has, base, i: (has[:i] & base[:i, None]).sum(0)), "indel"),
    "pos advanced through column i": (dict(advance=lambda has, base, i: has[:i + 1].sum(0)), "copies_3001"),
    "window grown once only": (dict(max_growths=1), "dirty_5100"),
    "cand >= 2": (dict(cand_min=2), "prefix_6"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_caught(runs, mutant):
    mutation, case = MUTANTS[mutant]
    z, ccs, log, _ = runs[case]
    try:
        got = restated(z, **mutation)
    except Stuck:
        return
    assert got != (ccs, log), f"{mutant}: {case} gives the oracle's CCS and breakpoint log all the same"
