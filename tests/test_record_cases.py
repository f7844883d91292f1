"""The constructed case families of tests/zmw_cases.py (ladder, block_edge,
band, tie) on the oracle alone: every class a family exists for is reached, as
the oracle's debug histograms count it, and the oracle's results on them are
pinned by tests/golden/record_cases.json (tools/make_golden.py).

The tables below are the contract of the generators: a change that silently
stops reaching a class fails here, on any machine.  tests/test_gpu_records.py
compares every kernel object with the oracle on the same cases.

What the classes mean for the kernel: a traceback move's row
distance is in the cell record's 3-bit tag for d = 1..4 (M moves); an escape
is decoded as 8 - tag for d = 5..8 on the objects with an 8-row ring (2-5) and
read from the tag plane on the 16-row-ring objects (0-1); rows of one or two
predecessors keep their distances in the row meta, rows of three or four in
the tag plane, rows of more than four -- or with a predecessor beyond the ring
-- in far slot records; records are staged in blocks of 32 rows.
"""
import json
import os

import pytest

from oracle import oracle as o
from tests.zmw_cases import (BAND_DEL, BAND_INS, BAND_M, BAND_OFFSETS, BLOCK_D17_RESIDUES, LADDER_DIST,
                             RECORD_FAMILIES, record_golden_entry)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_cases.json")
STATES = {s: i for i, s in enumerate(o.TB_STATES)}
CLASSES = {c: i for i, c in enumerate(o.TB_CLASSES)}


def _run_family(family):
    """The family through one Poa, single-threaded: the four histograms."""
    cases = RECORD_FAMILIES[family]()
    p = o.Poa()
    with o.counting():
        for reads in cases.values():
            p.poa(reads)
    return cases, o.tb_hist(True), o.band_hist(True), o.tb_events(True), o.tie_hist(True)


@pytest.fixture(scope="module")
def hists():
    return {f: _run_family(f) for f in RECORD_FAMILIES}


def test_case_limits():
    """Seeded and deterministic, small: at most ~700 bases a read and 13 reads
    a case (the six-predecessor ladders need 13)."""
    for f, gen in RECORD_FAMILIES.items():
        a, b = gen(), gen()
        assert a == b, f
        for name, reads in a.items():
            assert 1 <= len(reads) <= 13, (f, name)
            assert max(len(r) for r in reads) <= 730, (f, name)


# ladder: an M move and a D move at every listed distance from a junction row
# of every predecessor-count class
LADDER_TABLE = [(s, c, d) for s in o.TB_STATES for c in o.TB_CLASSES for d in LADDER_DIST]


def test_ladder_reaches_every_class(hists):
    _, tb, _, ev, _ = hists["ladder"]
    by = tb.sum(axis=2)
    missing = [(s, c, d) for s, c, d in LADDER_TABLE if by[STATES[s], CLASSES[c], d] == 0]
    assert not missing, f"ladder_cases() no longer reaches {missing}"
    assert ev["dext_chain"] >= 1 and ev["iext_chain"] >= 1
    # the smallest far rows: five and six predecessors exist
    p = o.Poa()
    degs = {name: (p.poa(reads), p.max_indegree())[1] for name, reads in RECORD_FAMILIES["ladder"]().items()
            if name.startswith("np5+")}
    assert {5, 6} <= set(degs.values()) <= {5, 6, 7}, degs


def test_lead_block_cases_put_rows_without_a_way_back_under_the_skip():
    """lead_block_<n>: a read Z + S (|Z| = n) gives LEAD columns in front of
    the junction, and later reads move over them, in M and in D state, to the
    skip's origin n + 3 rows back."""
    p = o.Poa()
    cases = {k: v for k, v in RECORD_FAMILIES["ladder"]().items() if k.startswith("lead_block_")}
    assert len(cases) == 6
    for name, reads in cases.items():
        n = int(name.rsplit("_", 1)[1])
        with o.counting():
            p.poa(reads)
        by = o.tb_hist().sum(axis=(1, 2))
        assert o.tb_events()["lead"] == 1, name
        assert by[STATES["M"], n + 3] >= 1 and by[STATES["D"], n + 3] >= 1, name


# block_edge: the distance-5 junction (two predecessors) on every residue of a
# 32-row block, M and D; the distance-17 one on residues 0, 1, 31
BLOCK_TABLE = ([(s, 5, r) for s in o.TB_STATES for r in range(32)] +
               [(s, 17, r) for s in o.TB_STATES for r in BLOCK_D17_RESIDUES])


def test_block_edge_reaches_every_residue(hists):
    _, tb, _, _, _ = hists["block_edge"]
    missing = [(s, d, r) for s, d, r in BLOCK_TABLE if tb[STATES[s], CLASSES["np2"], r, d] == 0]
    assert not missing, f"block_edge_cases() no longer reaches (state, distance, row mod 32) {missing}"
    # a distance-5 move leaves the block from residues 0 .. 4, a distance-17 one from 0 and 1
    assert sum(1 for s, d, r in BLOCK_TABLE if s == "M" and r < d) == 5 + 2


# band: every clamp, a partial band, every band-shift bin but >= 64 (no input
# found reaches it: an insertion cannot outrun half a band in one row), LEAD,
# MSRC at j = 0, trailing INS, both chains
BAND_BINS = ("shift_neg", "shift_0", "shift_1", "shift_2", "shift_3_63", "clamp_lo", "clamp_hi", "clamp_short",
             "partial")
BAND_EVENTS = ("lead", "msrc0", "trail_ins", "iext_chain", "dext_chain")


def test_band_reaches_every_class(hists):
    cases, _, band, ev, _ = hists["band"]
    missing = [k for k in BAND_BINS if band[k] == 0] + [k for k in BAND_EVENTS if ev[k] == 0]
    assert not missing, f"band_cases() no longer reaches {missing}"
    want = ([f"ins{n}" for n in BAND_INS] + [f"del{n}" for n in BAND_DEL] +
            [f"m{m}_{g}_graph" for m in BAND_M for g in ("long", "short")] +
            [f"{k}_{a}" for a in BAND_OFFSETS for k in ("inner", "outer")])
    assert not [n for n in want if n not in cases]
    assert BAND_INS == (60, 61, 62, 63, 64, 65, 126, 127, 128, 129, 130, 200)
    assert BAND_DEL == tuple(range(60, 71)) + (128, 129, 130)
    assert BAND_M == (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


# tie: every tie rule of SPEC.md met with equal operands
TIE_BINS = o.TIES


def test_tie_reaches_every_rule(hists):
    cases, _, _, _, tie = hists["tie"]
    missing = [k for k in TIE_BINS if tie[k] == 0]
    assert not missing, f"tie_cases() no longer reaches the tie rules {missing}"
    p = o.Poa()
    # §6 on the split columns: ties go to the smallest base
    T = cases["split_2_2"][0]
    for name, col, want in (("split_2_2", 150, 1), ("split_2_2_2", 90, 1)):
        cns, msa = p.poa(cases[name])
        assert len(cns) == len(T) and cns[col] == want, name
    # cnt[best] == gap keeps the column (>=)
    assert len(p.poa(cases["gap_equals_best_ins"])[0]) == len(T) + 7
    assert len(p.poa(cases["gap_equals_best_del"])[0]) == len(T)
    # §1: N is A
    assert p.poa(cases["only_N"])[0].tolist() == p.poa([r.replace(b"N", b"A") for r in cases["only_N"]])[0].tolist()


@pytest.mark.parametrize("family", list(RECORD_FAMILIES))
def test_oracle_reproduces_golden(family):
    with open(GOLDEN) as f:
        want = json.load(f)["families"][family]
    cases = RECORD_FAMILIES[family]()
    assert sorted(want) == sorted(cases)
    p = o.Poa()
    for name, reads in cases.items():
        assert record_golden_entry(p, reads) == want[name], f"{family}/{name}: the oracle moved"
