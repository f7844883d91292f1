"""Per-pass alignment statistics, CPU side (SPEC.md §10): the reference's
self-check against the oracle, the invariants of the definition and its anchor
values on the edge cases, the exported host function and the CLI's help text.
No GPU."""
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from ccsx_amd.build import BIN

from . import pass_ref as pr
from .zmw_cases import edge_cases, synth

CASES = edge_cases()
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]

# sums over the ZMW's reads of [match, mismatch, ins, del]
ANCHORS = {
    ("short_reads_60bp", cx.MODE_SHRED): [349, 5, 13, 7],
    ("short_reads_60bp", cx.MODE_PRIMITIVE): [349, 5, 13, 7],
    ("over_64_reads", cx.MODE_SHRED): [46595, 262, 3721, 2068],
    ("over_64_reads", cx.MODE_PRIMITIVE): [46595, 262, 3721, 2068],
    ("with_empty_segment", cx.MODE_SHRED): [13531, 208, 669, 517],
    ("with_empty_segment", cx.MODE_PRIMITIVE): [13531, 208, 669, 517],
    ("homopolymers", cx.MODE_SHRED): [23571, 445, 1347, 540],
    ("homopolymers", cx.MODE_PRIMITIVE): [23569, 445, 1349, 540],
}


def check_invariants(z, mode):
    """The three invariants of SPEC §10 on the reference's records of z."""
    ccs, rec, _ = pr.reference(z, mode)
    r = rec.astype(np.int64)
    lens = np.asarray([int(x) for x in z.lens], np.int64)
    assert r.shape == (len(lens), 6)
    # 1. every base of the segment is consumed exactly once, over all rounds
    assert (r[:, pr.MATCH] + r[:, pr.MISMATCH] + r[:, pr.INS] == lens).all()
    # 2. the spanned consensus bases lie inside [cbeg, cend) (equal in -P: one call)
    spanned = r[:, pr.MATCH] + r[:, pr.MISMATCH] + r[:, pr.DEL]
    width = r[:, pr.CEND] - r[:, pr.CBEG]
    assert (spanned <= width).all()
    if mode == cx.MODE_PRIMITIVE:
        assert (spanned == width).all()
    # 3. the stretch lies in the CCS
    assert (r[:, pr.CEND] <= len(ccs)).all() and (r[:, pr.CBEG] <= r[:, pr.CEND]).all()
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_invariants_edge_cases(name, mode):
    # reference() asserts CCS (and, shredded, the breakpoint log) against the oracle
    r = check_invariants(CASES[name], mode)
    want = ANCHORS.get((name, mode))
    if want is not None:
        assert r[:, :4].sum(0).tolist() == want


def test_anchor_cases_exist():
    assert {n for n, _ in ANCHORS} <= set(CASES)


def test_empty_segment_record_is_zero():
    z = CASES["with_empty_segment"]
    empty = [k for k, ln in enumerate(z.lens) if int(ln) == 0]
    assert empty
    for mode in MODES:
        _, rec, _ = pr.reference(z, mode)
        assert not rec[empty].any()


@pytest.mark.parametrize("L,passes", [(5000, 5), (9000, 3), (3500, 11)])
def test_reference_invariants_multi_round(L, passes):
    z = synth(3, L, passes)
    assert len(pr.reference(z, cx.MODE_SHRED)[2]) >= 2
    for mode in MODES:
        check_invariants(z, mode)


def test_pass_identity():
    recs = [(0, 0, 0, 0, 0, 0), (10, 0, 0, 0, 3, 13), (90, 4, 3, 3, 0, 97), (0, 5, 0, 0, 1, 6), (1, 1, 1, 0, 7, 9),
            (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 0, 0)]
    want = [0.0, 1.0, 0.9, 0.0, 1 / 3, 0.25]
    for rec, w in zip(recs, want):
        got = cx.pass_identity(rec)
        assert got == pr.identity(rec)  # the same division of the same integers, in double
        assert abs(got - w) <= 1e-15
    assert cx.pass_identity(np.asarray(recs[2], np.uint32)) == 0.9


def test_cli_help_lists_r():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=30)
    assert any(line.startswith("-r") for line in r.stdout.splitlines()), r.stdout
