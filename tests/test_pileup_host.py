"""Per-base strand pileup, CPU side (SPEC.md §12): the reference's self-check
against the oracle and every invariant of the definition on every case in both
modes (against tests/quality_ref.py, tests/pass_ref.py and tests/basemap_ref.py),
what the constructed cases must show, the exported ccsx_pileup_call against the
Python statement of the strand call, prepare()'s strand flags, and the CLI's
help text.  No GPU."""
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from ccsx_amd.build import BIN

from . import basemap_ref as br
from . import pass_ref as pr
from . import pileup_ref as pu
from . import quality_ref as qr
from .pileup_cases import CARRY_CASES, CARRY_FIRST_ROUND, all_cases, with_rev
from .zmw_cases import synth

CASES = all_cases()
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
MULTI = [(5000, 5), (9000, 3), (3500, 11)]
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def check_invariants(z, mode: int):
    """The invariants of SPEC.md §12 on the reference's records of z."""
    ccs, recs, tail, log, _ = pu.reference(z, mode)
    rev = pu.flags(z)
    assert recs.shape == (len(ccs), 12)
    if getattr(z, "rev", None) is None:
        assert not recs[:, pu.REV:].any()
    qccs, qual, _ = qr.reference(z, mode)
    pccs, st, _ = pr.reference(z, mode)
    bccs, maps = br.reference(z, mode)
    assert ccs == qccs == pccs == bccs
    r = recs.astype(np.int64)
    both = r[:, :6] + r[:, 6:]
    clean = ~(recs == 255).any(1)
    base = np.array([CODE[b] for b in ccs], np.int64)
    # per position and strand: the map entries of that strand's segments
    al = np.zeros((2, len(ccs)), np.int64)
    ins = np.zeros((2, len(ccs) + 1), np.int64)
    for k, m in enumerate(maps):
        w = m.astype(np.int64)
        off, isin = w & br.OFFSET, (w & br.INS) != 0
        al[rev[k]] += np.bincount(off[~isin], minlength=len(ccs))
        ins[rev[k]] += np.bincount(off[isin], minlength=len(ccs) + 1)
    for p in np.nonzero(clean)[0]:
        assert pu.call(recs[p], 2) == base[p]
        assert qr.phred(both[p, base[p]], both[p, :5].sum()) == qual[p]
        for s, o in ((0, pu.FWD), (1, pu.REV)):
            assert r[p, o:o + 4].sum() == al[s, p]
            assert r[p, o + pu.INS] == ins[s, p]
    if clean.all():
        sti = st.astype(np.int64)
        assert both[:, :4].sum() == (sti[:, pr.MATCH] + sti[:, pr.MISMATCH]).sum()
        assert both[np.arange(len(ccs)), base].sum() == sti[:, pr.MATCH].sum()
        assert both[:, pu.INS].sum() + tail == sti[:, pr.INS].sum()
        assert tail == ins[:, len(ccs)].sum()
    return ccs, recs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_invariants(name, mode):
    # reference() asserts its CCS and breakpoint log against the oracle's
    _, recs = check_invariants(CASES[name], mode)
    for rec in np.unique(recs, axis=0):
        for strand in (0, 1, 2):
            assert cx.pileup_call(rec, strand) == pu.call(rec, strand)


@pytest.mark.parametrize("L,passes", MULTI)
def test_reference_invariants_multi_round(L, passes):
    z = synth(3, L, passes)
    assert z.rev is not None and len(z.rev) == len(z.lens)
    assert len(pu.reference(z, cx.MODE_SHRED)[3]) >= 2
    for mode in MODES:
        check_invariants(z, mode)


@pytest.mark.parametrize("mode", MODES)
def test_heteroduplex(mode):
    ccs, recs, *_ = pu.reference(CASES["heteroduplex"], mode)
    assert pu.sites(recs) == [(150, 2, 1)] and ccs[150:151] == b"C"
    assert recs[150].tolist() == [0, 0, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0]
    assert pu.sites(pu.reference(CASES["heteroduplex_same_strand"], mode)[1]) == []


@pytest.mark.parametrize("mode", MODES)
def test_strand_deletion(mode):
    _, recs, *_ = pu.reference(CASES["strand_deletion"], mode)
    s = pu.sites(recs)
    assert len(s) == 10 and [p for p, _, _ in s] == list(range(s[0][0], s[0][0] + 10))
    assert all(f < 4 and v == 4 for _, f, v in s)


@pytest.mark.parametrize("name", CARRY_CASES)
def test_carry_across_rounds(name):
    z = CASES[name]
    g = int(name.split("_")[1][1:])
    reads = 2 if name.endswith("two_reads") else 1
    ccs, recs, tail, log, seen = pu.reference(z, cx.MODE_SHRED)
    assert log[0] == CARRY_FIRST_ROUND[g] and len(log) >= 2
    # the round's last g emitted columns are gap-consensus columns: the first
    # CCS base of round 2 carries their bases
    assert seen == g * reads
    p = log[0][0] - g  # the CCS bases round 1 emitted
    r = recs[p].astype(int)
    assert r[pu.FWD + pu.INS] + r[pu.REV + pu.INS] == g * reads
    # (reads 1 and 3 are reverse by the alternating flags)
    assert r[pu.REV + pu.INS] == g * reads


def test_edge_case_carries():
    # a later change of the inputs must not empty the carry tests silently
    assert pu.reference(CASES["lowercase_and_N"], cx.MODE_SHRED)[4] == 1


@pytest.mark.parametrize("mode", MODES)
def test_no_flags_and_one_strand(mode):
    _, recs, *_ = pu.reference(CASES["no_flags"], mode)
    assert not recs[:, pu.REV:].any() and recs[:, :pu.REV].any()
    _, recs, *_ = pu.reference(CASES["reverse_only"], mode)
    assert not recs[:, :pu.REV].any()
    assert all(pu.call(r, 0) == -1 for r in recs) and pu.sites(recs) == []


@pytest.mark.parametrize("mode", MODES)
def test_saturation(mode):
    _, alt, *_ = pu.reference(CASES["saturation_alternating"], mode)
    _, fwd, *_ = pu.reference(CASES["saturation_forward"], mode)
    assert not (alt == 255).any() and alt.max() == 150
    assert (fwd == 255).any() and not fwd[:, pu.REV:].any()
    # the forward-only counts are the two strands' sums, clamped
    both = alt[:, :6].astype(int) + alt[:, 6:]
    assert (np.minimum(both, 255) == fwd[:, :6]).all()


HAND = [
    ([0] * 12, (-1, -1, -1)),
    # a tie goes to the smallest base
    ([0, 3, 3, 0, 0, 0, 0, 0, 2, 2, 0, 9], (1, 2, 2)),
    # cnt = gap keeps the base, one less gives the gap
    ([2, 0, 0, 0, 2, 0, 0, 0, 0, 1, 2, 0], (0, 4, 4)),
    # gap only
    ([0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 7], (4, -1, 4)),
    # ins alone is no evidence
    ([0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 5], (-1, -1, -1)),
    ([255] * 12, (0, 0, 0)),
    ([0, 0, 0, 255, 255, 0, 255, 0, 0, 0, 0, 255], (3, 0, 0)),
]


@pytest.mark.parametrize("rec,want", HAND)
def test_pileup_call_hand_written(rec, want):
    assert tuple(pu.call(rec, s) for s in (0, 1, 2)) == want
    assert tuple(cx.pileup_call(np.asarray(rec, np.uint8), s) for s in (0, 1, 2)) == want
    assert cx.pileup_call(np.asarray(rec, np.uint8), 3) == -1
    assert cx.lib().ccsx_pileup_call(None, 0) == -1


def test_prepare_keeps_the_strand_flags():
    for hole, L, passes in ((1, 800, 6), (2, 600, 9), (3, 1500, 4)):
        subs, _ = cx.synth_zmw(20201104, hole, L, passes)
        z = cx.prepare(subs)
        offs, lens, rev = cx.prepare_segments(subs)
        assert (z.offs == offs).all() and (z.lens == lens).all()
        assert z.rev.dtype == np.uint8 and (z.rev == rev).all() and rev.any()
    # the field is optional
    z3 = cx.Prepared(z.seqs, z.offs, z.lens)
    assert z3.rev is None and with_rev(z3, None).rev is None


def test_cli_help_lists_s():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=30)
    assert any(line.startswith("-s") for line in r.stdout.splitlines()), r.stdout
