"""Per-strand consensus, CPU side (SPEC.md §14): the reference's self-check
against the oracle and every invariant of the definition on every case in both
modes (against tests/quality_ref.py and tests/pileup_ref.py), what the
constructed cases must show, the exported symbols and Engine methods, and the
CLI's -b option as far as it goes without a device.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from ccsx_amd.build import BIN

from . import pileup_ref as pu
from . import quality_ref as qr
from . import strand_ref as sr
from .strand_cases import PRIVATE_AT, PRIVATE_INS, all_cases, private_insertion_reads
from .zmw_cases import synth

CASES = all_cases()
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]


def check_invariants(z, mode: int) -> sr.StrandRef:
    """The invariants of SPEC.md §14 on the reference's strand consensuses of z."""
    r = sr.reference(z, mode)
    rev = pu.flags(z)
    qccs, qual, _ = qr.reference(z, mode)
    pccs, recs, *_ = pu.reference(z, mode)
    assert r.ccs == qccs == pccs
    ncols = len(r.calls)
    # a joint column always has a spanning read
    assert (r.cov.sum(1) >= 1).all()
    for s in (0, 1):
        assert len(r.seq[s]) == len(r.qual[s])
        assert len(r.seq[s]) <= r.pushed[s] and len(r.seq[s]) <= ncols
        assert len(r.seq[s]) == int(((r.calls[:, s] >= 0) & (r.calls[:, s] < 4)).sum())
        if len(r.qual[s]):
            assert r.qual[s].min() >= qr.Q_MIN and r.qual[s].max() <= qr.Q_MAX
    # one strand only: its consensus is the CCS and its qualities are §9's, byte for byte
    for s in (0, 1):
        if (rev == s).all():
            assert r.seq[s] == r.ccs and r.qual[s].tobytes() == qual
            assert len(r.seq[1 - s]) == 0 and r.pushed[1 - s] == 0
    # at every CCS base the column's call is the call of its pileup record
    clean = ~(recs == 255).any(1)
    assert len(r.base_col) == len(recs)
    for p in np.nonzero(clean)[0]:
        for s in (0, 1):
            assert int(r.calls[r.base_col[p], s]) == cx.pileup_call(recs[p], s) == pu.call(recs[p], s)
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_invariants(name, mode):
    # reference() asserts its CCS and breakpoint log against the oracle's
    check_invariants(CASES[name], mode)


@pytest.mark.parametrize("L,passes", [(5000, 5), (3500, 11)])
def test_reference_invariants_multi_round(L, passes):
    z = synth(3, L, passes)
    assert z.rev is not None and z.rev.any() and not z.rev.all()
    assert len(sr.reference(z, cx.MODE_SHRED).log) >= 2
    for mode in MODES:
        r = check_invariants(z, mode)
        assert len(r.seq[0]) and len(r.seq[1])


@pytest.mark.parametrize("mode", MODES)
def test_one_strand_only(mode):
    for name, s in (("no_flags", 0), ("all_zero_flags", 0), ("all_one_flags", 1), ("reverse_only", 1)):
        r = sr.reference(CASES[name], mode)
        _, qual, _ = qr.reference(CASES[name], mode)
        assert r.seq[s] == r.ccs and r.qual[s].tobytes() == qual and len(r.ccs) > 0
        assert r.seq[1 - s] == b"" and len(r.qual[1 - s]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_exact_copies_on_both_strands(mode):
    r = sr.reference(CASES["exact_both_strands"], mode)
    assert r.seq[0] == r.seq[1] == r.ccs and len(r.ccs) == 350


@pytest.mark.parametrize("mode", MODES)
def test_heteroduplex(mode):
    """split_2_2: reads G, C, G, C at column 150.  With the strands alternating
    (`heteroduplex`, flags [0, 1, 0, 1]) each strand is unanimous there and the
    two consensuses differ in exactly that position, each equal to its own
    reads.  With flags [0, 0, 1, 1] (`heteroduplex_same_strand`) each strand
    holds one G and one C: both tie to the smallest base, as the CCS does, and
    the consensuses are equal (tests/test_pileup_host.py: no discordant site)."""
    z = CASES["heteroduplex"]
    r = sr.reference(z, mode)
    f, v = r.seq
    assert len(f) == len(v) == len(r.ccs) == 300
    assert [p for p in range(300) if f[p] != v[p]] == [150]
    segs = [z.seqs[int(o):int(o) + int(ln)] for o, ln in zip(z.offs, z.lens)]
    assert f == segs[0] == segs[2] and v == segs[1] == segs[3]
    assert f[150:151] == b"G" and v[150:151] == b"C"
    r = sr.reference(CASES["heteroduplex_same_strand"], mode)
    assert r.seq[0] == r.seq[1] == r.ccs and r.ccs[150:151] == b"C"


@pytest.mark.parametrize("mode", MODES)
def test_strand_private_insertion(mode):
    reads = private_insertion_reads()
    r = sr.reference(CASES["private_insertion"], mode)
    assert r.ccs == reads[0]
    assert len(r.seq[1]) == len(r.ccs) + PRIVATE_INS and len(r.seq[0]) == len(r.ccs)
    assert r.seq[0] == reads[0] and r.seq[1] == reads[1]
    assert r.seq[1][:PRIVATE_AT] + r.seq[1][PRIVATE_AT + PRIVATE_INS:] == r.ccs


@pytest.mark.parametrize("mode", MODES)
def test_strand_deletion(mode):
    # the ten bases only the forward reads carry (gap = best in the joint column: kept in the CCS)
    r = sr.reference(CASES["strand_deletion"], mode)
    assert r.seq[0] == r.ccs and len(r.seq[1]) == len(r.ccs) - 10


def test_carry_cases_reach_the_round_edge():
    """The carry_g* cases: at least two rounds, and a strand base in the
    gap-consensus columns behind the first round's last CCS base."""
    from .pileup_cases import CARRY_CASES
    for name in CARRY_CASES:
        r = sr.reference(CASES[name], cx.MODE_SHRED)
        assert len(r.log) >= 2 and r.carry >= 1, name
        assert len(r.seq[1]) > len(r.ccs) == len(r.seq[0])


def test_fastq_record_layout():
    r = sr.reference(CASES["private_insertion"], cx.MODE_SHRED)
    rev = pu.flags(CASES["private_insertion"])
    fa = sr.fasta("m/7/ccs", r, False, rev, cx.qual_rq).split("\n")
    assert fa[0] == ">m/7/ccs/fwd" and fa[2] == ">m/7/ccs/rev" and len(fa[3]) == 420 and fa[4] == ""
    fq = sr.fasta("m/7/ccs", r, True, rev, cx.qual_rq).split("\n")
    assert fq[0].startswith("@m/7/ccs/fwd np=3 rq=0.") and fq[4].startswith("@m/7/ccs/rev np=2 rq=0.")
    assert fq[2] == fq[6] == "+" and len(fq[7]) == 420
    one = sr.reference(CASES["all_one_flags"], cx.MODE_SHRED)
    assert sr.fasta("m/8/ccs", one, False, np.ones(4), cx.qual_rq).startswith(">m/8/ccs/rev\n")


def test_library_exports_and_engine_methods():
    L = cx.lib()
    assert hasattr(L, "ccsx_gpu_set_by_strand") and hasattr(L, "ccsx_gpu_by_strand")
    assert callable(getattr(cx.Engine, "set_by_strand", None)) and callable(getattr(cx.Engine, "by_strand", None))


def test_cli_help_lists_b():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=30)
    assert any(line.startswith("-b") for line in r.stdout.splitlines()), r.stdout


def test_cli_takes_b_before_any_device(tmp_path):
    """-b FILE is an option of its own: a path that cannot be opened is refused
    with the other outputs' message, before a device is asked for."""
    fa = str(tmp_path / "in.fa")
    open(fa, "w").write(">m/1/0_4\nACGT\n")
    bad = str(tmp_path / "no_such_dir" / "strands.fa")
    r = subprocess.run([BIN, "-A", "-b", bad, fa, str(tmp_path / "out.fa")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Cannot open file for write!" in r.stderr and "Usage" not in r.stdout
    assert not os.path.exists(bad)
