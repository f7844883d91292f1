"""Per-base consensus qualities, CPU side (SPEC.md §9): the reference's
self-check against the oracle, the two exported host functions and the CLI's
help text.  No GPU."""
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from ccsx_amd.build import BIN

from . import quality_ref as qr
from .zmw_cases import edge_cases, synth

CASES = edge_cases()


@pytest.mark.parametrize("mode", [cx.MODE_SHRED, cx.MODE_PRIMITIVE])
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_matches_oracle_edge_cases(name, mode):
    # reference() asserts CCS (and, shredded, the breakpoint log) against the oracle
    ccs, qual, _ = qr.reference(CASES[name], mode)
    assert len(qual) == len(ccs)
    if ccs:
        q = np.frombuffer(qual, np.uint8)
        assert q.min() >= qr.Q_MIN and q.max() <= qr.Q_MAX


@pytest.mark.parametrize("L,passes", [(5000, 5), (3500, 11)])
def test_reference_matches_oracle_multi_round(L, passes):
    z = synth(3, L, passes)
    ccs, qual, log = qr.reference(z, cx.MODE_SHRED)
    assert len(log) >= 2 and len(qual) == len(ccs) > 0


def test_reference_reaches_both_clamps():
    hi = [n for n in ("many_passes_short", "over_64_reads") if qr.Q_MAX in qr.reference(CASES[n], cx.MODE_PRIMITIVE)[1]]
    lo = [n for n in ("two_segments", "unrelated_reads") if qr.Q_MIN in qr.reference(CASES[n], cx.MODE_PRIMITIVE)[1]]
    assert hi and lo, (hi, lo)


def test_qual_phred_matches_formula():
    for cov in range(131):
        for match in range(cov + 1):
            want = min(max(3 * (2 * match - cov), 2), 93)
            assert cx.qual_phred(match, cov) == want == int(qr.phred(match, cov)), (match, cov)


def test_qual_rq_matches_numpy():
    rng = np.random.default_rng(11)
    assert cx.qual_rq(b"") == 0.0
    for n in (1, 2, 63, 1000, 100000):
        q = rng.integers(0, 94, n, dtype=np.uint8)
        # both sides sum at most 1e5 doubles in [0, 1]: rounding stays far below 1e-12
        assert abs(cx.qual_rq(q) - qr.rq(q.tobytes())) <= 1e-12
    assert abs(cx.qual_rq(bytes([20] * 50)) - 0.99) <= 1e-12


def test_cli_help_lists_q():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=30)
    assert any(line.startswith("-q") for line in r.stdout.splitlines()), r.stdout
