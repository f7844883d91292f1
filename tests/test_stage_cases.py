"""tests/stage_cases.py's family does what it was built for, on the reference
alone (no GPU): on the oracle's CCS of its ZMWs, ccsx_barcode_host +
ccsx_barcode_call assign most reads to exactly the pair they were built with
and leave the random-ended ones unassigned, ccsx_scan_host finds adapters in
two thirds of the reads and none in the rest, and no two ZMWs share a report
line, a hit list or a CCS length -- so a record attached to the wrong ZMW
shows in every file the host program writes from it.  And
tests/cli_batches.py's check of a run's spread is not vacuous."""
import pytest

import ccsx_amd as cx
from tests import barcode_ref as BR
from tests import scan_ref as SR
from tests import stage_cases as st
from tests import stage_format as F
from tests.cli_batches import assert_spread, batch_lines, spread


@pytest.fixture(scope="module")
def reads():
    ps, ccs = st.oracle_ccs()
    assert len(ccs) == st.N and all(ccs)
    return [h for h, _ in st.kept()], ccs


def test_filters_and_chunks():
    holes = [h for h, _ in st.kept()]
    assert holes == list(range(st.N))
    every = [h for h, _ in st.family()[2]]
    assert len(every) == st.N + 2 and every.index(st.FEW_HOLE) == 38 and every.index(st.SHORT_HOLE) == 72
    # SPREAD's chunks of 16, 64 and the rest: min(12, n / 4) batches each
    assert [min(12, n // 4) for n in (16, 64, st.N - 80)] == [4, 12, 4]


def test_pieces_are_far_apart():
    bcs, ads, _ = st.family()
    rc = BR.revcomp
    for k, b in enumerate(bcs):
        assert len(b) == 16 and BR.edit_distance(b, rc(b)) >= 7
        assert all(BR.edit_distance(b, o) >= 7 and BR.edit_distance(b, rc(o)) >= 7 for o in bcs[:k])
    for k, a in enumerate(ads):
        assert len(a) == 25 and SR.edit_distance(a, rc(a)) >= 9
        assert all(SR.edit_distance(a, o) >= 9 and SR.edit_distance(a, rc(o)) >= 9 for o in ads[:k])


def test_demultiplexing_counts(reads):
    holes, ccs = reads
    bcs = st.family()[0]
    exact = unassigned = 0
    for h, c in zip(holes, ccs):
        r = cx.barcode_host(bcs, c, 96)
        assigned = cx.barcode_call(r, [16] * 12, len(c))[3]
        unassigned += not assigned
        pr = st.pair_of(h)
        exact += bool(assigned and pr and (r[0][0], r[1][0]) == (2 * pr[0], 2 * pr[1]))
    assert exact >= 70 and unassigned >= 8, (exact, unassigned)


def test_scan_counts(reads):
    holes, ccs = reads
    ads = st.family()[1]
    nhits = [len(cx.scan_host(ads, c)) for c in ccs]
    assert sum(1 for n in nhits if n >= 1) >= 56 and sum(1 for n in nhits if n == 0) >= 24, nhits
    # the layouts as built: none, one, two in opposite orientations
    for h, c in zip(holes, ccs):
        got = [(a, o) for a, o, _, _, _ in cx.scan_host(ads, c)]
        assert got == [(a, o) for a, o, _ in st.adapters_of(h)], h


def test_no_two_zmws_alike(reads):
    holes, ccs = reads
    bcs, ads, _ = st.family()
    assert len({len(c) for c in ccs}) == st.N
    recs = [(f"synth/{h}/ccs", c.decode(), None) for h, c in zip(holes, ccs)]
    _, report, _ = F.demux_files(recs, bcs, st.BC_NAMES, False, cx.barcode_host, cx.barcode_call)
    rows = [ln.split("\t", 1)[1] for ln in report.split("\n")[1:-1]]
    assert len(rows) == st.N == len(set(rows))
    hits, _, found = F.scan_files(recs, ads, st.AD_NAMES, False, cx.scan_host, cx.scan_cut)
    per = {}
    for ln in hits.split("\n")[1:-1]:
        name, rest = ln.split("\t", 1)
        per.setdefault(name, []).append(rest)
    assert len(per) == sum(1 for f in found if f) and len({tuple(v) for v in per.values()}) == len(per)


def test_fault_hole_is_inside_its_batch():
    """The hole the failed-ZMW run names is neither first nor last in its
    batch's order on the device, so the stages' compacted index differs from
    the batch index for every ZMW after it."""
    batch, pos = st.fault_batch(cx)
    assert 16 <= st.FAULT_HOLE < 80 and batch[pos] == st.FAULT_HOLE
    assert 0 < pos < len(batch) - 1, (batch, pos)


def _timing(batches):
    return "".join(f"[ccsx] chunk {c} batch of {n} ZMWs on context {w}: 10-20 ms\n" for c, n, w in batches)


def test_assert_spread_is_not_vacuous():
    """What a 300-ZMW run prints with the 256-ZMW floor (chunks of 16, 64 and
    220 ZMWs: n / 256 = 0, one batch each) fails the check; SPREAD's cut of
    the same input passes; so do neither one context nor two chunks."""
    one_batch_each = _timing([(0, 16, 0), (1, 64, 1), (2, 220, 0)])
    assert batch_lines(one_batch_each) == [(0, 16, 0), (1, 64, 1), (2, 220, 0)]
    assert spread(one_batch_each) == dict(chunks=3, chunk_batches=1, contexts=2, ctx_batches=2)
    with pytest.raises(AssertionError):
        assert_spread(one_batch_each)
    with pytest.raises(AssertionError):
        assert_spread(_timing([(0, 300, 0)]))   # the default first chunk: everything in one batch
    with pytest.raises(AssertionError):
        assert_spread(b"")
    cut = [(0, 4, b % 4) for b in range(4)] + [(1, 5, b % 4) for b in range(12)] + [(2, 18, b % 4) for b in range(12)]
    assert_spread(_timing(cut).encode())
    with pytest.raises(AssertionError):
        assert_spread(_timing([(c, n, 0) for c, n, _ in cut]))
    assert_spread(_timing([(c, n, 0) for c, n, _ in cut]), single=True)
    assert_spread(_timing([(c, 5, 0) for c in range(3) for _ in range(3)]), single=True)
    with pytest.raises(AssertionError):
        assert_spread(_timing(cut), single=True)
    with pytest.raises(AssertionError):
        assert_spread(_timing(cut[:16]))
