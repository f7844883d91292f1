"""The demultiplexer on the device (ccsx_barcode.hip, ccsx_gpu_bc_*) against
tests/barcode_ref.py, field for field: the constructed cases of
tests/barcode_cases.py, every set's in one call; cases alone; a second set on
the same context; a batch cut into several slices; the accuracy case on the
engine's own CCS; and the host program's -d and -D files."""
import os
import random
import subprocess

import pytest

import ccsx_amd as cx
from tests import barcode_cases as bc
from tests import barcode_ref as R
from tests import stage_format as F
from tools.gen_synth import write_subreads

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")


@pytest.fixture(scope="module")
def demux():
    d = cx.Demux(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def constructed(demux):
    """Every constructed case, the cases of one set in one call; the sets in
    turn on one context, so each set follows another with a different B or Wn."""
    got = {}
    before = demux.stats()
    for si, idx in bc.by_set().items():
        demux.set(*bc.SETS[si])
        for i, r in zip(idx, demux.score([bc.CASES[i][2] for i in idx])):
            got[i] = r
    return got, before, demux.stats()


@pytest.mark.parametrize("i", range(len(bc.CASES)), ids=bc.NAMES)
def test_constructed_equals_reference(constructed, i):
    assert constructed[0][i] == bc.reference(i)


def test_constructed_stats(constructed):
    _, before, after = constructed
    d = {k: after[k] - before[k] for k in after}
    nsets = len(bc.by_set())
    assert nsets == len(bc.SETS)
    assert d == dict(zmws=len(bc.CASES), slices=nsets, sets=nsets)


def test_each_case_alone_equals_the_batch(demux, constructed):
    names = ("copy_at_7", "n0", "b96_chunk0_and_chunk2", "mixed_64", "rows48")
    for name in names:
        i = bc.NAMES.index(name)
        _, si, ccs, _ = bc.CASES[i]
        demux.set(*bc.SETS[si])
        assert demux.score([ccs])[0] == constructed[0][i]


def test_second_set_leaves_no_state(demux):
    """A large set with long barcodes, then a small one of short barcodes and
    another window: lanes, chunks and rows of the first must not show."""
    reads = [bc.CASES[bc.NAMES.index(n)][2] for n in ("mixed_64", "b96_last_lane", "copy_at_7", "n1")]
    big = bc.BIG + [bc.MIXED[4]]
    small = [bc.BC[5], bc.BC[2]]
    for barcodes, window in ((big, 256), (small, 40), (big, 256), ([bc.BC[2]], 17)):
        demux.set(barcodes, window)
        assert demux.score(reads) == [R.score(barcodes, r, window) for r in reads]


@pytest.mark.parametrize("name", sorted(bc.REJECTED))
def test_rejected_set_keeps_the_earlier_one(demux, name):
    demux.set(bc.BC, 96)
    read = bc.CASES[0][2]
    want = demux.score([read])
    with pytest.raises(ValueError):
        demux.set(bc.REJECTED[name], 96)
    with pytest.raises(ValueError):
        demux.set(bc.BC, 257)
    assert demux.score([read]) == want == [bc.reference(0)]


def test_no_set_is_an_error():
    d = cx.Demux(0)
    try:
        with pytest.raises(cx.GpuError):
            d.score([b"ACGT"])
    finally:
        d.close()


def test_slices():
    rng = random.Random(5)
    barcodes = bc.BIG[:16]
    reads = []
    for k in range(300):
        body = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 150)))
        reads.append(body if k % 5 == 0 else barcodes[k % 16] + body + R.revcomp(barcodes[(7 * k) % 16]))
    # a read takes 2 x 96 + 44 bytes of the arena: 300 of them ~71 kB
    d = cx.Demux(0, 24_000)
    try:
        d.set(barcodes, 96)
        got = d.score(reads)
        st = d.stats()
    finally:
        d.close()
    assert st["zmws"] == 300 and st["sets"] == 1 and 3 <= st["slices"] <= 8
    assert got == [R.score(barcodes, r, 96) for r in reads]


@pytest.fixture(scope="module")
def accuracy(engine):
    barcodes, pairs, zmws = bc.accuracy_case()
    res = engine.run([cx.prepare(subs) for subs in zmws], cx.MODE_SHRED)
    assert all(status == 0 and ccs for ccs, status, _ in res)
    return barcodes, pairs, zmws, [ccs for ccs, _, _ in res]


def test_accuracy_on_the_engines_ccs(demux, accuracy):
    barcodes, pairs, _, reads = accuracy
    demux.set(barcodes, 96)
    got = demux.score(reads)
    assert demux.kernel_ms > 0
    for (i0, i1), ccs, g in zip(pairs, reads, got):
        assert g == R.score(barcodes, ccs, 96) == cx.barcode_host(barcodes, ccs, 96)
        call = cx.barcode_call(g, [16] * 12, len(ccs))
        assert call == R.call(g, [16] * 12, len(ccs))
        assert call[3], (i0, i1, g, call)
        assert {g[0][0] >> 1, g[1][0] >> 1} == {i0, i1}


@pytest.mark.parametrize("fastq", [False, True])
def test_cli_demux(tmp_path, accuracy, fastq):
    barcodes, pairs, zmws, _ = accuracy
    plain_subs = cx.synth_zmw(20201104, 99, 700, 8)[0]  # a ZMW without barcodes
    fa, bfa = str(tmp_path / "in.fa"), str(tmp_path / "bc.fa")
    write_subreads(fa, zmws[:6] + [plain_subs] + zmws[6:])
    names = [f"bc{1001 + i}" for i in range(12)]
    with open(bfa, "w") as f:
        for nm, b in zip(names, barcodes):
            f.write(f">{nm} sample\n{b.decode()}\n")
    out_b, out_0, dmx, rep = (str(tmp_path / n) for n in ("out_b", "out_0", "demux", "report.tsv"))
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, CCSX_DEV_SHARE="8")
    flags = ["-A", "-j", "2", "-m", "1000"] + (["-q"] if fastq else [])
    for extra, out in ((["-B", bfa, "-d", dmx, "-D", rep], out_b), ([], out_0)):
        r = subprocess.run([BIN] + flags + extra + [fa, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    main = open(out_b, "rb").read()
    assert main == open(out_0, "rb").read()
    recs = F.records(main.decode(), fastq)
    assert len(recs) == 13
    want_d, want_t, rows = F.demux_files(recs, barcodes, names, fastq, R.score, R.call)
    nassigned = 0
    for k, (r, (_, _, _, assigned, _)) in enumerate(rows):
        if k == 6:
            assert not assigned
            continue
        assert assigned
        nassigned += 1
        i0, i1 = pairs[k - (k > 6)]
        assert {r[0][0] >> 1, r[1][0] >> 1} == {i0, i1}
    assert nassigned == 12
    assert open(dmx).read() == want_d
    assert open(rep).read() == want_t
