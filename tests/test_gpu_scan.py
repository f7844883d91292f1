"""The adapter scanner on the device (ccsx_scan.hip, ccsx_gpu_scan_*) against
tests/scan_ref.py: the hits of the constructed cases of tests/scan_cases.py
field for field, every set's in one call; the bottom rows of the tile-edge and
read-length cases cell for cell (what pins the tiling: hits alone would hide an
error at a column below the threshold); cases alone; a second set on the same
context; a batch cut into several slices; a re-run with the counted capacity;
the host fallback; the accuracy case on the engine's own CCS; and the host
program's -i and -S files."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from tests import scan_cases as sc
from tests import scan_ref as R
from tests import stage_format as F
from tools.gen_synth import write_subreads

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")


@pytest.fixture(scope="module")
def scanner():
    s = cx.Scanner(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def constructed(scanner):
    """Every constructed case, the cases of one set in one call; the sets in
    turn on one context, so each set follows another with a different A, T or
    row count.  The tracked cases' bottom rows come from a second call."""
    got, tracks = {}, {}
    before = scanner.stats()
    for si, idx in sc.by_set().items():
        scanner.set(*sc.SETS[si])
        for i, r in zip(idx, scanner.scan([sc.CASES[i][2] for i in idx])):
            got[i] = r
    after = scanner.stats()
    for si, idx in sc.by_set().items():
        tr = [i for i in idx if sc.NAMES[i] in sc.TRACKED]
        if tr:
            scanner.set(*sc.SETS[si])
            for i, t in zip(tr, scanner.tracks([sc.CASES[i][2] for i in tr])):
                tracks[i] = t
    return got, tracks, before, after


def test_tile_constants_are_the_cases():
    for rows, wu in sc.WU.items():
        assert cx.Scanner.tile(rows) == (sc.TC, wu)
    with pytest.raises(ValueError):
        cx.Scanner.tile(24)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=sc.NAMES)
def test_constructed_equals_reference(constructed, i):
    assert constructed[0][i] == sc.reference(i)


@pytest.mark.parametrize("name", sc.TRACKED)
def test_tracks_equal_reference_cell_for_cell(constructed, name):
    i = sc.NAMES.index(name)
    _, si, ccs, _ = sc.CASES[i]
    want = R.tracks(sc.SETS[si][0], ccs)
    got = constructed[1][i]
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), (bad[:8].tolist(), [(int(got[p, j]), int(want[p, j])) for p, j in bad[:8]])


def test_constructed_stats(constructed):
    _, _, before, after = constructed
    d = {k: after[k] - before[k] for k in after}
    nsets = len(sc.by_set())
    assert nsets == len(sc.SETS)
    assert d["reads"] == len(sc.CASES) and d["sets"] == nsets and d["host_reads"] == 0 and d["candidates"] > 0
    assert d["slices"] == nsets + d["reruns"]


def test_each_case_alone_equals_the_batch(scanner, constructed):
    names = ("tile_ends_r64", "n0", "n_512", "tile_long_span", "last_of_64_reversed", "mixed_lengths", "short_1")
    for name in names:
        i = sc.NAMES.index(name)
        _, si, ccs, _ = sc.CASES[i]
        scanner.set(*sc.SETS[si])
        assert scanner.scan([ccs])[0] == constructed[0][i]


def test_second_set_leaves_no_state(scanner):
    """A large set with long adapters, then a small one of short adapters and
    another threshold: patterns and rows of the first must not show."""
    reads = [sc.CASES[sc.NAMES.index(n)][2] for n in ("mixed_lengths", "kinnex_array", "tile_ends_r16", "n1")]
    big = sc.KINNEX + [sc.AD[64]]
    small = [sc.AD[16], sc.KINNEX[2]]
    for adapters, T in ((big, 75), (small, 90), (big, 75), ([sc.KINNEX[4]], 60)):
        scanner.set(adapters, T)
        assert scanner.scan(reads) == [R.hits(adapters, r, T) for r in reads]


@pytest.mark.parametrize("name", sorted(sc.REJECTED))
def test_rejected_set_keeps_the_earlier_one(scanner, name):
    i = sc.NAMES.index("start_exact")
    scanner.set(*sc.SETS[0])
    read = sc.CASES[i][2]
    want = scanner.scan([read])
    with pytest.raises(ValueError):
        scanner.set(sc.REJECTED[name], 75)
    for T in sc.REJECTED_T:
        with pytest.raises(ValueError):
            scanner.set([sc.AD[64]], T)
    assert scanner.scan([read]) == want == [sc.reference(i)]


def test_no_set_is_an_error():
    s = cx.Scanner(0)
    try:
        with pytest.raises(cx.GpuError):
            s.scan([b"ACGT"])
        with pytest.raises(cx.GpuError):
            s.tracks([b"ACGT"])
    finally:
        s.close()


def test_a_read_past_the_column_field_is_an_error(scanner):
    scanner.set(*sc.SETS[0])
    with pytest.raises(cx.GpuError):
        scanner.scan([b"ACGT", b"A" * (1 << 24)])
    assert scanner.scan([b"ACGT"]) == [[]]


def test_slices():
    rng = random.Random(5)
    adapters = sc.KINNEX[:6]
    reads = []
    for k in range(300):
        body = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 700)))
        reads.append(body if k % 5 == 0 else body + adapters[k % 6] + body[:200] + R.revcomp(adapters[(7 * k) % 6]))
    # a read takes ~1.1 bytes of the arena per base: 300 of them ~200 kB
    s = cx.Scanner(0, 48_000)
    try:
        s.set(adapters)
        got = s.scan(reads)
        st = s.stats()
    finally:
        s.close()
    assert st["reads"] == 300 and st["sets"] == 1 and st["host_reads"] == 0 and 4 <= st["slices"] <= 16
    assert got == [R.hits(adapters, r) for r in reads]


def test_capacity_rerun():
    """40 tandem copies: some 240 candidates against a first buffer of 95
    records; the counted capacity fits the arena, so the slice runs once more."""
    i = sc.NAMES.index("tandem_40")
    s = cx.Scanner(0, 8192)
    try:
        s.set(*sc.SETS[0])
        got = s.scan([sc.CASES[i][2]])
        st = s.stats()
    finally:
        s.close()
    assert st["reruns"] == 1 and st["slices"] == 2 and st["host_reads"] == 0 and st["candidates"] > 95
    assert got == [sc.reference(i)]


def test_host_fallback():
    """A poly-A adapter on a poly-A read: a candidate at nearly every column,
    16 kB of records against an arena of 6 kB; the read is scanned on the host
    inside the call, its neighbours on the device."""
    i = sc.NAMES.index("poly_a")
    plain = sc.CASES[sc.NAMES.index("n1")][2]
    s = cx.Scanner(0, 6144)
    try:
        s.set(*sc.SETS[13])
        got = s.scan([plain, sc.CASES[i][2], plain])
        st = s.stats()
    finally:
        s.close()
    assert st["host_reads"] == 1 and st["reads"] == 3 and st["candidates"] >= 1982
    assert got == [[], sc.reference(i), []]


@pytest.fixture(scope="module")
def accuracy(engine):
    adapters, pairs, zmws = sc.accuracy_case()
    res = engine.run([cx.prepare(subs) for subs in zmws], cx.MODE_SHRED)
    assert all(status == 0 and ccs for ccs, status, _ in res)
    return adapters, pairs, zmws, [ccs for ccs, _, _ in res]


def test_accuracy_on_the_engines_ccs(scanner, accuracy):
    adapters, pairs, _, reads = accuracy
    scanner.set(adapters)
    got = scanner.scan(reads)
    assert scanner.kernel_ms > 0
    for (i, j), ccs, g in zip(pairs, reads, got):
        assert g == R.hits(adapters, ccs) == cx.scan_host(adapters, ccs)
        assert [h[:2] for h in g] == [(i, 0), (j, 1)], g
        pieces = cx.scan_cut(g, len(ccs))
        assert pieces == R.cut(g, len(ccs)) and len(pieces) == 3


@pytest.mark.parametrize("fastq", [False, True])
def test_cli_scan(tmp_path, accuracy, fastq):
    adapters, pairs, zmws, _ = accuracy
    plain_subs = cx.synth_zmw(20201104, 99, 700, 8)[0]  # a ZMW without adapters
    fa, afa = str(tmp_path / "in.fa"), str(tmp_path / "ad.fa")
    write_subreads(fa, zmws[:6] + [plain_subs] + zmws[6:])
    names = [f"ad{k}" for k in range(3)]
    with open(afa, "w") as f:
        for nm, a in zip(names, adapters):
            f.write(f">{nm} adapter\n{a.decode()}\n")
    out_i, out_0, rep, pcs = (str(tmp_path / n) for n in ("out_i", "out_0", "hits.tsv", "pieces"))
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, CCSX_DEV_SHARE="8")
    flags = ["-A", "-j", "2", "-m", "1000"] + (["-q"] if fastq else [])
    for extra, out in ((["-I", afa, "-i", rep, "-S", pcs], out_i), ([], out_0)):
        r = subprocess.run([BIN] + flags + extra + [fa, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    main = open(out_i, "rb").read()
    assert main == open(out_0, "rb").read()
    recs = F.records(main.decode(), fastq)
    assert len(recs) == 13
    want_t, want_p, found = F.scan_files(recs, adapters, names, fastq, R.hits, R.cut)
    assert [len(h) for h in found] == [0 if k == 6 else 2 for k in range(13)]
    assert open(rep).read() == want_t
    assert open(pcs).read() == want_p
