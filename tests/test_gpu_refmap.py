"""The reference mapper on the device (ccsx_ref.hip's vote kernel and the path
variant of ccsx_align.hip's band kernel, ccsx_gpu_ref_*) against
tests/refmap_ref.py: the records and words of the constructed cases of
tests/refmap_cases.py field for field and word for word, every set's in one
call; cases alone; a second set on the same context; a rejected set; no set;
a batch cut into several slices with a read that no slice holds; the
vote-overflow fallback at the smallest table the context accepts; the stats;
the accuracy case on the engine's own CCS; and the host program's -G -g under
tests/cli_batches.py's SPREAD against ccsx_ref_host, byte for byte."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from tests import refmap_cases as rc
from tests import refmap_ref as R
from tests import stage_cases as st
from tests.cli_batches import SPREAD, assert_spread
from tests.test_refmap_host import check_accuracy

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")


def by_set() -> dict:
    out: dict = {}
    for i, c in enumerate(rc.CASES):
        out.setdefault(c[1], []).append(i)
    return out


def same(got, want) -> bool:
    return got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def mapper():
    m = cx.RefMapper(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def constructed(mapper):
    """Every constructed case, the cases of one set in one call; the sets in
    turn on one context, so each set follows another one."""
    got = {}
    before = mapper.stats()
    for si, idx in by_set().items():
        mapper.set(rc.SETS[si])
        for i, r in zip(idx, mapper.map([rc.CASES[i][2] for i in idx])):
            got[i] = r
    return got, before, mapper.stats()


@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.NAMES)
def test_constructed_equals_reference(constructed, i):
    rec, words = constructed[0][i]
    want, want_words = rc.reference(i)
    assert rec == want
    bad = np.flatnonzero(words != want_words)
    assert not len(bad), (bad[:8].tolist(), words[bad[:8]].tolist(), want_words[bad[:8]].tolist())


def test_constructed_stats(constructed):
    _, before, after = constructed
    d = {k: after[k] - before[k] for k in after}
    nsets = len(by_set())
    assert nsets == len(rc.SETS)
    mapped = sum(1 for i in range(len(rc.CASES)) if rc.reference(i)[0][0] >= 0)
    assert d == dict(reads=len(rc.CASES), slices=nsets, sets=nsets, mapped=mapped, overflows=0, host_reads=0)
    assert 0 < mapped < len(rc.CASES)


def test_each_case_alone_equals_the_batch(mapper, constructed):
    for name in ("n0", "n13", "diag_m33", "palindrome", "revcomp_read", "band_first_cells", "band_last_cells", "n_65", "no_hit"):
        i = rc.NAMES.index(name)
        _, si, read, _ = rc.CASES[i]
        mapper.set(rc.SETS[si])
        assert same(mapper.map([read])[0], constructed[0][i]), name
        assert mapper.map([read], words=False)[0] == (constructed[0][i][0], None)
    assert mapper.map([]) == []


def test_second_set_leaves_no_state(mapper):
    """A large set, then a small one whose table is shorter, then the large one
    again: targets, table and directory of the other must not show."""
    reads = [rc.CASES[rc.NAMES.index(n)][2] for n in ("exact", "revcomp_read", "target_13", "occ_64", "n13", "no_hit")]
    for si in (9, 1, 0, 4, 9, 0):
        mapper.set(rc.SETS[si])
        want = [R.record(rc.SETS[si], r) for r in reads]
        assert all(same(g, w) for g, w in zip(mapper.map(reads), want)), si


@pytest.mark.parametrize("name", sorted(rc.REJECTED))
def test_rejected_set_keeps_the_earlier_one(mapper, constructed, name):
    i = rc.NAMES.index("exact")
    mapper.set(rc.SETS[0])
    with pytest.raises(ValueError):
        mapper.set(rc.REJECTED[name])
    assert same(mapper.map([rc.CASES[i][2]])[0], rc.reference(i))


def test_no_set_is_an_error():
    m = cx.RefMapper(0)
    try:
        with pytest.raises(cx.GpuError):
            m.map([b"ACGTACGTACGTACGT"])
        for slots in (0, 32, 96, 8192):
            with pytest.raises(ValueError):
                m.vote_cap(slots)
    finally:
        m.close()


def mixed_reads(n: int, seed: int = 5) -> list:
    """n reads of 0 .. 700 bases: stretches of set 0's targets in either
    strand, with errors, junk ends or all junk."""
    from tests.polish_ref import mutate
    rng = random.Random(seed)
    reads = []
    for k in range(n):
        t = rc.SETS[0][k % 3]
        b = rng.randrange(len(t) - 100)
        s = t[b:b + rng.randrange(0, 600)]
        if k % 4 == 1:
            s = mutate(rng, s, .02, .04, .04)
        if k % 4 == 2:
            s = rc.rnd(1000 + k, rng.randrange(60)) + s + rc.rnd(2000 + k, rng.randrange(60))
        if k % 7 == 6:
            s = rc.rnd(3000 + k, rng.randrange(300))
        reads.append(R.revcomp(s) if k % 2 else s)
    return reads


def test_slices_and_a_read_no_slice_holds():
    """200 mixed reads and one of 3500 bases in an arena of 1 MiB: the set's
    head takes 0.27 MiB, a base 262 bytes, so a slice holds some 2800 bases
    and the long read none; it is mapped on the host inside the call."""
    reads = mixed_reads(200)
    long_read = rc.T0[:1400] + rc.T0[100:1500] + rc.T0[:700]
    reads.insert(77, long_read)
    want = [R.record(rc.SETS[0], r) for r in reads]
    m = cx.RefMapper(0, 1 << 20)
    try:
        m.set(rc.SETS[0])
        got = m.map(reads)
        stats = m.stats()
    finally:
        m.close()
    bad = [k for k, (g, w) in enumerate(zip(got, want)) if not same(g, w)]
    assert not bad, (bad[:8], [(got[k][0], want[k][0]) for k in bad[:3]])
    assert stats["reads"] == 201 and stats["host_reads"] == 1 and stats["overflows"] == 0 and 10 <= stats["slices"] <= 60
    assert stats["mapped"] == sum(1 for r, _ in want if r[0] >= 0) and 100 < stats["mapped"] < 201


def test_vote_overflow_runs_on_the_host():
    """A table of 64 slots: 60 units of the tandem repeat vote for 77
    (target, orientation, bin) keys and overflow it, 3 units and a plain read
    do not; the overflowed read comes from ccsx_ref_host inside the call."""
    reads = [rc.U * 3, rc.U * 60, rc.U[:15], rc.U * 60]
    want = [R.record(rc.SETS[4], r) for r in reads]
    keys = [sum(len(R.seed(q, R.target_codes(rc.SETS[4][0]))) for q in (R.read_codes(r), R.read_codes(R.revcomp(r))))
            for r in reads]
    assert keys[0] <= 64 < keys[1] and keys[2] <= 64, keys
    m = cx.RefMapper(0)
    try:
        m.set(rc.SETS[4])
        m.vote_cap(64)
        got = m.map(reads)
        small = m.stats()
        m.vote_cap(4096)
        again = m.map(reads)
        full = m.stats()
    finally:
        m.close()
    assert all(same(g, w) for g, w in zip(got, want)) and all(same(g, w) for g, w in zip(again, want))
    assert small["overflows"] == 2 and small["host_reads"] == 2 and small["reads"] == 4 and small["mapped"] == 4
    assert full["overflows"] == 2 and full["host_reads"] == 2 and full["reads"] == 8


@pytest.fixture(scope="module")
def accuracy(engine):
    targets, planted, zmws = rc.accuracy_case(rc.ACCURACY_SEED)
    res = engine.run([cx.prepare(subs) for subs in zmws], cx.MODE_SHRED)
    assert all(status == 0 and ccs for ccs, status, _ in res)
    return targets, planted, [ccs for ccs, _, _ in res]


def test_accuracy_on_the_engines_ccs(mapper, accuracy):
    targets, planted, reads = accuracy
    mapper.set(targets)
    got = mapper.map(reads)
    assert mapper.vote_ms > 0 and mapper.band_ms > 0
    rs = cx.RefSet(targets)
    for ccs, g in zip(reads, got):
        assert same(g, R.record(targets, ccs)) and same(g, cx.ref_host(rs, ccs))
    check_accuracy(targets, planted, reads, [g[0] for g in got])


# --- the host program

GROUPS = {"p": ["p"], "B": ["d", "D"], "I": ["i", "S"], "G": ["g"]}
DEFAULT = dict(CCSX_DEV_SHARE="8")
REF_NAMES = [f"ref{k}" for k in range(4)]


@pytest.fixture(scope="module")
def panel():
    """Four targets cut from the stage family's oracle CCS reads: target k is
    bases [100, 500) of the reads of the holes h = k mod 4 (without every 8th
    hole, whose reads stay unmapped or map by a shared adapter only), the odd
    targets reverse-complemented, so their reads map on '-'."""
    _, ccs = st.oracle_ccs()
    ts = [b"", b"", b"", b""]
    for (h, _), c in zip(st.kept(), ccs):
        if h % 8 != 7:
            ts[h % 4] += c[100:500]
    return [R.revcomp(t) if k % 2 else t for k, t in enumerate(ts)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, panel):
    d = tmp_path_factory.mktemp("refmap_in")
    fa, bfa, afa = st.write_inputs(d)
    gfa = str(d / "ref.fa")
    with open(gfa, "w") as f:
        for nm, t in zip(REF_NAMES, panel):
            f.write(f">{nm} panel\n{t.decode()}\n")
    return fa, bfa, afa, gfa


@pytest.fixture(scope="module")
def cli(inputs, tmp_path_factory):
    fa, bfa, afa, gfa = inputs

    def run(groups, fastq, env, extra=()):
        d = tmp_path_factory.mktemp("refmap_run")
        args = ["-A", "-j", "4", "-m", str(st.MIN_TOTAL)] + (["-q"] if fastq else []) + list(extra)
        for g in groups:
            args += {"B": ["-B", bfa], "I": ["-I", afa], "G": ["-G", gfa]}.get(g, [])
            for k in GROUPS[g]:
                args += ["-" + k, str(d / k)]
        r = subprocess.run([BIN] + args + [fa, str(d / "out")], capture_output=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        keys = ["out"] + [k for g in groups for k in GROUPS[g]]
        return {k: open(d / k, "rb").read() for k in keys}, r.stderr.decode(errors="replace")

    return run


def records(main: bytes, fastq: bool) -> list:
    lines = main.decode().split("\n")[:-1]
    step = 4 if fastq else 2
    return [(lines[k][1:].split(" ")[0], lines[k + 1].encode()) for k in range(0, len(lines), step)]


def want_paf(recs, panel, y=50, Y=75, every=8) -> tuple:
    """The -g file of the main output's reads by ccsx_ref_host and
    refmap_ref.paf_line; every 8th read also by refmap_ref.record."""
    rs = cx.RefSet(panel)
    out, nrep = "", 0
    for k, (name, ccs) in enumerate(recs):
        rec, words = cx.ref_host(rs, ccs)
        if k % every == 0:
            assert same((rec, words), R.record(panel, ccs))
        if cx.ref_pass(rec, y, Y):
            out += R.paf_line(name, ccs, rec, words, REF_NAMES[rec[0]], len(panel[rec[0]]))
            nrep += 1
    return out.encode(), nrep


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_cli_map_alone(cli, panel, fastq):
    files, stderr = cli(["G"], fastq, SPREAD)
    assert_spread(stderr)
    plain, _ = cli([], fastq, DEFAULT)
    assert files["out"] == plain["out"]
    recs = records(files["out"], fastq)
    assert len(recs) == st.N and [c for _, c in recs] == list(st.oracle_ccs()[1])
    want, nrep = want_paf(recs, panel)
    assert files["g"] == want
    # both strands, and reads that are not reported
    assert 80 <= nrep < st.N and b"\t-\tref1\t" in want and b"\t+\tref0\t" in want


def test_cli_thresholds(cli, panel):
    files, _ = cli(["G"], False, DEFAULT, extra=["-Y", "100", "-y", "401"])
    want, nrep = want_paf(records(files["out"], False), panel, y=401, Y=100)
    assert files["g"] == want and 0 < nrep < 80


@pytest.fixture(scope="module")
def everything(cli):
    files, stderr = cli(list(GROUPS), True, SPREAD)
    assert_spread(stderr)
    return files


@pytest.mark.parametrize("group", list(GROUPS))
def test_cli_with_the_other_stages(cli, everything, group):
    """-p -B -I -G at once under SPREAD: each file equals the file of a run with
    that option alone (and -q) as one chunk and one batch."""
    alone, _ = cli([group], True, DEFAULT)
    for k in ["out"] + GROUPS[group]:
        assert alone[k], k
        assert everything[k] == alone[k], k


def test_cli_failed_zmw_inside_a_batch(cli, everything):
    """One ZMW fails on the device (the CCSX_FAULT_HOLE test hook) inside its
    batch: the mapper's compacted index is one behind the batch's from there
    on.  The -g file is the full run's minus that hole's line."""
    files, stderr = cli(list(GROUPS), True, dict(SPREAD, CCSX_FAULT_HOLE=str(st.FAULT_HOLE)))
    assert_spread(stderr)
    assert f"synth/{st.FAULT_HOLE}: no CCS" in stderr and "mapper:" not in stderr
    name = b"synth/%d/" % st.FAULT_HOLE
    want = b"".join(ln + b"\n" for ln in everything["g"].split(b"\n")[:-1] if not ln.startswith(name))
    assert want != everything["g"] and files["g"] == want
