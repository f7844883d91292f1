"""Per-base consensus qualities from the GPU engine (SPEC.md §9): bases
against the oracle, quality bytes byte-for-byte against tests/quality_ref.py
(the definition is integer: no tolerance), through every path the CCS bytes
take -- every kernel object, the HBM-read instance, full-capacity re-runs,
multi-slice runs, submit / collect, and the CLI's -q."""
import os
import random
import subprocess

import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from oracle.oracle import prepare as oracle_prepare
from tests.cli_batches import SPREAD, assert_spread
from tests import quality_ref as qr
from tests.zmw_cases import edge_cases, raw, synth
from tools.gen_synth import records, write, write_bam

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]


@pytest.fixture
def qengine(engine):
    """The shared engine with quality on; quality, forced configurations and
    test hooks are switched back off afterwards."""
    engine.set_quality(True)
    try:
        yield engine
    finally:
        engine.set_quality(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)


def _assert_exact(zs, mode, got, quals):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        rccs, rqual, _ = qr.reference(z, mode)
        assert rccs == ccs
        assert quals[i] == rqual, f"ZMW {i}: qualities differ from the reference"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.quality(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(qengine, mode):
    """n < 3, an empty segment, nw = 2 (70 reads), both clamps, window growth
    without a breakpoint, ragged spans (cov < n)."""
    cases = edge_cases()
    zs = [cases[k] for k in sorted(cases)]
    _check(qengine, zs, mode)
    allq = b"".join(qr.reference(z, mode)[1] for z in zs)
    assert qr.Q_MIN in allq and qr.Q_MAX in allq


@pytest.mark.parametrize("L,passes", [(5000, 5), (9000, 3), (3500, 11)])
def test_shredded_multi_round(qengine, L, passes):
    """Several shredding rounds: only columns [0, i) of each round are emitted
    (colrate 60 below ten reads, 80 from ten on)."""
    zs = [synth(8100 + h, L, passes) for h in range(4)]
    assert all(len(qr.reference(z, cx.MODE_SHRED)[2]) >= 2 for z in zs)
    _check(qengine, zs, cx.MODE_SHRED)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(qengine, cfg, mode):
    zs = [synth(8200 + h, 3000, 8) for h in range(6)]
    qengine.set_kernel_cfg(cfg)
    _check(qengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert qengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_long_reads_primitive(qengine):
    """-P pushes the 20 kb segments whole: a 20 kb LDS read buffer, beyond the
    int16 ring's 16,256 bases (the LDS instance still: its buffer holds reads
    up to 100 kb; the HBM-read instance is test_hbm_read_instance's)."""
    _check(qengine, [synth(8300, 20000, 5)], cx.MODE_PRIMITIVE)


def test_hbm_read_instance(qengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (nw = 66 mask words)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    before = qengine.hbm_launches()
    _check(qengine, [raw(segs)], cx.MODE_SHRED)
    assert qengine.hbm_launches() - before >= 1


@pytest.mark.parametrize("hook", ["tight_out", "tight_rows"])
def test_full_capacity_rerun(qengine, hook):
    """ZMWs that outgrow a tight cap are re-run with full caps, by ccsx_gpu_run
    and inside ccsx_gpu_collect: their qualities come from the re-run."""
    zs = [synth(8400 + h, 1500, 6) for h in range(4)] + [cx.prepare([b"ACGTACGTAC"] * 5)]
    if hook == "tight_out":
        qengine.set_tight_out(64)
    else:
        qengine.set_tight_rows(600)
    before = qengine.rerun_count()
    _check(qengine, zs, cx.MODE_SHRED)
    assert qengine.rerun_count() - before >= 4
    s = qengine.submit(zs, cx.MODE_SHRED)
    got = qengine.collect(s)
    assert qengine.rerun_count() - before >= 8
    _assert_exact(zs, cx.MODE_SHRED, got, [qengine.quality(i, s) for i in range(len(zs))])


def test_multi_slice_run(qengine):
    """12 ZMWs in at least 3 slices: qualities gathered in input order."""
    zs = [synth(8500 + h, 1200 + 300 * (h % 4), 5 + h % 3) for h in range(12)]
    tot = sum(qengine.zmw_bytes(z) for z in zs)
    qengine.set_slot_budget(int(tot / 3.5))
    st0 = qengine.run_stats()
    _check(qengine, zs, cx.MODE_SHRED)
    assert qengine.run_stats()["slices"] - st0["slices"] >= 3


def test_submit_collect_both_slots(qengine):
    zs1 = [synth(8600 + h, 2500, 6) for h in range(5)]
    zs2 = [synth(8650 + h, 1500, 9) for h in range(7)]
    s1 = qengine.submit(zs1)
    s2 = qengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = qengine.collect(s1)
    g2 = qengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [qengine.quality(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [qengine.quality(i, s2) for i in range(len(zs2))])
    with pytest.raises(cx.GpuError):
        qengine.quality(len(zs1), s1)
    # a batch submitted, or run, with quality off has none
    qengine.set_quality(False)
    s3 = qengine.submit(zs1)
    qengine.collect(s3)
    with pytest.raises(cx.GpuError):
        qengine.quality(0, s3)
    qengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError):
        qengine.quality(0)


def test_stage_launch_fetch(qengine):
    zs = [synth(8700 + h, 2000, 6) for h in range(3)]
    qengine.stage(zs, cx.MODE_SHRED)
    qengine.launch(cx.MODE_SHRED)
    got = qengine.fetch()
    _assert_exact(zs, cx.MODE_SHRED, got, [qengine.quality(i) for i in range(len(zs))])


def _outcap(z):
    # ccsx_layout.h zcaps, tight caps: min(S + 16, 2 x longest segment + 1,024)
    lens = [int(x) for x in z.lens]
    return min(sum(lens) + 16, 2 * max(lens) + 1024)


# ccsx_gpu_zmw_bytes (shredded, -P) and ccsx_gpu_staged_bytes of the three ZMWs
# below as the library computed them before it knew of qualities
OFF_BYTES = {"zmw_bytes": [(5692042, 5692042), (3761272, 3761272), (342326, 342326)], "staged": 9795064}


def test_off_means_off(engine):
    """Quality off: the sizes are what they were without the feature; on adds
    exactly one more output slab per ZMW; the CCS bytes are the same."""
    zs = [synth(8800, 3000, 6), synth(8801, 1500, 12), synth(8802, 60, 9)]
    try:
        engine.set_quality(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_quality(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_quality(False)
    assert off == OFF_BYTES["zmw_bytes"] and staged_off == OFF_BYTES["staged"]
    caps = [_outcap(z) for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in caps]
    assert staged_on - staged_off == sum(caps)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _fastq(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    recs = []
    for i in range(0, len(lines) - 1, 4):
        head, seq, plus, q = lines[i:i + 4]
        assert head[:1] == b"@" and plus == b"+" and len(q) == len(seq)
        name, np_, rq = head[1:].split(b" ")
        assert np_.startswith(b"np=") and rq.startswith(b"rq=")
        recs.append((name, seq, q, int(np_[3:]), float(rq[3:])))
    return recs


def _fasta(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def _cli_check(tmp_path, src, args, mode, env=None, is_bam=False, exclude=(), err=None):
    """`args src` with and without -q: same bases; qualities, np and rq from
    the reference on the oracle's preparation of the same records.  err: a list
    that receives the stderr of the run with -q."""
    fq, fa_out = str(tmp_path / "out.fq"), str(tmp_path / "out.fa")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(env or {}, CCSX_DEV_SHARE="8")
    for extra, out in ((["-q"], fq), ([], fa_out)):
        r = subprocess.run([BIN] + args + extra + [src, out], capture_output=True, timeout=300,
                           env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if err is not None and extra:
            err.append(r.stderr)
    got = _fastq(fq)
    assert [(n, s) for n, s, _, _, _ in got] == _fasta(fa_out)
    want = []
    for movie, hole, subs in cx.read_zmws(src, is_bam):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000) or hole in exclude:
            continue
        p = oracle_prepare(subs)
        ccs, qual, _ = qr.reference(p, mode)
        if ccs:
            want.append((b"%s/%s/ccs" % (movie.encode(), hole.encode()), ccs, qual, len(p.lens)))
    assert len(got) == len(want)
    for (name, seq, q, np_, rq), (wname, wccs, wqual, wnp) in zip(got, want):
        assert name == wname and seq == wccs and np_ == wnp
        assert q == bytes(x + 33 for x in wqual), name
        assert abs(rq - qr.rq(wqual)) <= 1e-6
    return len(got)


@pytest.mark.parametrize("mode_flag,mode", [([], 0), (["-P"], 1)])
def test_cli_fastq(tmp_path, mode_flag, mode):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    # a ZMW with too few subreads and one outside -m are filtered out
    with open(fa, "ab") as f:
        f.write(b">synth/900/0_10\nACGTACGTAC\n")
        subs, _ = cx.synth_zmw(20201104, 901, 300, 8)
        for i, s in enumerate(subs):
            f.write(b">synth/901/%d_%d\n%s\n" % (i, i + 1, s))
    assert _cli_check(tmp_path, fa, ["-A", "-j", "2", "-X", "3,5"] + mode_flag, mode, exclude={"3", "5"}) == 10


def test_cli_fastq_async_contexts_order(tmp_path):
    """Pipelined submit / collect on two contexts, three batches per context
    and chunk: records stay in input order, each with its own qualities. The run is
    tests/cli_batches.py's SPREAD, and must have spread: several chunks, several
    batches per chunk, several contexts, slots reused.  (Until CCSX_MIN_BATCH
    existed this test asked for 2 contexts x 3 batches and, 300 ZMWs being
    fewer than two batches of the 256-ZMW floor, ran one batch on one context.)"""
    fa = str(tmp_path / "in.fa")
    write(fa, 300, 1000, 6)
    err = []
    assert _cli_check(tmp_path, fa, ["-A", "-j", "4"], 0, env=SPREAD, err=err) == 300
    assert_spread(err[0])


def test_cli_fastq_bam_input(tmp_path):
    bam = str(tmp_path / "in.bam")
    write_bam(bam, records(20, 1500, 7, hole0=100))
    assert _cli_check(tmp_path, bam, ["-j", "4"], 0, is_bam=True) == 20
