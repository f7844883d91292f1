"""Per-base consensus kinetics from the GPU engine (SPEC.md §13): bases against
the oracle, records byte-for-byte against tests/kinetics_ref.py (the definition
is integer: no tolerance), through every path the CCS bytes take -- every kernel
object, the HBM-read instance, full-capacity re-runs, multi-slice runs, submit /
collect, stage / launch / fetch, and the CLI's -k."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from oracle.oracle import prepare as oracle_prepare
from oracle.oracle import prepare_segments as oracle_prepare_segments
from tests.cli_batches import SPREAD, assert_spread
from tests import basemap_ref as br
from tests import kinetics_ref as kr
from tests import pass_ref as pr
from tests import pileup_ref as pu
from tests import quality_ref as qr
from tests.kinetics_cases import alternating, patterns, tagged_records, with_kin, write_bam
from tests.zmw_cases import edge_cases, raw, shred_cases, synth
from tools.gen_synth import records

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]


@pytest.fixture
def kengine(engine):
    """The shared engine with the kinetics on; it, the other features, forced
    configurations and test hooks are switched back off afterwards."""
    engine.set_kinetics(True)
    try:
        yield engine
    finally:
        engine.set_kinetics(False)
        engine.set_pileup(False)
        engine.set_base_map(False)
        engine.set_pass_stats(False)
        engine.set_quality(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)


def _assert_exact(zs, mode, got, kins):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        rccs, recs, _, _ = kr.reference(z, mode)
        assert rccs == ccs
        g = kins[i]
        assert g.dtype == np.uint8 and g.shape == (len(ccs), 8)
        bad = np.nonzero((g != recs).any(1))[0]
        assert len(bad) == 0, f"ZMW {i}: {len(bad)} records differ from the reference, first at {bad[0]}: " \
                              f"{g[bad[0]].tolist()} != {recs[bad[0]].tolist()}"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.kinetics(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(kengine, mode):
    """n < 3, an empty segment, nw = 2 (70 reads), ragged spans; strands
    alternating in push order, planes over all 256 codes."""
    cases = edge_cases()
    _check(kengine, [with_kin(cases[k], alternating(len(cases[k].lens)), seed=j) for j, k in enumerate(sorted(cases))], mode)


EDGES = ["n63", "n64", "n65", "n128", "n129", "final_2943", "final_2944", "final_2945", "copies_14000", "indel", "two_reads",
         "empty_segment"]


@pytest.mark.parametrize("name", EDGES)
def test_mask_word_and_column_edges(kengine, name):
    """Read counts around the 64-read mask words (sums crossing words), final
    rounds of 64 m - 1 / 64 m / 64 m + 1 columns, seven rounds, cursors after an
    insertion and a deletion; every strand pattern that fits."""
    z = raw(shred_cases()[name])
    zs = [with_kin(z, rev, seed=3 + j) for j, (_, rev) in enumerate(sorted(patterns(len(z.lens)).items()))]
    _check(kengine, zs, cx.MODE_SHRED)


def test_saturation_and_missing_planes(kengine):
    """300 x 150 bases all forward: n saturates at 255 and the means are exact
    over 300; in a batch of three the middle ZMW comes without planes."""
    rng = np.random.default_rng(3)
    ins = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))
    z = with_kin(raw([ins] * 300), None, seed=17)
    a, b, c = with_kin(synth(9200, 1500, 6), seed=1), with_kin(synth(9201, 1500, 6), planes=False), \
        with_kin(synth(9202, 1500, 6), seed=2)
    for mode in MODES:
        _check(kengine, [z, a, b, c], mode)
        k = kengine.kinetics(0)
        assert (k[:, 2] == 255).all() and not k[:, 3:].any()
        assert (kr.reference(z, mode)[2][:, 0] == 300).all()
        assert len(kengine.kinetics(2)) > 1000 and not kengine.kinetics(2).any()
        assert kengine.kinetics(1)[:, [2, 5]].all(1).sum() > 1000


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(kengine, cfg, mode):
    zs = [with_kin(synth(9300 + h, 3000, 8), seed=h) for h in range(6)]
    kengine.set_kernel_cfg(cfg)
    _check(kengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert kengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_over_64_reads_on_every_kernel_object(kengine, cfg):
    a, b = edge_cases()["over_64_reads"], raw(shred_cases()["n129"])
    zs = [with_kin(a, alternating(len(a.lens)), seed=5), with_kin(b, alternating(len(b.lens)), seed=6)]
    kengine.set_kernel_cfg(cfg)
    _check(kengine, zs, cx.MODE_SHRED)
    assert kengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_long_reads_primitive(kengine):
    """-P pushes the 20 kb segments whole: the planes are indexed over the whole
    segments (the records of the CCS's last bases come from bases near 20,000)."""
    z = with_kin(synth(9400, 20000, 5), seed=9)
    _check(kengine, [z], cx.MODE_PRIMITIVE)
    assert len(kengine.kinetics(0)) > 19000 and kengine.kinetics(0)[-100:, [2, 5]].any()


def test_hbm_read_instance(kengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (66 mask words per column)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    z = with_kin(raw(segs), alternating(4200), seed=4)
    before = kengine.hbm_launches()
    _check(kengine, [z], cx.MODE_SHRED)
    assert kengine.hbm_launches() - before >= 1
    # (2,100 reads per strand: both counts saturate at the insert's 60 bases; a
    # stray column a few mutated reads win may follow them)
    assert (kengine.kinetics(0)[:, [2, 5]] == 255).all(1).sum() >= 60


@pytest.mark.parametrize("hook", ["tight_out", "tight_rows"])
def test_full_capacity_rerun(kengine, hook):
    """ZMWs that outgrow a tight cap are re-run with full caps, by ccsx_gpu_run
    and inside ccsx_gpu_collect: their records come from the re-run."""
    zs = [with_kin(synth(9500 + h, 1500, 6), seed=h) for h in range(4)] + [with_kin(cx.prepare([b"ACGTACGTAC"] * 5), seed=8)]
    if hook == "tight_out":
        kengine.set_tight_out(64)
    else:
        kengine.set_tight_rows(600)
    before = kengine.rerun_count()
    _check(kengine, zs, cx.MODE_SHRED)
    assert kengine.rerun_count() - before >= 4
    s = kengine.submit(zs, cx.MODE_SHRED)
    got = kengine.collect(s)
    assert kengine.rerun_count() - before >= 8
    _assert_exact(zs, cx.MODE_SHRED, got, [kengine.kinetics(i, s) for i in range(len(zs))])


def test_multi_slice_run(kengine):
    """12 ZMWs in at least 3 slices: records gathered in input order."""
    zs = [with_kin(synth(9600 + h, 1200 + 300 * (h % 4), 5 + h % 3), seed=h) for h in range(12)]
    tot = sum(kengine.zmw_bytes(z) for z in zs)
    kengine.set_slot_budget(int(tot / 3.5))
    st0 = kengine.run_stats()
    _check(kengine, zs, cx.MODE_SHRED)
    assert kengine.run_stats()["slices"] - st0["slices"] >= 3


def test_submit_collect_both_slots(kengine):
    zs1 = [with_kin(synth(9700 + h, 2500, 6), seed=h) for h in range(5)]
    zs2 = [with_kin(synth(9750 + h, 1500, 9), seed=h) for h in range(7)]
    s1 = kengine.submit(zs1)
    with pytest.raises(cx.GpuError):  # not collected yet
        kengine.kinetics(0, s1)
    s2 = kengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = kengine.collect(s1)
    g2 = kengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [kengine.kinetics(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [kengine.kinetics(i, s2) for i in range(len(zs2))])
    with pytest.raises(cx.GpuError):
        kengine.kinetics(len(zs1), s1)
    # a batch submitted, or run, with the feature off has none
    kengine.set_kinetics(False)
    s3 = kengine.submit(zs1)
    kengine.collect(s3)
    with pytest.raises(cx.GpuError):
        kengine.kinetics(0, s3)
    kengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError):
        kengine.kinetics(0)


def test_stage_launch_twice_fetch(kengine):
    """A staged slice launched twice: every record is written once per launch
    and the partial sums of the second mask word start from word 0's store, so
    the second launch leaves the same plane."""
    b = raw(shred_cases()["n129"])
    zs = [with_kin(synth(9800 + h, 2000, 6), seed=h) for h in range(3)] + [with_kin(synth(9810, 5000, 5), seed=4),
                                                                         with_kin(b, alternating(129), seed=5)]
    kengine.stage(zs, cx.MODE_SHRED)
    kengine.launch(cx.MODE_SHRED)
    got = kengine.fetch()
    first = [kengine.kinetics(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, first)
    kengine.launch(cx.MODE_SHRED)
    got = kengine.fetch()
    second = [kengine.kinetics(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, second)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("mode", MODES)
def test_all_five_features(kengine, mode):
    """Quality, pass statistics, the map, the pileup and the kinetics in one
    run, each against its own reference; the CCS and the other four outputs are
    byte-equal with the kinetics on and off."""
    e = edge_cases()
    zs = [with_kin(synth(9900 + h, 2500, 7), seed=h) for h in range(3)] + \
        [with_kin(e["ragged_lengths"], alternating(8), seed=7), with_kin(e["over_64_reads"], alternating(70), seed=8)]
    for on in (True, False):
        kengine.set_kinetics(on)
        kengine.set_quality(True)
        kengine.set_pass_stats(True)
        kengine.set_base_map(True)
        kengine.set_pileup(True)
        got = kengine.run(zs, mode)
        if on:
            _assert_exact(zs, mode, got, [kengine.kinetics(i) for i in range(len(zs))])
        else:
            with pytest.raises(cx.GpuError):
                kengine.kinetics(0)
        others = []
        for i, z in enumerate(zs):
            qual, rec, maps, pile = kengine.quality(i), kengine.pass_stats(i), kengine.base_map(i), kengine.pileup(i)
            assert qual == qr.reference(z, mode)[1], f"ZMW {i}: qualities differ from the reference"
            assert np.array_equal(rec, pr.reference(z, mode)[1]), f"ZMW {i}: pass records differ from the reference"
            for g, w in zip(maps, br.reference(z, mode)[1]):
                assert np.array_equal(g, w), f"ZMW {i}: map differs from the reference"
            assert np.array_equal(pile, pu.reference(z, mode)[1]), f"ZMW {i}: pileup differs from the reference"
            others.append((got[i][0], qual, rec.tobytes(), [m.tobytes() for m in maps], pile.tobytes()))
        if on:
            with_on = others
            # the GPU's own records agree: fwd n + rev n = the pileup's count of the CCS base
            for i in range(len(zs)):
                k, p = kengine.kinetics(i).astype(np.int64), kengine.pileup(i)
                ok = ~(p == 255).any(1) & (k[:, 2] < 255) & (k[:, 5] < 255)
                pp = p.astype(np.int64)
                own = (pp[:, :4] + pp[:, 6:10])[np.arange(len(k)), [b"ACGT".index(c) for c in got[i][0]]]
                assert ((k[:, 2] + k[:, 5]) == own)[ok].all()
        else:
            assert others == with_on
    # the kinetics alone: independent of the others
    kengine.set_kinetics(True)
    kengine.set_quality(False)
    kengine.set_pass_stats(False)
    kengine.set_base_map(False)
    kengine.set_pileup(False)
    _check(kengine, zs[:1], mode)
    with pytest.raises(cx.GpuError):
        kengine.base_map(0)


def _sizes(z, shred: bool):
    """ccsx_layout.h zcaps / zlayout (tight caps) and ccsx_gpu.cpp zmw_bytes,
    restated: the device bytes of one ZMW with every optional output off."""
    lens = [int(x) for x in z.lens]
    S, lmax, n = sum(lens), max(lens), len(lens)
    hi = max(int(o) + ln for o, ln in zip(z.offs, lens))
    a256 = lambda x: (x + 255) & ~255  # noqa: E731
    lw = min(lmax, 4096) if shred and lmax > 4096 else lmax
    rcap, ecap = S + 16, S + n + 16
    r = 3 * lw + 4096
    if r < S:
        rcap = r + 16
        ecap = 2 * rcap
    scap = rcap // 32 + 64
    lcap, nw = lmax + 16, max((n + 63) // 64, 1)
    wcap = rcap // 16 + 64
    outcap = min(S + 16, 2 * lmax + 1024)
    sizes = [rcap, rcap * nw * 8, (rcap + 1) * 4, ecap * 4] * 2
    sizes += [rcap * 4, rcap, rcap * 4, rcap * 128, rcap * 128, scap * (128 * 8 + 16), rcap * 8]
    sizes += [lcap * 4, lcap * 4, lcap * 4, lcap, lcap * 4, (rcap + 1) * 4, rcap + 1, rcap * 4, (rcap + 1) * 4]
    sizes += [rcap * 4, rcap, rcap * nw * 8, (rcap + 1) * 4] + [n * 4] * 6
    ext = a256(a256(a256(wcap * 128 * 4) + ((lcap + 15) // 16 + 2) * 4) + n * 4)
    total = sum(a256(x) for x in sizes) + a256(ext)
    return total + hi + outcap + n * 8 + 88 + 32, outcap, total  # (88: sizeof(ZmwDesc))


def test_sizes(engine):
    """Kinetics off: the sizes are what the layout gives without any optional
    plane (computed from the formula, not recorded); on adds exactly 8 x the
    output slab + 2 x the pushed bases + a byte per segment; the CCS is the same."""
    zs = [with_kin(synth(9950, 3000, 6), seed=1), with_kin(synth(9951, 1500, 12), seed=2), with_kin(synth(9952, 60, 9), seed=3)]
    try:
        engine.set_kinetics(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_kinetics(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_kinetics(False)
    assert off == [(_sizes(z, True)[0], _sizes(z, False)[0]) for z in zs]
    hi = [max(int(o) + int(ln) for o, ln in zip(z.offs, z.lens)) for z in zs]
    assert staged_off == sum(_sizes(z, True)[2] + h + _sizes(z, True)[1] for z, h in zip(zs, hi))
    add = [8 * _sizes(z, True)[1] + 2 * int(sum(z.lens)) + len(z.lens) for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in add]
    assert staged_on - staged_off == sum(add)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _tagged_bam(path, nzmw, L, passes, hole0=0, sub=b"C", drop_pw=()):
    """A BAM of synthetic ZMWs whose subreads carry seeded ip / pw arrays (sub);
    the ZMWs at the indices in drop_pw have one subread without pw."""
    recs, _ = tagged_records(list(records(nzmw, L, passes, hole0=hole0)), seed=hole0 + 1, sub=sub)
    holes = sorted({int(r[0].split(b"/")[1]) for r in recs})
    for j in drop_pw:
        k = next(x for x, r in enumerate(recs) if int(r[0].split(b"/")[1]) == holes[j]) + 1
        name, seq, aux = recs[k]
        recs[k] = (name, seq, aux[:aux.index(b"snBf")])  # (ip stays, pw and what follows go)
    write_bam(path, recs)


def _cli_check(tmp_path, bam, args, mode, env=None, sub_qual=False, stderr=None):
    """`args bam` with and without -k: the same CCS file; the SAM rebuilt from
    the reference on the oracle's preparation, strand flags and the planes.
    stderr: a list that receives the stderr of the run with -k."""
    out_k, out_0, sam = str(tmp_path / "out_k"), str(tmp_path / "out_0"), str(tmp_path / "kin.sam")
    env = dict(os.environ, **dict(env or {}, CCSX_DEV_SHARE="8"))
    err = b""
    for extra, out in ((["-k", sam], out_k), ([], out_0)):
        r = subprocess.run([BIN] + args + extra + [bam, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        err = err or r.stderr
    if stderr is not None:
        stderr.append(err)
    assert open(out_k, "rb").read() == open(out_0, "rb").read()
    want, nline, nnone = "@HD\tVN:1.6\tSO:unknown\n", 0, 0
    for movie, hole, subs, ipd, pw in cx.read_zmws(bam, True, kinetics=True):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        p = oracle_prepare(subs)
        _, _, revs = oracle_prepare_segments(subs)
        z = cx.prepare(subs, ipd, pw) if ipd is not None else cx.prepare(subs)
        assert z.seqs == p.seqs and z.offs.tolist() == list(p.offs) and z.rev.tolist() == list(revs)
        ccs = kr.reference(z, mode)[0]
        if not ccs:
            continue
        qual = qr.reference(z, mode)[1] if sub_qual else None
        want += kr.sam_line(f"{movie}/{hole}/ccs", z, mode, qual, cx.qual_rq(qual) if sub_qual else None)
        nline += 1
        nnone += ipd is None
    assert open(sam).read() == want
    assert f"{nnone} ZMWs without kinetics".encode() in err
    return nline, nnone


@pytest.mark.parametrize("flags,mode", [([], 0), (["-P"], 1), (["-q", "-r", "-a", "-s"], 0)])
def test_cli_kinetics(tmp_path, flags, mode):
    bam = str(tmp_path / "in.bam")
    _tagged_bam(bam, 12, 1500, 7)
    flags = [x for f in flags for x in ([f, str(tmp_path / ("side" + f))] if f in ("-r", "-a", "-s") else [f])]
    assert _cli_check(tmp_path, bam, ["-j", "2"] + flags, mode, sub_qual="-q" in flags) == (12, 0)


def test_cli_kinetics_async_contexts_order(tmp_path):
    """Pipelined submit / collect on two contexts, three batches per context
    and chunk: the lines stay in input order, each ZMW with its own arrays. The run is
    tests/cli_batches.py's SPREAD, and must have spread: several chunks, several
    batches per chunk, several contexts, slots reused.  (Until CCSX_MIN_BATCH
    existed this test asked for 2 contexts x 3 batches and, 300 ZMWs being
    fewer than two batches of the 256-ZMW floor, ran one batch on one context.)"""
    bam = str(tmp_path / "in.bam")
    _tagged_bam(bam, 300, 1000, 6)
    err = []
    assert _cli_check(tmp_path, bam, ["-j", "4"], 0, env=SPREAD, stderr=err) == (300, 0)
    assert_spread(err[0])


def test_cli_frames_and_missing_pw(tmp_path):
    """B:S frames are encoded on the host; a ZMW with a subread lacking pw gets
    its line without the arrays and is counted on stderr."""
    bam = str(tmp_path / "in.bam")
    _tagged_bam(bam, 6, 1500, 7, sub=b"S", drop_pw=(2,))
    assert _cli_check(tmp_path, bam, ["-j", "2"], 0) == (6, 1)


def test_cli_refuses_fasta_input(tmp_path):
    r = subprocess.run([BIN, "-A", "-k", str(tmp_path / "k.sam"), str(tmp_path / "none.fa"), str(tmp_path / "out")],
                       capture_output=True, timeout=60)
    assert r.returncode == 1 and b"-k needs BAM input" in r.stderr
    assert not os.path.exists(tmp_path / "k.sam") and not os.path.exists(tmp_path / "out")
