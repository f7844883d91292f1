"""Per-base strand pileup from the GPU engine (SPEC.md §12): bases against the
oracle, records byte-for-byte against tests/pileup_ref.py (the definition is
integer: no tolerance), through every path the CCS bytes take -- every kernel
object, the HBM-read instance, full-capacity re-runs, multi-slice runs, submit /
collect, stage / launch / fetch, and the CLI's -s."""
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
from tests import pass_ref as pr
from tests import pileup_ref as pu
from tests import quality_ref as qr
from tests.pileup_cases import CARRY_CASES, alternating, constructed, edge, with_rev
from tests.zmw_cases import raw, synth
from tools.gen_synth import records, write, write_bam

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]


@pytest.fixture
def pengine(engine):
    """The shared engine with the pileup on; it, the other features, forced
    configurations and test hooks are switched back off afterwards."""
    engine.set_pileup(True)
    try:
        yield engine
    finally:
        engine.set_pileup(False)
        engine.set_base_map(False)
        engine.set_pass_stats(False)
        engine.set_quality(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)


def _assert_exact(zs, mode, got, piles):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        rccs, recs, *_ = pu.reference(z, mode)
        assert rccs == ccs
        g = piles[i]
        assert g.dtype == np.uint8 and g.shape == (len(ccs), 12)
        bad = np.nonzero((g != recs).any(1))[0]
        assert len(bad) == 0, f"ZMW {i}: {len(bad)} records differ from the reference, first at {bad[0]}: " \
                              f"{g[bad[0]].tolist()} != {recs[bad[0]].tolist()}"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.pileup(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(pengine, mode):
    """n < 3, an empty segment, nw = 2 (70 reads), ragged spans (cov < n),
    window growth without a breakpoint; strands alternating in push order."""
    cases = edge()
    _check(pengine, [cases[k] for k in sorted(cases)], mode)


@pytest.mark.parametrize("mode", MODES)
def test_constructed_cases(pengine, mode):
    """Heteroduplex, strand deletion, the carry across rounds, no flags, one
    strand only, nw = 5 with and without saturated fields."""
    cases = constructed()
    names = sorted(cases)
    _check(pengine, [cases[k] for k in names], mode)
    het = pengine.pileup(names.index("heteroduplex"))
    assert pu.sites(het) == [(150, 2, 1)]
    assert not pengine.pileup(names.index("no_flags"))[:, pu.REV:].any()
    assert (pengine.pileup(names.index("saturation_forward")) == 255).any()


@pytest.mark.parametrize("L,passes", [(5000, 5), (9000, 3), (3500, 11)])
def test_shredded_multi_round(pengine, L, passes):
    """Several shredding rounds: the records run over the whole CCS, the
    dropped bases of a round's last columns go to the next round's first base."""
    zs = [synth(8100 + h, L, passes) for h in range(4)]
    assert all(z.rev is not None and z.rev.any() for z in zs)
    assert all(len(pu.reference(z, cx.MODE_SHRED)[3]) >= 2 for z in zs)
    _check(pengine, zs, cx.MODE_SHRED)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(pengine, cfg, mode):
    zs = [synth(8200 + h, 3000, 8) for h in range(6)]
    pengine.set_kernel_cfg(cfg)
    _check(pengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert pengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_carry_on_every_kernel_object(pengine, cfg):
    cases = constructed()
    zs = [cases[k] for k in CARRY_CASES] + [edge()["lowercase_and_N"]]
    assert all(pu.reference(z, cx.MODE_SHRED)[4] >= 1 for z in zs)
    pengine.set_kernel_cfg(cfg)
    _check(pengine, zs, cx.MODE_SHRED)
    assert pengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_long_reads_primitive(pengine):
    """-P pushes the 20 kb segments whole: a 20 kb LDS read buffer, beyond the
    int16 ring's 16,256 bases."""
    _check(pengine, [synth(8300, 20000, 5)], cx.MODE_PRIMITIVE)


def test_hbm_read_instance(pengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (nw = 66 strand words); 2,100
    reads per strand saturate the counts."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    z = with_rev(raw(segs), alternating(4200))
    before = pengine.hbm_launches()
    _check(pengine, [z], cx.MODE_SHRED)
    assert pengine.hbm_launches() - before >= 1
    assert (pengine.pileup(0) == 255).any()


@pytest.mark.parametrize("hook", ["tight_out", "tight_rows"])
def test_full_capacity_rerun(pengine, hook):
    """ZMWs that outgrow a tight cap are re-run with full caps, by ccsx_gpu_run
    and inside ccsx_gpu_collect: their records come from the re-run."""
    zs = [synth(8400 + h, 1500, 6) for h in range(4)] + [cx.prepare([b"ACGTACGTAC"] * 5)]
    if hook == "tight_out":
        pengine.set_tight_out(64)
    else:
        pengine.set_tight_rows(600)
    before = pengine.rerun_count()
    _check(pengine, zs, cx.MODE_SHRED)
    assert pengine.rerun_count() - before >= 4
    s = pengine.submit(zs, cx.MODE_SHRED)
    got = pengine.collect(s)
    assert pengine.rerun_count() - before >= 8
    _assert_exact(zs, cx.MODE_SHRED, got, [pengine.pileup(i, s) for i in range(len(zs))])


def test_multi_slice_run(pengine):
    """12 ZMWs in at least 3 slices: records gathered in input order."""
    zs = [synth(8500 + h, 1200 + 300 * (h % 4), 5 + h % 3) for h in range(12)]
    tot = sum(pengine.zmw_bytes(z) for z in zs)
    pengine.set_slot_budget(int(tot / 3.5))
    st0 = pengine.run_stats()
    _check(pengine, zs, cx.MODE_SHRED)
    assert pengine.run_stats()["slices"] - st0["slices"] >= 3


def test_submit_collect_both_slots(pengine):
    zs1 = [synth(8600 + h, 2500, 6) for h in range(5)]
    zs2 = [synth(8650 + h, 1500, 9) for h in range(7)]
    s1 = pengine.submit(zs1)
    with pytest.raises(cx.GpuError):  # not collected yet
        pengine.pileup(0, s1)
    s2 = pengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = pengine.collect(s1)
    g2 = pengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [pengine.pileup(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [pengine.pileup(i, s2) for i in range(len(zs2))])
    with pytest.raises(cx.GpuError):
        pengine.pileup(len(zs1), s1)
    # a batch submitted, or run, with the feature off has none
    pengine.set_pileup(False)
    s3 = pengine.submit(zs1)
    pengine.collect(s3)
    with pytest.raises(cx.GpuError):
        pengine.pileup(0, s3)
    pengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError):
        pengine.pileup(0)


def test_stage_launch_twice_fetch(pengine):
    """A staged slice launched twice: every record is written once per launch,
    the second launch leaves the same plane."""
    zs = [synth(8700 + h, 2000, 6) for h in range(3)] + [synth(8710, 5000, 5)]
    pengine.stage(zs, cx.MODE_SHRED)
    pengine.launch(cx.MODE_SHRED)
    got = pengine.fetch()
    first = [pengine.pileup(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, first)
    pengine.launch(cx.MODE_SHRED)
    got = pengine.fetch()
    second = [pengine.pileup(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, second)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("mode", MODES)
def test_all_four_features(pengine, mode):
    """Quality, pass statistics, the map and the pileup in one run: every plane
    exact, and the GPU's own map and pass records satisfy SPEC.md §12's
    cross-checks against the GPU's pileup."""
    zs = [synth(8800 + h, 2500, 7) for h in range(3)] + [edge()["ragged_lengths"]]
    pengine.set_quality(True)
    pengine.set_pass_stats(True)
    pengine.set_base_map(True)
    got = pengine.run(zs, mode)
    piles = [pengine.pileup(i) for i in range(len(zs))]
    _assert_exact(zs, mode, got, piles)
    for i, z in enumerate(zs):
        ccs = got[i][0]
        qual = pengine.quality(i)
        assert qual == qr.reference(z, mode)[1], f"ZMW {i}: qualities differ from the reference"
        rec = pengine.pass_stats(i)
        assert np.array_equal(rec, pr.reference(z, mode)[1]), f"ZMW {i}: pass records differ from the reference"
        maps = pengine.base_map(i)
        for g, w in zip(maps, br.reference(z, mode)[1]):
            assert np.array_equal(g, w), f"ZMW {i}: map differs from the reference"
        # (SPEC.md §12: the cross-checks hold wherever no field of the record is saturated)
        r = piles[i].astype(np.int64)
        ok = ~(piles[i] == 255).any(1)
        assert ok.sum() > len(ccs) // 2
        both = r[:, :6] + r[:, 6:]
        base = np.array([b"ACGT".index(b) for b in ccs], np.int64)
        sti = rec.astype(np.int64)
        own = both[np.arange(len(ccs)), base]
        assert (qr.phred(own, both[:, :5].sum(1)) == np.frombuffer(qual, np.uint8))[ok].all()
        if ok.all():
            assert both[:, :4].sum() == (sti[:, pr.MATCH] + sti[:, pr.MISMATCH]).sum()
            assert own.sum() == sti[:, pr.MATCH].sum()
        rev = pu.flags(z)
        al = np.zeros((2, len(ccs)), np.int64)
        ins = np.zeros((2, len(ccs) + 1), np.int64)
        for k, m in enumerate(maps):
            w = m.astype(np.int64)
            off, isin = w & br.OFFSET, (w & br.INS) != 0
            al[rev[k]] += np.bincount(off[~isin], minlength=len(ccs))
            ins[rev[k]] += np.bincount(off[isin], minlength=len(ccs) + 1)
        for s, o in ((0, pu.FWD), (1, pu.REV)):
            assert (r[:, o:o + 4].sum(1) == al[s])[ok].all()
            assert (r[:, o + pu.INS] == ins[s, :len(ccs)])[ok].all()
        if ok.all():
            assert both[:, pu.INS].sum() + ins[:, len(ccs)].sum() == sti[:, pr.INS].sum()
    # the pileup alone: independent of the others
    pengine.set_quality(False)
    pengine.set_pass_stats(False)
    pengine.set_base_map(False)
    _check(pengine, zs[:1], mode)
    with pytest.raises(cx.GpuError):
        pengine.base_map(0)


def _outcap(z):
    # ccsx_layout.h zcaps, tight caps: min(S + 16, 2 x longest segment + 1,024)
    lens = [int(x) for x in z.lens]
    return min(sum(lens) + 16, 2 * max(lens) + 1024)


# ccsx_gpu_zmw_bytes (shredded, -P) and ccsx_gpu_staged_bytes of the three ZMWs
# below as the library computed them before it knew of any optional plane
OFF_BYTES = {"zmw_bytes": [(5692042, 5692042), (3761272, 3761272), (342326, 342326)], "staged": 9795064}


def test_off_means_off(engine):
    """Pileup off: the sizes are what they were without the feature; on adds
    exactly 12 x the output slab + a byte per segment; the CCS is the same."""
    zs = [synth(8800, 3000, 6), synth(8801, 1500, 12), synth(8802, 60, 9)]
    try:
        engine.set_pileup(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_pileup(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_pileup(False)
    assert off == OFF_BYTES["zmw_bytes"] and staged_off == OFF_BYTES["staged"]
    add = [12 * _outcap(z) + len(z.lens) for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in add]
    assert staged_on - staged_off == sum(add)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _cli_check(tmp_path, src, args, mode, env=None, is_bam=False, err=None):
    """`args src` with and without -s: the same CCS file; the site file rebuilt
    from the reference on the oracle's preparation and strand flags.  err: a
    list that receives the stderr of the run with -s."""
    out_s, out_0, sites = str(tmp_path / "out_s"), str(tmp_path / "out_0"), str(tmp_path / "sites.tsv")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, **dict(env or {}, CCSX_DEV_SHARE="8"))
    for extra, out in ((["-s", sites], out_s), ([], out_0)):
        r = subprocess.run([BIN] + args + extra + [src, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if err is not None and extra:
            err.append(r.stderr)
    assert open(out_s, "rb").read() == open(out_0, "rb").read()
    want, nrec = "", 0
    for movie, hole, subs in cx.read_zmws(src, is_bam):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        p = oracle_prepare(subs)
        _, _, revs = oracle_prepare_segments(subs)
        assert len(revs) == len(p.lens)
        ccs, recs, *_ = pu.reference(cx.Prepared(p.seqs, p.offs, p.lens, revs), mode)
        if not ccs:
            continue
        nrec += 1
        want += pu.site_lines(f"{movie}/{hole}/ccs", ccs, recs)
    got = open(sites).read()
    assert got == want
    return nrec, want.count("\n")


@pytest.mark.parametrize("flags,mode", [([], 0), (["-P"], 1), (["-q", "-r", "-a"], 0)])
def test_cli_sites(tmp_path, flags, mode):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    flags = [x for f in flags for x in ([f, str(tmp_path / ("side" + f))] if f in ("-r", "-a") else [f])]
    assert _cli_check(tmp_path, fa, ["-A", "-j", "2"] + flags, mode)[0] == 12


def test_cli_sites_async_contexts_order(tmp_path):
    """Pipelined submit / collect on two contexts, three batches per context
    and chunk: the sites stay in input order, each ZMW with its own lines. The run is
    tests/cli_batches.py's SPREAD, and must have spread: several chunks, several
    batches per chunk, several contexts, slots reused.  (Until CCSX_MIN_BATCH
    existed this test asked for 2 contexts x 3 batches and, 300 ZMWs being
    fewer than two batches of the 256-ZMW floor, ran one batch on one context.)"""
    fa = str(tmp_path / "in.fa")
    write(fa, 300, 1000, 6)
    err = []
    assert _cli_check(tmp_path, fa, ["-A", "-j", "4"], 0, env=SPREAD, err=err)[0] == 300
    assert_spread(err[0])


def test_cli_sites_bam_input(tmp_path):
    bam = str(tmp_path / "in.bam")
    write_bam(bam, records(20, 1500, 7, hole0=100))
    assert _cli_check(tmp_path, bam, ["-j", "4"], 0, is_bam=True)[0] == 20
