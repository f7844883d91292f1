"""Per-strand consensus from the GPU engine (SPEC.md §14): the CCS against the
oracle, both strands' bases and qualities byte-for-byte against
tests/strand_ref.py (the definition is integer: no tolerance), through every
path the CCS bytes take -- every kernel object, the HBM-read instance, the
full-capacity re-run a long strand consensus forces, multi-slice runs, submit /
collect, stage / launch / fetch, and the CLI's -b."""
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
from tests import strand_ref as sr
from tests.kinetics_cases import with_kin
from tests.pileup_cases import CARRY_CASES, alternating, edge, with_rev
from tests.pileup_cases import constructed as pileup_constructed
from tests.strand_cases import constructed
from tests.zmw_cases import raw, synth
from tools.gen_synth import records, write, write_bam

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
OTHERS = ("quality", "pass_stats", "base_map", "pileup", "kinetics")


@pytest.fixture
def bengine(engine):
    """The shared engine with the by-strand output on; it, the other features,
    forced configurations and test hooks are switched back off afterwards."""
    engine.set_by_strand(True)
    try:
        yield engine
    finally:
        engine.set_by_strand(False)
        for n in OTHERS:
            getattr(engine, "set_" + n)(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)
        engine.set_fault(-1)


def _assert_exact(zs, mode, got, strands):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        r = sr.reference(z, mode)
        assert r.ccs == ccs
        f, fq, v, vq = strands[i]
        for s, (g, gq) in enumerate(((f, fq), (v, vq))):
            assert isinstance(g, bytes) and gq.dtype == np.uint8 and len(g) == len(gq)
            assert len(g) == len(r.seq[s]), f"ZMW {i} strand {s}: {len(g)} bases, the reference has {len(r.seq[s])}"
            assert g == r.seq[s], f"ZMW {i} strand {s}: bases differ from the reference"
            bad = np.nonzero(gq != r.qual[s])[0]
            assert len(bad) == 0, f"ZMW {i} strand {s}: {len(bad)} qualities differ, first at {bad[0]}: " \
                                  f"{gq[bad[0]]} != {r.qual[s][bad[0]]}"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.by_strand(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(bengine, mode):
    """n < 3, an empty segment, nw = 2 (70 reads), ragged spans (cov < n),
    window growth without a breakpoint; strands alternating in push order."""
    cases = edge()
    _check(bengine, [cases[k] for k in sorted(cases)], mode)


@pytest.mark.parametrize("mode", MODES)
def test_constructed_cases(bengine, mode):
    """The pileup's constructed cases (heteroduplex, strand deletion, the carry
    cases, no flags, one strand only, nw = 5) and this output's own: exact
    copies on both strands, all-zero and all-one flags, the strand-private
    insertion."""
    cases = {**pileup_constructed(), **constructed()}
    names = sorted(cases)
    _check(bengine, [cases[k] for k in names], mode)
    f, _, v, _ = bengine.by_strand(names.index("heteroduplex"))
    assert [p for p in range(300) if f[p] != v[p]] == [150] and f[150:151] == b"G" and v[150:151] == b"C"
    f, _, v, _ = bengine.by_strand(names.index("private_insertion"))
    assert len(f) == 400 and len(v) == 420
    f, fq, v, vq = bengine.by_strand(names.index("no_flags"))
    assert v == b"" and len(vq) == 0 and len(f) == 300
    f, _, v, _ = bengine.by_strand(names.index("all_one_flags"))
    assert f == b"" and len(v) == 350


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(bengine, cfg, mode):
    zs = [synth(8200 + h, 3000, 8) for h in range(6)]
    bengine.set_kernel_cfg(cfg)
    _check(bengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert bengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_cursors_across_rounds_on_every_kernel_object(bengine, cfg):
    """Several shredding rounds: each strand's cursor runs on from round to
    round; the carry cases call a strand base in the gap-consensus columns
    behind a round's last CCS base."""
    cases = pileup_constructed()
    carry = [cases[k] for k in CARRY_CASES]
    for z in carry:
        r = sr.reference(z, cx.MODE_SHRED)
        assert len(r.log) >= 2 and r.carry >= 1
    zs = [synth(8100 + h, 5000, 5) for h in range(4)]
    assert all(len(sr.reference(z, cx.MODE_SHRED).log) >= 2 and z.rev.any() and not z.rev.all() for z in zs)
    bengine.set_kernel_cfg(cfg)
    _check(bengine, zs + carry, cx.MODE_SHRED)
    assert bengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_hbm_read_instance(bengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (nw = 66 strand words)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    z = with_rev(raw(segs), alternating(4200))
    before = bengine.hbm_launches()
    _check(bengine, [z], cx.MODE_SHRED)
    assert bengine.hbm_launches() - before >= 1
    assert (bengine.by_strand(0)[1] == qr.Q_MAX).any()


def test_long_strand_consensus_reruns_with_full_capacity(bengine):
    """A strand consensus longer than the tight output slab, which the CCS
    fits: the ZMW fails with the slab's status and is re-run with full caps, by
    ccsx_gpu_run and inside ccsx_gpu_collect; the CCS, the strands and the other
    outputs come from the re-run."""
    z = constructed()["private_insertion"]
    zs = [z, synth(8400, 1500, 6)]
    r = sr.reference(z, cx.MODE_SHRED)
    tight = len(r.ccs) + 10
    assert len(r.ccs) <= tight < len(r.seq[1]) and len(r.seq[0]) <= tight
    bengine.set_quality(True)
    bengine.set_pileup(True)
    bengine.set_tight_out(tight)
    before = bengine.rerun_count()

    def others(slot=-1):
        for i, x in enumerate(zs):
            assert bengine.quality(i, slot) == qr.reference(x, cx.MODE_SHRED)[1]
            assert np.array_equal(bengine.pileup(i, slot), pu.reference(x, cx.MODE_SHRED)[1])

    _check(bengine, zs, cx.MODE_SHRED)
    assert bengine.rerun_count() - before >= 1
    others()
    s = bengine.submit(zs, cx.MODE_SHRED)
    got = bengine.collect(s)
    assert bengine.rerun_count() - before >= 2
    _assert_exact(zs, cx.MODE_SHRED, got, [bengine.by_strand(i, s) for i in range(len(zs))])
    others(s)
    # without the output the tight slab holds the ZMW: the re-run is this output's
    bengine.set_by_strand(False)
    before = bengine.rerun_count()
    got = bengine.run([z], cx.MODE_SHRED)
    assert got[0][0] == r.ccs and bengine.rerun_count() == before


def test_multi_slice_run(bengine):
    """12 ZMWs in at least 3 slices: strands gathered in input order."""
    zs = [synth(8500 + h, 1200 + 300 * (h % 4), 5 + h % 3) for h in range(12)]
    tot = sum(bengine.zmw_bytes(z) for z in zs)
    bengine.set_slot_budget(int(tot / 3.5))
    st0 = bengine.run_stats()
    _check(bengine, zs, cx.MODE_SHRED)
    assert bengine.run_stats()["slices"] - st0["slices"] >= 3


def test_submit_collect_both_slots(bengine):
    zs1 = [synth(8600 + h, 2500, 6) for h in range(5)]
    zs2 = [synth(8650 + h, 1500, 9) for h in range(7)]
    s1 = bengine.submit(zs1)
    with pytest.raises(cx.GpuError, match="not collected"):
        bengine.by_strand(0, s1)
    s2 = bengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = bengine.collect(s1)
    g2 = bengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [bengine.by_strand(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [bengine.by_strand(i, s2) for i in range(len(zs2))])
    with pytest.raises(cx.GpuError, match="beyond the batch"):
        bengine.by_strand(len(zs1), s1)
    # a batch submitted, or run, with the feature off has none
    bengine.set_by_strand(False)
    s3 = bengine.submit(zs1)
    bengine.collect(s3)
    with pytest.raises(cx.GpuError, match="ran with the by-strand output off"):
        bengine.by_strand(0, s3)
    bengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError, match="ran with the by-strand output off"):
        bengine.by_strand(0)


def test_stage_launch_twice_fetch(bengine):
    """A staged slice launched twice: every byte is written once per launch,
    the second launch leaves the same plane."""
    zs = [synth(8700 + h, 2000, 6) for h in range(3)] + [synth(8710, 5000, 5)]
    bengine.stage(zs, cx.MODE_SHRED)
    bengine.launch(cx.MODE_SHRED)
    got = bengine.fetch()
    first = [bengine.by_strand(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, first)
    bengine.launch(cx.MODE_SHRED)
    got = bengine.fetch()
    second = [bengine.by_strand(i) for i in range(len(zs))]
    _assert_exact(zs, cx.MODE_SHRED, got, second)
    for a, b in zip(first, second):
        assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("mode", MODES)
def test_all_six_outputs(bengine, mode):
    """Every output in one run: the strands exact, the other five exact against
    their own references; the GPU's strands agree with the GPU's own pileup at
    every CCS base (SPEC.md §14)."""
    zs = [with_kin(z, seed=40 + j) for j, z in
          enumerate([synth(8800 + h, 2500, 7) for h in range(3)] + [edge()["ragged_lengths"]])]
    for n in OTHERS:
        getattr(bengine, "set_" + n)(True)
    got = bengine.run(zs, mode)
    strands = [bengine.by_strand(i) for i in range(len(zs))]
    _assert_exact(zs, mode, got, strands)
    for i, z in enumerate(zs):
        assert bengine.quality(i) == qr.reference(z, mode)[1], f"ZMW {i}: qualities differ from the reference"
        assert np.array_equal(bengine.pass_stats(i), pr.reference(z, mode)[1]), f"ZMW {i}: pass records differ"
        for g, w in zip(bengine.base_map(i), br.reference(z, mode)[1]):
            assert np.array_equal(g, w), f"ZMW {i}: map differs from the reference"
        pile = bengine.pileup(i)
        assert np.array_equal(pile, pu.reference(z, mode)[1]), f"ZMW {i}: pileup differs from the reference"
        assert np.array_equal(bengine.kinetics(i), kr.reference(z, mode)[1]), f"ZMW {i}: kinetics differ"
        # a strand's bases at the CCS's columns are its pileup calls there
        r = sr.reference(z, mode)
        for s in (0, 1):
            calls = r.calls[:, s]
            at = np.cumsum((calls >= 0) & (calls < 4)) - 1  # the strand offset of a column's base
            for p in np.nonzero(~(pile == 255).any(1))[0][::17]:
                c = cx.pileup_call(pile[p], s)
                col = r.base_col[p]
                assert c == calls[col]
                if 0 <= c < 4:
                    assert strands[i][2 * s][at[col]:at[col] + 1] == b"ACGT"[c:c + 1]
    # the strands alone: independent of the others
    for n in OTHERS:
        getattr(bengine, "set_" + n)(False)
    _check(bengine, zs[:1], mode)
    with pytest.raises(cx.GpuError, match="ran with the pileup off"):
        bengine.pileup(0)


@pytest.mark.parametrize("path", ["run", "submit"])
def test_failed_zmw_is_refused(bengine, path):
    zs = [synth(8900 + h, 1500, 6) for h in range(3)]
    bengine.set_fault(1)
    if path == "run":
        with pytest.raises(cx.GpuError):
            bengine.run(zs, cx.MODE_SHRED)
        slot = -1
    else:
        slot = bengine.submit(zs, cx.MODE_SHRED)
        got = bengine.collect(slot)
        assert got[1][1] != 0 and got[1][0] == b""
    with pytest.raises(cx.GpuError, match="that ZMW failed: it has no strand consensus"):
        bengine.by_strand(1, slot)
    for i in (0, 2):
        r = sr.reference(zs[i], cx.MODE_SHRED)
        f, fq, v, vq = bengine.by_strand(i, slot)
        assert (f, v) == r.seq and np.array_equal(fq, r.qual[0]) and np.array_equal(vq, r.qual[1])


def _outcap(z):
    # ccsx_layout.h zcaps, tight caps: min(S + 16, 2 x longest segment + 1,024)
    lens = [int(x) for x in z.lens]
    return min(sum(lens) + 16, 2 * max(lens) + 1024)


# ccsx_gpu_zmw_bytes (shredded, -P) and ccsx_gpu_staged_bytes of the three ZMWs
# below as the library computed them before it knew of any optional plane
OFF_BYTES = {"zmw_bytes": [(5692042, 5692042), (3761272, 3761272), (342326, 342326)], "staged": 9795064}


def test_off_means_off(engine):
    """Output off: the sizes are what they were without the feature; on adds
    exactly 4 x the output slab + a byte per segment + 8 per ZMW; the CCS is the same."""
    zs = [synth(8800, 3000, 6), synth(8801, 1500, 12), synth(8802, 60, 9)]
    try:
        engine.set_by_strand(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_by_strand(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_by_strand(False)
    assert off == OFF_BYTES["zmw_bytes"] and staged_off == OFF_BYTES["staged"]
    add = [4 * _outcap(z) + len(z.lens) + 8 for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in add]
    assert staged_on - staged_off == sum(add)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _cli_check(tmp_path, src, args, mode, fastq, is_bam=False, env=None, err=None):
    """`args src` with and without -b: the same main output; the -b file
    rebuilt from the reference on the oracle's preparation and strand flags.
    err: a list that receives the stderr of the run with -b."""
    out_b, out_0, strands = str(tmp_path / "out_b"), str(tmp_path / "out_0"), str(tmp_path / "strands")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, **dict(env or {}, CCSX_DEV_SHARE="8"))
    for extra, out in ((["-b", strands], out_b), ([], out_0)):
        r = subprocess.run([BIN] + args + extra + [src, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if err is not None and extra:
            err.append(r.stderr)
    assert open(out_b, "rb").read() == open(out_0, "rb").read()
    want, nrec = "", 0
    for movie, hole, subs in cx.read_zmws(src, is_bam):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        p = oracle_prepare(subs)
        _, _, revs = oracle_prepare_segments(subs)
        assert len(revs) == len(p.lens)
        r = sr.reference(cx.Prepared(p.seqs, p.offs, p.lens, revs), mode)
        if not r.ccs:
            continue
        nrec += 1
        want += sr.fasta(f"{movie}/{hole}/ccs", r, fastq, revs, cx.qual_rq)
    assert open(strands).read() == want
    return nrec, want.count(">" if not fastq else "\n+\n")


@pytest.mark.parametrize("flags,mode", [([], 0), (["-P"], 1), (["-q"], 0), (["-q", "-r", "-a", "-s"], 0)])
def test_cli_by_strand(tmp_path, flags, mode):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    fastq = "-q" in flags
    flags = [x for f in flags for x in ([f, str(tmp_path / ("side" + f))] if f in ("-r", "-a", "-s") else [f])]
    nrec, nstrand = _cli_check(tmp_path, fa, ["-A", "-j", "2"] + flags, mode, fastq)
    assert nrec == 12 and nstrand == 24


def test_cli_by_strand_async_contexts_order(tmp_path):
    """Pipelined submit / collect on 2 x 2 contexts, three batches per context
    and chunk (tests/cli_batches.py's SPREAD, and the run must have spread):
    the records stay in input order, each ZMW with its own two strands."""
    fa = str(tmp_path / "in.fa")
    write(fa, 300, 1000, 6)
    err = []
    nrec, nstrand = _cli_check(tmp_path, fa, ["-A", "-j", "4"], 0, False, env=SPREAD, err=err)
    assert nrec == 300 and nstrand == 600
    assert_spread(err[0])


def test_cli_by_strand_bam_input(tmp_path):
    bam = str(tmp_path / "in.bam")
    write_bam(bam, records(20, 1500, 7, hole0=100))
    assert _cli_check(tmp_path, bam, ["-j", "4"], 0, False, is_bam=True)[0] == 20
