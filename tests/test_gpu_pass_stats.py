"""Per-pass alignment statistics from the GPU engine (SPEC.md §10): bases
against the oracle, records for exact equality against tests/pass_ref.py (the
definition is integer: no tolerance), through every path the CCS bytes take --
every kernel object, the HBM-read instance, full-capacity re-runs, multi-slice
runs, submit / collect, stage / launch / fetch, and the CLI's -r."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from oracle.oracle import prepare as oracle_prepare
from tests.cli_batches import SPREAD, assert_spread
from tests import pass_ref as pr
from tests import quality_ref as qr
from tests.zmw_cases import edge_cases, raw, synth
from tools.gen_synth import write

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]


@pytest.fixture
def pengine(engine):
    """The shared engine with pass statistics on; they, quality, forced
    configurations and test hooks are switched back off afterwards."""
    engine.set_pass_stats(True)
    try:
        yield engine
    finally:
        engine.set_pass_stats(False)
        engine.set_quality(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)
        engine.set_fault(-1)


def _assert_exact(zs, mode, got, recs):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        rccs, rrec, _ = pr.reference(z, mode)
        assert rccs == ccs
        assert recs[i].dtype == np.uint32 and recs[i].shape == (len(z.lens), 6)
        assert np.array_equal(recs[i], rrec), f"ZMW {i}: pass records differ from the reference"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.pass_stats(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(pengine, mode):
    """n < 3, an empty segment (an all-zero record), nw = 2 (70 reads), ragged
    spans (del with cov < n), window growth without a breakpoint."""
    cases = edge_cases()
    names = sorted(cases)
    zs = [cases[k] for k in names]
    _check(pengine, zs, mode)
    rec = pengine.pass_stats(names.index("with_empty_segment"))
    assert not rec[1].any() and rec[0].any()


@pytest.mark.parametrize("L,passes", [(5000, 5), (9000, 3), (3500, 11)])
def test_shredded_multi_round(pengine, L, passes):
    """Several shredding rounds: the records sum the emitted columns [0, i) of
    every round, cbeg / cend run over the whole CCS."""
    zs = [synth(8100 + h, L, passes) for h in range(4)]
    assert all(len(pr.reference(z, cx.MODE_SHRED)[2]) >= 2 for z in zs)
    _check(pengine, zs, cx.MODE_SHRED)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(pengine, cfg, mode):
    zs = [synth(8200 + h, 3000, 8) for h in range(6)]
    pengine.set_kernel_cfg(cfg)
    _check(pengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert pengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_long_reads_primitive(pengine):
    """-P pushes the 20 kb segments whole: one POA call of ~25k columns."""
    _check(pengine, [synth(8300, 20000, 5)], cx.MODE_PRIMITIVE)


def test_hbm_read_instance(pengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (nw = 66 mask words)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    before = pengine.hbm_launches()
    _check(pengine, [raw(segs)], cx.MODE_SHRED)
    assert pengine.hbm_launches() - before >= 1


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
    _assert_exact(zs, cx.MODE_SHRED, got, [pengine.pass_stats(i, s) for i in range(len(zs))])


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
    s2 = pengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = pengine.collect(s1)
    g2 = pengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [pengine.pass_stats(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [pengine.pass_stats(i, s2) for i in range(len(zs2))])
    with pytest.raises(cx.GpuError):
        pengine.pass_stats(len(zs1), s1)
    # a batch submitted, or run, with the feature off has none
    pengine.set_pass_stats(False)
    s3 = pengine.submit(zs1)
    pengine.collect(s3)
    with pytest.raises(cx.GpuError):
        pengine.pass_stats(0, s3)
    pengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError):
        pengine.pass_stats(0)


def test_stage_launch_twice_fetch(pengine):
    """A staged slice launched twice: the kernel resets the records, the second
    launch's are not added to the first's."""
    zs = [synth(8700 + h, 2000, 6) for h in range(3)] + [synth(8710, 5000, 5)]
    pengine.stage(zs, cx.MODE_SHRED)
    pengine.launch(cx.MODE_SHRED)
    pengine.launch(cx.MODE_SHRED)
    got = pengine.fetch()
    _assert_exact(zs, cx.MODE_SHRED, got, [pengine.pass_stats(i) for i in range(len(zs))])


@pytest.mark.parametrize("path", ["run", "submit"])
def test_failed_zmw_has_no_records(pengine, path):
    """set_fault(j): ZMW j has no records, every other ZMW's are exact."""
    zs = [synth(8750 + h, 1500, 6) for h in range(4)]
    j = 2
    pengine.set_fault(j)
    if path == "run":
        # (run() raises on a failed ZMW; the call's other results stay with the context)
        with pytest.raises(cx.GpuError):
            pengine.run(zs, cx.MODE_SHRED)
        slot = -1
    else:
        slot = pengine.submit(zs, cx.MODE_SHRED)
        got = pengine.collect(slot)
        assert got[j][1] != 0
        want, _, _ = batch(zs, cx.MODE_SHRED, 8)
        assert [g[0] for i, g in enumerate(got) if i != j] == [w for i, w in enumerate(want) if i != j]
    with pytest.raises(cx.GpuError):
        pengine.pass_stats(j, slot)
    for i, z in enumerate(zs):
        if i != j:
            assert np.array_equal(pengine.pass_stats(i, slot), pr.reference(z, cx.MODE_SHRED)[1]), i


@pytest.mark.parametrize("mode", MODES)
def test_with_quality(pengine, mode):
    """Quality and pass statistics in the same run: two planes, both exact."""
    zs = [synth(8800 + h, 2500, 7) for h in range(3)] + [edge_cases()["ragged_lengths"]]
    pengine.set_quality(True)
    got = pengine.run(zs, mode)
    _assert_exact(zs, mode, got, [pengine.pass_stats(i) for i in range(len(zs))])
    for i, z in enumerate(zs):
        assert pengine.quality(i) == qr.reference(z, mode)[1], f"ZMW {i}: qualities differ from the reference"
    # quality alone: no records
    pengine.set_pass_stats(False)
    pengine.run(zs[:1], mode)
    assert pengine.quality(0) == qr.reference(zs[0], mode)[1]
    with pytest.raises(cx.GpuError):
        pengine.pass_stats(0)


def test_off_means_off(engine):
    """Feature off: the sizes are what they are on an engine whose setting was
    never touched; on adds exactly 24 bytes per segment; same CCS bytes."""
    zs = [synth(8800, 3000, 6), synth(8801, 1500, 12), synth(8802, 60, 9)]
    fresh = cx.Engine(0)
    try:
        never = [(fresh.zmw_bytes(z, cx.MODE_SHRED), fresh.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        fresh.stage(zs, cx.MODE_SHRED)
        staged_never = fresh.staged_bytes()
    finally:
        fresh.close()
    try:
        engine.set_pass_stats(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_pass_stats(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_pass_stats(False)
    assert off == never and staged_off == staged_never
    add = [24 * len(z.lens) for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in add]
    assert staged_on - staged_off == sum(add)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _report(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and lines[0].startswith(b"#")
    assert lines[0][1:].split(b"\t") == [b"name", b"pass", b"sbeg", b"slen", b"match", b"mismatch", b"ins", b"del",
                                         b"cbeg", b"cend", b"identity"]
    rows = []
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        assert len(f) == 11
        rows.append((f[0], [int(x) for x in f[1:10]], float(f[10])))
    return rows


def _cli_check(tmp_path, src, args, mode, env=None, err=None):
    """`args src` with and without -r: the same CCS file; the report's lines
    from the reference on the oracle's preparation of the same records.  err: a
    list that receives the stderr of the run with -r."""
    out_r, out_0, rep = str(tmp_path / "out_r"), str(tmp_path / "out_0"), str(tmp_path / "passes.tsv")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, **dict(env or {}, CCSX_DEV_SHARE="8"))
    for extra, out in ((["-r", rep], out_r), ([], out_0)):
        r = subprocess.run([BIN] + args + extra + [src, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if err is not None and extra:
            err.append(r.stderr)
    assert open(out_r, "rb").read() == open(out_0, "rb").read()
    want = []
    nrec = 0
    for movie, hole, subs in cx.read_zmws(src, False):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        p = oracle_prepare(subs)
        ccs, rec, _ = pr.reference(p, mode)
        if not ccs:
            continue
        nrec += 1
        for k in range(len(p.lens)):
            want.append((b"%s/%s/ccs" % (movie.encode(), hole.encode()),
                         [k, int(p.offs[k]), int(p.lens[k])] + [int(x) for x in rec[k]], pr.identity(rec[k])))
    got = _report(rep)
    assert len(got) == len(want)
    for (name, ints, ident), (wname, wints, wident) in zip(got, want):
        assert name == wname and ints == wints, (name, ints, wints)
        assert abs(ident - wident) <= 1e-6
    return nrec


@pytest.mark.parametrize("flags,mode", [([], 0), (["-P"], 1), (["-q"], 0)])
def test_cli_report(tmp_path, flags, mode):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    assert _cli_check(tmp_path, fa, ["-A", "-j", "2"] + flags, mode) == 12


def test_cli_report_async_contexts_order(tmp_path):
    """Pipelined submit / collect on two contexts, three batches per context
    and chunk: the report stays in input order, each ZMW with its own records. The run is
    tests/cli_batches.py's SPREAD, and must have spread: several chunks, several
    batches per chunk, several contexts, slots reused.  (Until CCSX_MIN_BATCH
    existed this test asked for 2 contexts x 3 batches and, 300 ZMWs being
    fewer than two batches of the 256-ZMW floor, ran one batch on one context.)"""
    fa = str(tmp_path / "in.fa")
    write(fa, 300, 1000, 6)
    err = []
    assert _cli_check(tmp_path, fa, ["-A", "-j", "4"], 0, env=SPREAD, err=err) == 300
    assert_spread(err[0])
