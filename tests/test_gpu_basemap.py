"""Subread-to-CCS coordinate map from the GPU engine (SPEC.md §11): bases
against the oracle, maps for exact equality against tests/basemap_ref.py (the
definition is integer: no tolerance), through every path the CCS bytes take --
every kernel object, the HBM-read instance, full-capacity re-runs, multi-slice
runs, submit / collect, stage / launch / fetch, and the CLI's -a."""
import ctypes as C
import os
import random
import re
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
from tests import quality_ref as qr
from tests.zmw_cases import edge_cases, raw, shred_cases, synth
from tools.gen_synth import write

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
# chunk boundaries of the column walk (i mod 64, spans that begin / end on a
# chunk edge), the carried cursors over two to seven rounds, a read without a
# base before the breakpoint, an empty segment
SHRED = ("copies_3001", "copies_14000", "span_begin_edge", "span_end_edge", "prefix_10_read2_from_5", "empty_segment",
         "ragged_1001", "i_mod64_0", "i_mod64_63")


@pytest.fixture
def mengine(engine):
    """The shared engine with the map on; it, the other features, forced
    configurations and test hooks are switched back off afterwards."""
    engine.set_base_map(True)
    try:
        yield engine
    finally:
        engine.set_base_map(False)
        engine.set_pass_stats(False)
        engine.set_quality(False)
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)
        engine.set_fault(-1)


def _assert_exact(zs, mode, got, maps):
    want, _, _ = batch(zs, mode, 8)
    for i, z in enumerate(zs):
        ccs, status, _ = got[i]
        assert status == 0 and ccs == want[i], f"ZMW {i}: CCS differs from the oracle"
        rccs, rmaps = br.reference(z, mode)
        assert rccs == ccs
        assert len(maps[i]) == len(z.lens)
        for k, (g, w) in enumerate(zip(maps[i], rmaps)):
            assert g.dtype == np.uint32 and not g.flags.writeable
            assert np.array_equal(g, w), f"ZMW {i} segment {k}: map differs from the reference"


def _check(engine, zs, mode):
    got = engine.run(zs, mode)
    _assert_exact(zs, mode, got, [engine.base_map(i) for i in range(len(zs))])


@pytest.mark.parametrize("mode", MODES)
def test_edge_cases(mengine, mode):
    """n < 3, an empty segment (a zero-length map), nw = 2 (70 reads), ragged
    spans, window growth without a breakpoint."""
    cases = edge_cases()
    names = sorted(cases)
    zs = [cases[k] for k in names]
    _check(mengine, zs, mode)
    m = mengine.base_map(names.index("with_empty_segment"))
    assert len(m[1]) == 0 and len(m[0]) > 0


def test_shred_cases(mengine):
    """Constructed shredding cases: chunk edges of the column walk, cursors
    carried over the rounds."""
    cases = shred_cases()
    assert set(SHRED) <= set(cases)
    zs = [raw(cases[k]) for k in SHRED]
    assert all(len(pr.reference(z, cx.MODE_SHRED)[2]) >= 2 for z in zs[:2])
    _check(mengine, zs, cx.MODE_SHRED)


@pytest.mark.parametrize("L,passes", [(5000, 5), (9000, 3), (3500, 11)])
def test_shredded_multi_round(mengine, L, passes):
    """Several shredding rounds: a segment's entries continue where the
    previous round's cursor left them, offsets run over the whole CCS."""
    zs = [synth(8100 + h, L, passes) for h in range(4)]
    assert all(len(pr.reference(z, cx.MODE_SHRED)[2]) >= 2 for z in zs)
    _check(mengine, zs, cx.MODE_SHRED)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("mode", MODES)
def test_every_kernel_object(mengine, cfg, mode):
    zs = [synth(8200 + h, 3000, 8) for h in range(6)]
    mengine.set_kernel_cfg(cfg)
    _check(mengine, zs, mode)
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert mengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


def test_hbm_read_instance(mengine):
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (nw = 66 mask words, the
    segments' entry offsets summed across the words)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    before = mengine.hbm_launches()
    _check(mengine, [raw(segs)], cx.MODE_SHRED)
    assert mengine.hbm_launches() - before >= 1


@pytest.mark.parametrize("hook", ["tight_out", "tight_rows"])
def test_full_capacity_rerun(mengine, hook):
    """ZMWs that outgrow a tight cap are re-run with full caps, by ccsx_gpu_run
    and inside ccsx_gpu_collect: their maps come from the re-run."""
    zs = [synth(8400 + h, 1500, 6) for h in range(4)] + [cx.prepare([b"ACGTACGTAC"] * 5)]
    if hook == "tight_out":
        mengine.set_tight_out(64)
    else:
        mengine.set_tight_rows(600)
    before = mengine.rerun_count()
    _check(mengine, zs, cx.MODE_SHRED)
    assert mengine.rerun_count() - before >= 4
    s = mengine.submit(zs, cx.MODE_SHRED)
    got = mengine.collect(s)
    assert mengine.rerun_count() - before >= 8
    _assert_exact(zs, cx.MODE_SHRED, got, [mengine.base_map(i, s) for i in range(len(zs))])


def test_multi_slice_run(mengine):
    """12 ZMWs in at least 3 slices: maps gathered in input order."""
    zs = [synth(8500 + h, 1200 + 300 * (h % 4), 5 + h % 3) for h in range(12)]
    tot = sum(mengine.zmw_bytes(z) for z in zs)
    mengine.set_slot_budget(int(tot / 3.5))
    st0 = mengine.run_stats()
    _check(mengine, zs, cx.MODE_SHRED)
    assert mengine.run_stats()["slices"] - st0["slices"] >= 3


def test_submit_collect_both_slots(mengine):
    zs1 = [synth(8600 + h, 2500, 6) for h in range(5)]
    zs2 = [synth(8650 + h, 1500, 9) for h in range(7)]
    s1 = mengine.submit(zs1)
    s2 = mengine.submit(zs2)
    assert {s1, s2} == {0, 1}
    g1 = mengine.collect(s1)
    g2 = mengine.collect(s2)
    _assert_exact(zs1, cx.MODE_SHRED, g1, [mengine.base_map(i, s1) for i in range(len(zs1))])
    _assert_exact(zs2, cx.MODE_SHRED, g2, [mengine.base_map(i, s2) for i in range(len(zs2))])
    # refusals: a ZMW beyond the batch, a segment beyond the ZMW's
    with pytest.raises(cx.GpuError):
        mengine.base_map(len(zs1), s1)
    L = cx.lib()
    p, n = C.POINTER(C.c_uint32)(), C.c_uint32(0)
    nseg = len(zs1[0].lens)
    assert L.ccsx_gpu_base_map(mengine._ctx, s1, 0, nseg - 1, C.byref(p), C.byref(n)) == 0 and n.value == int(zs1[0].lens[-1])
    assert L.ccsx_gpu_base_map(mengine._ctx, s1, 0, nseg, C.byref(p), C.byref(n)) == -1 and not p and n.value == 0
    # a batch submitted, or run, with the feature off has none
    mengine.set_base_map(False)
    s3 = mengine.submit(zs1)
    mengine.collect(s3)
    with pytest.raises(cx.GpuError):
        mengine.base_map(0, s3)
    mengine.run(zs1[:2], cx.MODE_SHRED)
    with pytest.raises(cx.GpuError):
        mengine.base_map(0)


def test_stage_launch_twice_fetch(mengine):
    """A staged slice launched twice: every entry is written once per launch,
    the second launch leaves the same map."""
    zs = [synth(8700 + h, 2000, 6) for h in range(3)] + [synth(8710, 5000, 5)]
    mengine.stage(zs, cx.MODE_SHRED)
    mengine.launch(cx.MODE_SHRED)
    mengine.launch(cx.MODE_SHRED)
    got = mengine.fetch()
    _assert_exact(zs, cx.MODE_SHRED, got, [mengine.base_map(i) for i in range(len(zs))])


@pytest.mark.parametrize("path", ["run", "submit"])
def test_failed_zmw_has_no_map(mengine, path):
    """set_fault(j): ZMW j has no map, every other ZMW's is exact."""
    zs = [synth(8750 + h, 1500, 6) for h in range(4)]
    j = 2
    mengine.set_fault(j)
    if path == "run":
        # (run() raises on a failed ZMW; the call's other results stay with the context)
        with pytest.raises(cx.GpuError):
            mengine.run(zs, cx.MODE_SHRED)
        slot = -1
    else:
        slot = mengine.submit(zs, cx.MODE_SHRED)
        got = mengine.collect(slot)
        assert got[j][1] != 0
        want, _, _ = batch(zs, cx.MODE_SHRED, 8)
        assert [g[0] for i, g in enumerate(got) if i != j] == [w for i, w in enumerate(want) if i != j]
    with pytest.raises(cx.GpuError):
        mengine.base_map(j, slot)
    for i, z in enumerate(zs):
        if i != j:
            for g, w in zip(mengine.base_map(i, slot), br.reference(z, cx.MODE_SHRED)[1]):
                assert np.array_equal(g, w), i


@pytest.mark.parametrize("mode", MODES)
def test_all_three_features(mengine, mode):
    """Quality, pass statistics and the map in one run: every plane exact, and
    the map's flag counts are the GPU's own pass records."""
    zs = [synth(8800 + h, 2500, 7) for h in range(3)] + [edge_cases()["ragged_lengths"]]
    mengine.set_quality(True)
    mengine.set_pass_stats(True)
    got = mengine.run(zs, mode)
    maps = [mengine.base_map(i) for i in range(len(zs))]
    _assert_exact(zs, mode, got, maps)
    for i, z in enumerate(zs):
        assert mengine.quality(i) == qr.reference(z, mode)[1], f"ZMW {i}: qualities differ from the reference"
        rec = mengine.pass_stats(i)
        assert np.array_equal(rec, pr.reference(z, mode)[1]), f"ZMW {i}: pass records differ from the reference"
        for k, m in enumerate(maps[i]):
            ins, mis = (m & br.INS) != 0, (m & br.MISMATCH) != 0
            assert [int((~ins & ~mis).sum()), int(mis.sum()), int(ins.sum())] == rec[k, :3].tolist()
    # the map alone, then pass statistics alone: independent
    mengine.set_quality(False)
    mengine.set_pass_stats(False)
    _check(mengine, zs[:1], mode)
    with pytest.raises(cx.GpuError):
        mengine.pass_stats(0)
    mengine.set_base_map(False)
    mengine.set_pass_stats(True)
    mengine.run(zs[:1], mode)
    assert np.array_equal(mengine.pass_stats(0), pr.reference(zs[0], mode)[1])
    with pytest.raises(cx.GpuError):
        mengine.base_map(0)


def test_off_means_off(engine):
    """Feature off: the sizes are what they are on an engine whose setting was
    never touched; on adds exactly 4 bytes per pushed base; same CCS bytes."""
    zs = [synth(8800, 3000, 6), synth(8801, 1500, 12), synth(8802, 60, 9)]
    fresh = cx.Engine(0)
    try:
        never = [(fresh.zmw_bytes(z, cx.MODE_SHRED), fresh.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        fresh.stage(zs, cx.MODE_SHRED)
        staged_never = fresh.staged_bytes()
    finally:
        fresh.close()
    try:
        engine.set_base_map(False)
        off = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_off = engine.staged_bytes()
        ccs_off = engine.run(zs, cx.MODE_SHRED)
        engine.set_base_map(True)
        on = [(engine.zmw_bytes(z, cx.MODE_SHRED), engine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        engine.stage(zs, cx.MODE_SHRED)
        staged_on = engine.staged_bytes()
        ccs_on = engine.run(zs, cx.MODE_SHRED)
    finally:
        engine.set_base_map(False)
    assert off == never and staged_off == staged_never
    add = [4 * sum(int(x) for x in z.lens) for z in zs]
    assert [(a - c, b - d) for (a, b), (c, d) in zip(on, off)] == [(x, x) for x in add]
    assert staged_on - staged_off == sum(add)
    assert [g for g, _, _ in ccs_on] == [g for g, _, _ in ccs_off]


def _paf(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b""
    rows = []
    for ln in lines[:-1]:
        f = ln.decode().split("\t")
        assert len(f) == 14 and f[12].startswith("sb:i:") and f[13].startswith("cg:Z:")
        rows.append(f)
    return rows


def _cli_check(tmp_path, src, args, mode, env=None, err=None):
    """`args src` with and without -a: the same CCS file; every PAF line
    rebuilt from the reference on the oracle's preparation of the same records.
    err: a list that receives the stderr of the run with -a."""
    out_a, out_0, paf = str(tmp_path / "out_a"), str(tmp_path / "out_0"), str(tmp_path / "aln.paf")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, **dict(env or {}, CCSX_DEV_SHARE="8"))
    for extra, out in ((["-a", paf], out_a), ([], out_0)):
        r = subprocess.run([BIN] + args + extra + [src, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if err is not None and extra:
            err.append(r.stderr)
    assert open(out_a, "rb").read() == open(out_0, "rb").read()
    want = []
    nrec = 0
    for movie, hole, subs in cx.read_zmws(src, False):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        p = oracle_prepare(subs)
        _, _, revs = oracle_prepare_segments(subs)  # (the strand column: the oracle's seg_rev)
        assert len(revs) == len(p.lens)
        ccs, maps = br.reference(p, mode)
        if not ccs:
            continue
        nrec += 1
        for k, m in enumerate(maps):
            a = br.cigar(m)
            if a is None:
                continue
            ln, rev = int(p.lens[k]), bool(revs[k])
            q = (ln - a["qe"], ln - a["qs"]) if rev else (a["qs"], a["qe"])
            want.append([f"{movie}/{hole}/{k}", str(ln), str(q[0]), str(q[1]), "-" if rev else "+", f"{movie}/{hole}/ccs",
                         str(len(ccs)), str(a["ts"]), str(a["te"]), str(a["n_eq"]),
                         str(a["n_eq"] + a["n_x"] + a["n_ins"] + a["n_del"]), "255", f"sb:i:{int(p.offs[k])}",
                         "cg:Z:" + a["cigar"]])
    got = _paf(paf)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g[:12], w[:12])
        # the CIGAR consumes exactly the query and CCS intervals of its line
        ops = re.findall(r"(\d+)([=XID])", g[13][5:])
        assert "".join(n + o for n, o in ops) == g[13][5:]
        qn = sum(int(n) for n, o in ops if o in "=XI")
        tn = sum(int(n) for n, o in ops if o in "=XD")
        assert qn == int(g[3]) - int(g[2]) and tn == int(g[8]) - int(g[7])
    return nrec


@pytest.mark.parametrize("flags,mode", [([], 0), (["-P"], 1), (["-q", "-r"], 0)])
def test_cli_paf(tmp_path, flags, mode):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    if "-r" in flags:  # (-r takes its file)
        flags = flags + [str(tmp_path / "passes.tsv")]
    assert _cli_check(tmp_path, fa, ["-A", "-j", "2"] + flags, mode) == 12


def test_cli_paf_async_contexts_order(tmp_path):
    """Pipelined submit / collect on two contexts, three batches per context
    and chunk: the PAF stays in input order, each ZMW with its own lines. The run is
    tests/cli_batches.py's SPREAD, and must have spread: several chunks, several
    batches per chunk, several contexts, slots reused.  (Until CCSX_MIN_BATCH
    existed this test asked for 2 contexts x 3 batches and, 300 ZMWs being
    fewer than two batches of the 256-ZMW floor, ran one batch on one context.)"""
    fa = str(tmp_path / "in.fa")
    write(fa, 300, 1000, 6)
    err = []
    assert _cli_check(tmp_path, fa, ["-A", "-j", "4"], 0, env=SPREAD, err=err) == 300
    assert_spread(err[0])
