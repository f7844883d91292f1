"""The host program's per-batch gather (host/main.cpp's worker: every optional
output cut out of a device context per batch and slot, and the polisher, the
demultiplexer and the scanner run per batch on one shared context each) on
tests/stage_cases.py's family under tests/cli_batches.py's SPREAD: three
chunks, up to twelve batches per chunk, four workers.  Every comparison is
byte for byte, and no expectation comes from the configuration under test:

* each stage alone (-p; -B -d -D; -I -i -S), with and without -q, against the
  oracle's CCS, the qualities' reference and the stages' host definitions
  (ccsx_polish_host on the engine's drafts and maps, ccsx_barcode_host +
  ccsx_barcode_call, ccsx_scan_host + ccsx_scan_cut; every 8th ZMW also
  against the Python references);
* everything at once (-q -r -a -s -b -p -B -d -D -I -i -S), pipelined and with
  CCSX_ASYNC=0, against runs with one option each in the default
  configuration (one chunk, one batch: the path the other CLI tests pin);
* the same with one ZMW failed by the test hook in the middle of a batch, so
  the stages' compacted index differs from the batch index after it;
* the same on one worker, which separates an indexing error from one of
  concurrency.

(-k needs BAM input: tests/test_gpu_kinetics.py's order test covers it.)"""
import os
import subprocess
from collections import namedtuple

import pytest

import ccsx_amd as cx
from tests import barcode_ref as BR
from tests import quality_ref as qr
from tests import scan_ref as SR
from tests import stage_cases as st
from tests import stage_format as F
from tests.cli_batches import SINGLE, SPREAD, assert_spread

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")

# option group -> the files it writes (the key is the option's letter)
GROUPS = {"r": ["r"], "a": ["a"], "s": ["s"], "b": ["b"], "p": ["p"], "B": ["d", "D"], "I": ["i", "S"]}
FASTQ_LIKE = {"out", "b", "p", "d", "S"}   # records of 4 lines with -q; the others are one line per row
DEFAULT = dict(CCSX_DEV_SHARE="8")         # one chunk, one batch (an eighth of the device per context)
Run = namedtuple("Run", "files stderr")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return st.write_inputs(tmp_path_factory.mktemp("stage_in"))


@pytest.fixture(scope="module")
def cli(inputs, tmp_path_factory):
    """cli(groups, fastq, env) -> Run: one run of the host program, its files by key."""
    fa, bfa, afa = inputs

    def run(groups, fastq, env):
        d = tmp_path_factory.mktemp("stage_run")
        args = ["-A", "-j", "4", "-m", str(st.MIN_TOTAL)] + (["-q"] if fastq else [])
        for g in groups:
            if g == "B":
                args += ["-B", bfa]
            if g == "I":
                args += ["-I", afa]
            for k in GROUPS[g]:
                args += ["-" + k, str(d / k)]
        r = subprocess.run([BIN] + args + [fa, str(d / "out")], capture_output=True, timeout=300,
                           env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        keys = ["out"] + [k for g in groups for k in GROUPS[g]]
        return Run({k: open(d / k, "rb").read() for k in keys}, r.stderr.decode(errors="replace"))

    return run


_main: dict = {}


def main_records(fastq: bool) -> list:
    """[(header without its first character, bases, qualities)] of the main
    output by the oracle alone (and tests/quality_ref.py with -q), computed once."""
    if fastq not in _main:
        ps, ccs = st.oracle_ccs()
        recs = []
        for (h, _), p, c in zip(st.kept(), ps, ccs):
            assert c
            if fastq:
                qc, qual, _ = qr.reference(p, 0)
                assert qc == c
                recs.append((f"synth/{h}/ccs np={len(p.lens)} rq={cx.qual_rq(qual):.6f}", c.decode(),
                             bytes(q + 33 for q in qual).decode()))
            else:
                recs.append((f"synth/{h}/ccs", c.decode(), None))
        _main[fastq] = recs
    return _main[fastq]


def main_text(recs, fastq: bool) -> bytes:
    return "".join(f"@{h}\n{s}\n+\n{q}\n" if fastq else f">{h}\n{s}\n" for h, s, q in recs).encode()


@pytest.fixture(scope="module")
def polished(engine):
    """[(name, bases, qualities)] by ccsx_polish_host on the engine's drafts and
    maps of the family (one ccsx_gpu_run with the base map on), the drafts held
    to the oracle's CCS."""
    ks = st.kept()
    zs = [cx.prepare(subs) for _, subs in ks]
    engine.set_base_map(True)
    try:
        res = engine.run(zs, cx.MODE_SHRED)
        items = [(ccs, [z.seqs[int(o):int(o) + int(n)] for o, n in zip(z.offs, z.lens)], engine.base_map(i))
                 for i, (z, (ccs, status, _)) in enumerate(zip(zs, res)) if status == 0 and ccs]
    finally:
        engine.set_base_map(False)
    assert [it[0] for it in items] == list(st.oracle_ccs()[1])
    out = []
    for (h, _), it in zip(ks, items):
        seq, qual, _, _, status = cx.polish_host(*it)
        assert status == 0 and seq
        out.append((f"synth/{h}/ccs/polished", seq.decode(), bytes(q + 33 for q in qual).decode()))
    # (the stage does something here: a file equal to the draft's would pin nothing)
    assert any(seq != it[0].decode() for (_, seq, _), it in zip(out, items))
    return out


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_polish_alone(cli, polished, fastq):
    run = cli(["p"], fastq, SPREAD)
    assert_spread(run.stderr)
    assert run.files["out"] == main_text(main_records(fastq), fastq)
    assert run.files["p"] == main_text(polished, fastq)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_demux_alone(cli, fastq):
    bcs = st.family()[0]
    run = cli(["B"], fastq, SPREAD)
    assert_spread(run.stderr)
    recs = main_records(fastq)
    assert run.files["out"] == main_text(recs, fastq)
    want_d, want_t, rows = F.demux_files(recs, bcs, st.BC_NAMES, fastq, cx.barcode_host, cx.barcode_call)
    assert run.files["d"].decode() == want_d
    assert run.files["D"].decode() == want_t
    assert sum(1 for _, c in rows if c[3]) >= 70 and sum(1 for _, c in rows if not c[3]) >= 8
    for (_, seq, _), (r, c) in list(zip(recs, rows))[::8]:
        assert r == BR.score(bcs, seq.encode(), 96) and c == BR.call(r, [16] * 12, len(seq))


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_scan_alone(cli, fastq):
    ads = st.family()[1]
    run = cli(["I"], fastq, SPREAD)
    assert_spread(run.stderr)
    recs = main_records(fastq)
    assert run.files["out"] == main_text(recs, fastq)
    want_t, want_p, found = F.scan_files(recs, ads, st.AD_NAMES, fastq, cx.scan_host, cx.scan_cut)
    assert run.files["i"].decode() == want_t
    assert run.files["S"].decode() == want_p
    assert sum(1 for f in found if f) >= 56 and sum(1 for f in found if not f) >= 24
    for (_, seq, _), hs in list(zip(recs, found))[::8]:
        assert hs == SR.hits(ads, seq.encode()) and cx.scan_cut(hs, len(seq)) == SR.cut(hs, len(seq))


@pytest.fixture(scope="module")
def everything(cli):
    """Everything at once under SPREAD: the run the three tests below compare."""
    run = cli(list(GROUPS), True, SPREAD)
    assert_spread(run.stderr)
    return run


@pytest.fixture(scope="module")
def everything_sync(cli):
    run = cli(list(GROUPS), True, dict(SPREAD, CCSX_ASYNC="0"))
    assert_spread(run.stderr)
    return run


@pytest.mark.parametrize("group", list(GROUPS))
def test_everything_at_once(cli, everything, everything_sync, group):
    """Each file of the run with every option on, pipelined and one
    ccsx_gpu_run per batch, equals the file of a run with that option alone
    (and -q) as one chunk and one batch."""
    alone = cli([group], True, DEFAULT)
    for k in ["out"] + GROUPS[group]:
        assert alone.files[k], k
        assert everything.files[k] == alone.files[k], k
        assert everything_sync.files[k] == alone.files[k], k


def test_single_worker(cli, everything):
    """SPREAD's chunks on one context with one worker: the same files."""
    run = cli(list(GROUPS), True, SINGLE)
    assert_spread(run.stderr, single=True)
    assert set(run.files) == set(everything.files)
    for k, v in run.files.items():
        assert v == everything.files[k], k


def _without_hole(key: str, data: bytes, hole: int) -> bytes:
    """A file of a -q run minus the records of one hole."""
    lines = data.split(b"\n")
    assert lines[-1] == b""
    lines = lines[:-1]
    name = b"synth/%d/" % hole
    if key in FASTQ_LIKE:
        assert len(lines) % 4 == 0
        keep = [lines[k:k + 4] for k in range(0, len(lines), 4) if not lines[k][1:].startswith(name)]
        lines = [ln for rec in keep for ln in rec]
    else:
        lines = [ln for ln in lines if not ln.startswith(name)]
    return b"".join(ln + b"\n" for ln in lines)


def test_failed_zmw_among_the_others(cli, everything):
    """One ZMW of the 64-ZMW chunk fails on the device (the CCSX_FAULT_HOLE test
    hook), at a position inside its batch: the stages skip it, so from there on
    their compacted index is one behind the batch's.  Every file is the full
    run's minus that hole's records."""
    batch, pos = st.fault_batch(cx)
    assert batch[pos] == st.FAULT_HOLE and 0 < pos < len(batch) - 1, (batch, pos)
    run = cli(list(GROUPS), True, dict(SPREAD, CCSX_FAULT_HOLE=str(st.FAULT_HOLE)))
    assert_spread(run.stderr)
    # the batch ran as computed: a batch of that size in the second chunk
    assert f"[ccsx] chunk 1 batch of {len(batch)} ZMWs" in run.stderr
    assert f"synth/{st.FAULT_HOLE}: no CCS" in run.stderr and run.stderr.count(": no CCS") == 1
    for word in ("polisher:", "demultiplexer:", "scanner:"):
        assert word not in run.stderr, run.stderr[-2000:]
    assert set(run.files) == set(everything.files)
    for k, v in run.files.items():
        want = _without_hole(k, everything.files[k], st.FAULT_HOLE)
        if k in ("out", "r", "a", "b", "p", "D", "i", "S"):   # (the hole has two adapters; sites and an assignment it may lack)
            assert want != everything.files[k], k
        assert v == want, k
