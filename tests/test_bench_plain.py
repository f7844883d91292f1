"""bench.py's plain run (the headline alone) and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_records_lengths(tmp_path):
    """One length per record in output order, an empty CCS as 0."""
    fa = tmp_path / "ccs.fa"
    fa.write_bytes(b">m/7/ccs\nACGT\n>m/9/ccs\n\n>m/12/ccs\nGG\n")
    scan = {}
    bench.read_records(str(fa), {9, 12}, scan)
    assert scan["nrec"] == 3 and scan["in_order"] and scan["lens"] == [4, 0, 2]
    assert scan["got"] == {9: b"", 12: b"GG"}


def test_dump_sample_is_fixed():
    ids = range(1000, 26000)
    s = bench.dump_sample(ids)
    assert s == bench.dump_sample(ids) == sorted(s)
    assert len(set(s)) == bench.DUMP_SAMPLE and set(s) <= set(ids)
    assert bench.dump_sample(range(5)) == [0, 1, 2, 3, 4]


def test_dump_outputs_arrays_and_size_cap(tmp_path, monkeypatch):
    ccs = {3: b"ACGT", 5: b"", 8: b"TTG"}
    n = bench.dump_outputs(str(tmp_path / "d"), [3, 5, 8], ccs, [4, 9, 0, 3])
    a = {k: np.load(tmp_path / "d" / (k + ".npy")) for k in n}
    assert sorted(a) == ["ccs_len", "sample_ccs", "sample_ids", "sample_len"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["ccs_len"].tolist() == [4, 9, 0, 3]
    assert a["sample_ids"].tolist() == [3, 5, 8] and a["sample_len"].tolist() == [4, 0, 3]
    assert bytes(a["sample_ccs"].astype(np.uint8)) == b"ACGTTTG"
    assert n == {k: v.size for k, v in a.items()}
    # the sample is cut where the files would pass the limit
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (1 << 16) + 4 * 8 + 4 * 4 + 16 + 8)
    bench.dump_outputs(str(tmp_path / "e"), [3, 5, 8], ccs, [4, 9, 0, 3])
    assert np.load(tmp_path / "e" / "sample_ids.npy").tolist() == [3]
    assert np.load(tmp_path / "e" / "ccs_len.npy").tolist() == [4, 9, 0, 3]


@pytest.mark.gpu
def test_plain_run_measures_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """A plain run: --steps sets the work (3 steps of 32 config-E ZMWs through
    the CLI), the line holds the headline's fields and none of the --full
    lines, and --dump-outputs holds the last step's CCS: all their lengths,
    and sampled CCS that are the oracle's for those holes."""
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "0",
           "--e-zmws", "32", "--settle", "0", "--out-dir", str(tmp_path / "logs"), "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "CCS ZMWs/sec (whole node)" and out["unit"] == "ZMWs/s" and out["higher_is_better"]
    assert out["dtype"] == "int32" and out["steps"] == 3 and out["warmup"] == 0
    assert out["cli"]["zmws"] == out["cli"]["records"] == 96 and out["cli"]["records_in_input_order"]
    assert out["ms_per_step"] == pytest.approx(out["cli"]["cli_s"] * 1e3 / 3, rel=1e-3)
    assert out["value"] == pytest.approx(96 / out["cli"]["cli_s"], rel=1e-3)
    for k in ("roofline", "kernel_B", "e2e", "cpu_baseline", "one_process"):
        assert k not in out
    a = {k: np.load(d / (k + ".npy")) for k in ("ccs_len", "sample_ids", "sample_len", "sample_ccs")}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    last = range(bench.E_HOLE0 + 64, bench.E_HOLE0 + 96)
    assert a["ccs_len"].size == 32 and a["sample_ids"].tolist() == list(last)
    assert a["sample_len"].tolist() == a["ccs_len"].tolist() and a["sample_ccs"].size == a["sample_len"].sum()
    # the first four sampled CCS against the oracle's
    import ccsx_amd as cx
    from oracle.oracle import prepare as oracle_prepare
    ends = np.cumsum(a["sample_len"]).astype(int)
    pairs = []
    for i, h in enumerate(list(last)[:4]):
        got = bytes(a["sample_ccs"][ends[i] - int(a["sample_len"][i]):ends[i]].astype(np.uint8))
        pairs.append((oracle_prepare(cx.synth_zmw(bench.SEED, h, *bench.zmw_shape(bench.CONFIGS["E"], h))[0]), got))
    assert bench.oracle_check(pairs, 4) == 4
