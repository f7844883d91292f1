"""ccsx_barcode_host (SPEC.md §16 as a sequential loop, host/barcode.cpp)
against tests/barcode_ref.py on the constructed cases, field for field; what
each case was built to reach; ccsx_barcode_call against its Python statement at
the thresholds' edges; the barcode file reader; the host program's usage errors
(no GPU is touched); the host functions under AddressSanitizer +
UndefinedBehaviorSanitizer (tools/barcode_sanitize.cpp, a stand-alone program;
only that program runs under the sanitizer); and the accuracy case through the
oracle's CCS.

Accuracy, measured on the reference (barcode_cases.accuracy_case, seed 7): all
12 ZMWs assigned to their pair; the smallest lead and the smallest score are
printed by the test and recorded in DESIGN.md §20."""
import gzip
import os
import subprocess

import pytest

import ccsx_amd as cx
from oracle.oracle import Poa, prepare

from . import barcode_cases as bc
from . import barcode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ccsx_amd", "bin", "ccsx")
EXE = os.path.join(ROOT, "build", "barcode_sanitize")
SRCS = ["tools/barcode_sanitize.cpp", "ccsx_amd/csrc/host/barcode.cpp"]


@pytest.mark.parametrize("i", range(len(bc.CASES)), ids=bc.NAMES)
def test_host_equals_reference(i):
    _, si, ccs, expect = bc.CASES[i]
    barcodes, window = bc.SETS[si]
    want = bc.reference(i)
    assert cx.barcode_host(barcodes, ccs, window) == want
    # the situation the case was built for
    for e, key in enumerate(("e0", "e1")):
        if key in expect:
            assert want[e][:len(expect[key])] == expect[key], (key, want[e])
    if "check" in expect:
        assert expect["check"](want), want


def test_cases_reach_their_shapes():
    by = {c[0]: c for c in bc.CASES}
    n = lambda name: len(by[name][2])  # noqa: E731
    assert n("n0") == 0 and n("n1") == 1 and n("n_lt_L") < 16 and n("n_lt_wn") < 96 <= n("overlapping_windows") < 192
    assert {w for _, w in bc.SETS} >= {1, 256}
    assert {len(s) for s, _ in bc.SETS} >= {1, 32, 33, 96}
    assert sorted(len(b) for b in bc.MIXED) == [1, 8, 16, 25, 40, 64]
    assert bc.PAL == R.revcomp(bc.PAL) and R.edit_distance(bc.NEARPAL, R.revcomp(bc.NEARPAL)) == 2
    assert bc.BIG_TIE[70] == bc.BIG_TIE[3] and (2 * 70) // 64 == 2


@pytest.mark.parametrize("name", sorted(bc.REJECTED))
def test_rejected_sets(name):
    assert not R.set_ok(bc.REJECTED[name])
    with pytest.raises(ValueError):
        cx.barcode_host(bc.REJECTED[name], b"ACGTACGTACGT", 96)


@pytest.mark.parametrize("window", [0, 257])
def test_rejected_windows(window):
    with pytest.raises(ValueError):
        cx.barcode_host(bc.BC, b"ACGTACGTACGT", window)


@pytest.mark.parametrize("i", range(len(bc.CALLS)), ids=[c[0] for c in bc.CALLS])
def test_call_equals_its_statement(i):
    _, result, lens, n, T, D, expect = bc.CALLS[i]
    want = R.call(result, lens, n, T, D)
    assert want == expect
    assert cx.barcode_call(result, lens, n, T, D) == want


def test_call_on_the_cases():
    for i, (_, si, ccs, _) in enumerate(bc.CASES):
        lens = [len(b) for b in bc.SETS[si][0]]
        r = bc.reference(i)
        assert cx.barcode_call(r, lens, len(ccs)) == R.call(r, lens, len(ccs))


def test_barcode_file_reader(tmp_path):
    fa = tmp_path / "bc.fa"
    fa.write_text(">bc1 first barcode\nACGTACGT\nacgt\n>bc2\tx\nTTTTGGGG\n>lone\nA\n")
    want = [("bc1", b"ACGTACGTacgt"), ("bc2", b"TTTTGGGG"), ("lone", b"A")]
    assert cx.read_barcodes(str(fa)) == want
    fq = tmp_path / "bc.fq.gz"
    with gzip.open(fq, "wt") as f:
        f.write("@bc1\nACGTACGTacgt\n+\nIIIIIIIIIIII\n@bc2\nTTTTGGGG\n+\nIIIIIIII\n")
    assert cx.read_barcodes(str(fq)) == want[:2]
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    for p in (empty, tmp_path / "absent.fa"):
        with pytest.raises(OSError):
            cx.read_barcodes(str(p))


@pytest.mark.skipif(not os.path.exists(BIN), reason="host program not built")
def test_cli_usage_errors(tmp_path):
    """-d / -D without -B and a bad barcode file end the program before the
    input or a device is opened: the input named here does not exist."""
    good, bad_n, bad_len = tmp_path / "good.fa", tmp_path / "n.fa", tmp_path / "long.fa"
    good.write_text(">a\nACGTACGTACGTACGT\n")
    bad_n.write_text(">a\nACGTACGTNCGTACGT\n")
    bad_len.write_text(">a\n" + "ACGT" * 17 + "\n")
    absent_in, out = str(tmp_path / "absent.fa"), str(tmp_path / "out.fa")

    def run(*args):
        return subprocess.run([BIN, "-A", *args, absent_in, out], capture_output=True, timeout=60)

    for args in (("-d", str(tmp_path / "d")), ("-D", str(tmp_path / "t"))):
        r = run(*args)
        assert r.returncode == 1 and b"need a barcode file" in r.stderr
    for f in (bad_n, bad_len, tmp_path / "none.fa"):
        r = run("-B", str(f))
        assert r.returncode == 1 and b"is not a barcode file" in r.stderr
    for w in ("0", "257"):
        r = run("-B", str(good), "-W", w)
        assert r.returncode == 1 and b"-W" in r.stderr
    assert not os.path.exists(out)
    # a good set gets as far as the input
    r = run("-B", str(good))
    assert r.returncode == 1 and b"Failed to open infile" in r.stderr


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")] + \
        [os.path.join(ROOT, "ccsx_amd", "csrc", h) for h in ("ccsx_barcode.h", "ccsx_polish.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-DCCSX_BARCODE_NO_READER", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ccsx_amd", "csrc"), "-o", EXE] + srcs, check=True)
    return EXE


def test_barcode_host_clean_under_asan_ubsan(sanitized):
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized, "60"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, nz, assigned, refused = r.stdout.split()
    assert word == "ok" and int(nz) == 60 and int(refused) == 60 and int(assigned) > 0


@pytest.fixture(scope="module")
def accuracy():
    barcodes, pairs, zmws = bc.accuracy_case()
    poa = Poa()
    reads = []
    for subs in zmws:
        p = prepare(subs)
        reads.append(poa.zmw(p.seqs, p.offs, p.lens, 0))
    return barcodes, pairs, reads


def test_accuracy_every_zmw_assigned_to_its_pair(accuracy):
    barcodes, pairs, reads = accuracy
    for a in range(12):
        assert R.edit_distance(barcodes[a], R.revcomp(barcodes[a])) >= 7
        for b in range(a):
            assert R.edit_distance(barcodes[a], barcodes[b]) >= 7 and R.edit_distance(barcodes[a], R.revcomp(barcodes[b])) >= 7
    lens = [16] * 12
    leads, scores = [], []
    for (i0, i1), ccs in zip(pairs, reads):
        want = R.score(barcodes, ccs, 96)
        assert cx.barcode_host(barcodes, ccs, 96) == want
        call = R.call(want, lens, len(ccs))
        assert cx.barcode_call(want, lens, len(ccs)) == call
        leads += [e[1] - e[3] for e in want]
        scores += [e[1] for e in want]
        print(f"pair {(i0, i1)}: {want} -> {call}")
        assert call[3], (i0, i1, want, call)
        assert {want[0][0] >> 1, want[1][0] >> 1} == {i0, i1}
    print(f"smallest lead {min(leads)}, smallest score {min(scores)}")
