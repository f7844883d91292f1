"""ccsx_scan_host, ccsx_scan_start and ccsx_scan_cut (SPEC.md §17 on the host,
host/scan.cpp) against tests/scan_ref.py on the constructed cases, field for
field; what each case was built to reach; the invariant max_k G = score; the
host program's usage errors (no GPU is touched); the host functions under
AddressSanitizer + UndefinedBehaviorSanitizer (tools/scan_sanitize.cpp, a
stand-alone program; only that program runs under the sanitizer); and the
accuracy case through the oracle's CCS.

Accuracy, measured on the reference (scan_cases.accuracy_case, seed 7): every
read has exactly its two planted hits; the smallest score and the largest
deviation of start / end from the planted coordinates are printed by the test
and recorded in DESIGN.md §21."""
import os
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import Poa, prepare

from . import scan_cases as sc
from . import scan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ccsx_amd", "bin", "ccsx")
EXE = os.path.join(ROOT, "build", "scan_sanitize")
SRCS = ["tools/scan_sanitize.cpp", "ccsx_amd/csrc/host/scan.cpp"]


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=sc.NAMES)
def test_host_equals_reference(i):
    _, si, ccs, expect = sc.CASES[i]
    adapters, T = sc.SETS[si]
    want = sc.reference(i)
    assert cx.scan_host(adapters, ccs, T) == want
    # the situation the case was built for
    sc.check_expect(want, expect)
    # the start alone, and the invariant: the anchored maximum is the score
    for a, o, s, e, score in want:
        assert cx.scan_start(adapters[a], o, ccs, e) == (s, score) == R.start(adapters[a], o, ccs, e)
        assert 1 <= e - s < 1.5 * len(adapters[a])
    # the cut of the case's hits
    for lmin in (1, 50):
        assert cx.scan_cut(want, len(ccs), lmin) == R.cut(want, len(ccs), lmin)


def test_cases_reach_their_shapes():
    by = {c[0]: c for c in sc.CASES}
    n = lambda name: len(by[name][2])  # noqa: E731
    assert n("n0") == 0 and n("n1") == 1 and n("n_lt_L") < 25
    assert [n(f"n_{k}") for k in (sc.TC - 1, sc.TC, sc.TC + 1)] == [sc.TC - 1, sc.TC, sc.TC + 1]
    assert n("n_64_tiles") == 64 * sc.TC + 5 and n("n_64_tiles") // sc.TC + 1 > 64
    assert sc.NAMES.index("n1") < sc.NAMES.index("n0") < sc.NAMES.index("short_0") and by["n0"][1] == by["n1"][1]
    assert sum(n(f"short_{k}") // sc.TC + 1 for k in range(3)) == 3
    assert {len(s) for s, _ in sc.SETS} >= {1, 16, 64}
    assert sorted(len(a) for a in sc.MIXED) == [1, 8, 16, 25, 40, 64]
    assert {(max(len(a) for a in s) + 15) // 16 * 16 for s, _ in sc.SETS} == {16, 32, 48, 64}
    assert all(sc.WU[r] == -(-5 * r // 2) and sc.WU[r] % 8 == 0 for r in sc.WU) and sc.TC % 8 == 0
    assert sc.PAL == R.revcomp(sc.PAL) and R.revcomp(sc.HALF)[:12] == sc.HALF[-12:]
    # the long-span case: 35 read bases under a 25-base adapter
    h = [x for x in sc.reference(sc.NAMES.index("tile_long_span")) if x[3] == sc.TC + 2]
    assert h and h[0][3] - h[0][2] == 35 and h[0][4] == 5
    # the missed adapter: one hit, two pieces that are reverse complements of each other
    i = sc.NAMES.index("missed_adapter")
    ccs, hits = sc.CASES[i][2], sc.reference(i)
    (b0, e0, l0, r0), (b1, e1, l1, r1) = R.cut(hits, len(ccs))
    assert len(hits) == 1 and (l0, r0, l1, r1) == (-1, 0, 0, -1) and ccs[b0:e0] == R.revcomp(ccs[b1:e1])


@pytest.mark.parametrize("name", sorted(sc.REJECTED))
def test_rejected_sets(name):
    assert not R.set_ok(sc.REJECTED[name])
    with pytest.raises(ValueError):
        cx.scan_host(sc.REJECTED[name], b"ACGTACGTACGT")


@pytest.mark.parametrize("T", sc.REJECTED_T)
def test_rejected_thresholds(T):
    assert not R.set_ok([sc.A25], T)
    with pytest.raises(ValueError):
        cx.scan_host([sc.A25], b"ACGTACGTACGT", T)


@pytest.mark.parametrize("i", range(len(sc.CUTS)), ids=[c[0] for c in sc.CUTS])
def test_cut_equals_its_statement(i):
    _, hits, n, lmin, expect = sc.CUTS[i]
    assert R.cut(hits, n, lmin) == expect
    assert cx.scan_cut(hits, n, lmin) == expect


def test_tiled_tracks_equal_the_untiled_ones():
    """The tiling argument on the reference itself: a DP started WU columns
    before a tile from H(i, .) = -2 i gives the untiled bottom row from the
    tile's first column on, for every tile start of a tile-edge read."""
    for rows, si in sc.ROWS_SET.items():
        adapters = sc.SETS[si][0]
        ccs = sc.CASES[sc.NAMES.index(f"tile_misc_r{rows}")][2]
        y = R.codes(ccs)
        for x in R.patterns(adapters):
            full = R.matrix(x, y)[-1]
            for t0 in range(sc.TC, len(ccs) + 1, sc.TC):
                s = t0 - sc.WU[rows]
                part = R.matrix(x, y[s:t0 + sc.TC - 1])[-1]
                assert np.array_equal(part[t0 - s:], full[t0:t0 + sc.TC][:len(part) - (t0 - s)])


@pytest.mark.skipif(not os.path.exists(BIN), reason="host program not built")
def test_cli_usage_errors(tmp_path):
    """-i / -S / -E / -e without -I and a bad adapter file end the program
    before the input or a device is opened: the input named here does not exist."""
    good, bad_n, bad_len, many = (tmp_path / n for n in ("good.fa", "n.fa", "long.fa", "many.fa"))
    good.write_text(">a\nACGTACGTACGTACGTACGTACGTA\n")
    bad_n.write_text(">a\nACGTACGTNCGTACGT\n")
    bad_len.write_text(">a\n" + "ACGT" * 17 + "\n")
    many.write_text("".join(f">a{k}\nACGTACGTACGT\n" for k in range(65)))
    absent_in, out = str(tmp_path / "absent.fa"), str(tmp_path / "out.fa")

    def run(*args):
        return subprocess.run([BIN, "-A", *args, absent_in, out], capture_output=True, timeout=60)

    for args in (("-i", str(tmp_path / "i")), ("-S", str(tmp_path / "s")), ("-E", "80"), ("-e", "10")):
        r = run(*args)
        assert r.returncode == 1 and b"need an adapter file" in r.stderr
    for f in (bad_n, bad_len, many, tmp_path / "none.fa"):
        r = run("-I", str(f))
        assert r.returncode == 1 and b"is not an adapter file" in r.stderr
    for t in ("0", "101"):
        r = run("-I", str(good), "-E", t)
        assert r.returncode == 1 and b"-E" in r.stderr
    r = run("-I", str(good), "-e", "-1")
    assert r.returncode == 1 and b"-e" in r.stderr
    assert not os.path.exists(out)
    # a good set gets as far as the input
    r = run("-I", str(good))
    assert r.returncode == 1 and b"Failed to open infile" in r.stderr


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")] + \
        [os.path.join(ROOT, "ccsx_amd", "csrc", h) for h in ("ccsx_scan.h", "ccsx_polish.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ccsx_amd", "csrc"), "-o", EXE] + srcs, check=True)
    return EXE


def test_scan_host_clean_under_asan_ubsan(sanitized):
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized, "60"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, nz, nhits, refused = r.stdout.split()
    assert word == "ok" and int(nz) == 60 and int(refused) == 60 and int(nhits) > 0


@pytest.fixture(scope="module")
def accuracy():
    adapters, pairs, zmws = sc.accuracy_case()
    poa = Poa()
    reads = []
    for subs in zmws:
        p = prepare(subs)
        reads.append(poa.zmw(p.seqs, p.offs, p.lens, 0))
    return adapters, pairs, reads


def planted(ccs: bytes, what: bytes) -> tuple:
    """[b, e) of the CCS bases closest to `what` (the planted adapter as the
    CCS shows it): the best semi-global placement by edit distance."""
    best = None
    for b in range(len(ccs) - len(what) + 1):
        d = sum(x != y for x, y in zip(ccs[b:b + len(what)], what))
        if best is None or d < best[0]:
            best = (d, b)
    return best[1], best[1] + len(what)


def test_accuracy_two_planted_hits_per_read(accuracy):
    adapters, pairs, reads = accuracy
    for a in range(3):
        assert R.edit_distance(adapters[a], R.revcomp(adapters[a])) >= 9
        for b in range(a):
            assert R.edit_distance(adapters[a], adapters[b]) >= 9 and R.edit_distance(adapters[a], R.revcomp(adapters[b])) >= 9
    scores, devs, tdevs = [], [], []
    for (i, j), ccs in zip(pairs, reads):
        want = R.hits(adapters, ccs)
        assert cx.scan_host(adapters, ccs) == want
        print(f"pair {(i, j)}: n = {len(ccs)}, {want}")
        # exactly the two planted hits, in order, the second reverse-complemented
        assert [h[:2] for h in want] == [(i, 0), (j, 1)], want
        for h, what, tb in zip(want, (adapters[i], R.revcomp(adapters[j])), (300, 625)):
            b, e = planted(ccs, what)
            assert h[2] < e and b < h[3], (h, b, e)
            scores.append(h[4])
            devs += [abs(h[2] - b), abs(h[3] - e)]
            tdevs += [abs(h[2] - tb), abs(h[3] - tb - 25)]  # (the template's coordinates: the CCS's indels move them)
        pieces = R.cut(want, len(ccs))
        assert cx.scan_cut(want, len(ccs)) == pieces and len(pieces) == 3
        assert [(p[2], p[3]) for p in pieces] == [(-1, 0), (0, 1), (1, -1)]
    print(f"smallest score {min(scores)}, largest deviation of start / end from the adapter in the CCS {max(devs)}, "
          f"from the template's coordinates {max(tdevs)}")
