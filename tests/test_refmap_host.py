"""ccsx_ref_set_make, ccsx_ref_host and ccsx_ref_pass (SPEC.md §18 on the host,
host/refmap.cpp) against tests/refmap_ref.py on the constructed cases, field
for field and word for word; what each case was built to reach; the winner's d0
against ccsx_pairwise_seed and its ten fields against ccsx_pairwise_band on
that pair; §18's identities between the words' CIGAR (ccsx_map_cigar) and the
record; the report rule at its thresholds; the sets that are none; the host
program's usage errors (no GPU is touched); the host functions under
AddressSanitizer + UndefinedBehaviorSanitizer (tools/refmap_sanitize.cpp, a
stand-alone program; only that program runs under the sanitizer); and the
accuracy case through the oracle's CCS.

Accuracy, measured on the reference (refmap_cases.accuracy_case, seed 0, the
first seed tried: the reference maps 12 of 12 reads to the planted target and
strand, [tb, te) overlapping the planted stretch, all 12 passing the defaults):
the smallest identity mat / aln and the largest deviation of tb / te from the
planted stretch are printed by the test and recorded in DESIGN.md §22, not
asserted."""
import os
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import Poa, prepare

from . import refmap_cases as rc
from . import refmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ccsx_amd", "bin", "ccsx")
EXE = os.path.join(ROOT, "build", "refmap_sanitize")
SRCS = ["tools/refmap_sanitize.cpp", "ccsx_amd/csrc/host/refmap.cpp", "ccsx_amd/csrc/host/pairwise.cpp",
        "ccsx_amd/csrc/host/basemap.cpp"]
F = {n: k for k, n in enumerate(cx.REF_FIELDS)}


@pytest.fixture(scope="module")
def sets():
    return [cx.RefSet(s) for s in rc.SETS]


@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.NAMES)
def test_host_equals_reference(sets, i):
    _, si, read, expect = rc.CASES[i]
    want, want_words = rc.reference(i)
    got, words = cx.ref_host(sets[si], read)
    assert got == want
    assert np.array_equal(words, want_words)
    assert cx.ref_host(sets[si], read, words=False) == (want, None)
    # the situation the case was built for
    rc.check_expect(want, expect)
    if want[0] < 0:
        assert want == R.UNMAPPED and (words == R.INS).all() and not cx.ref_pass(want, 0, 0)
        return
    # the winner's pair by the pairwise aligner's two halves
    g, o, d0 = want[:3]
    q = bytes(R.read_codes(R.revcomp(read) if o else read))
    t = bytes(R.target_codes(rc.SETS[si][g]))
    assert cx.pairwise_seed(q, t) == d0
    band = cx.pairwise_band(q, t, d0)
    assert tuple(band[k] for k in ("qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln", "score")) == want[5:]
    # §18's identities: the words' CIGAR is the record
    aln = cx.map_cigar(words)
    assert aln is not None
    assert (aln["qs"], aln["qe"], aln["ts"], aln["te"], aln["n_eq"], aln["n_x"], aln["n_ins"], aln["n_del"]) == want[5:13]
    ref = R.cigar(want_words, len(read))
    assert aln["cigar"] == ref[8] and ref[:8] == want[5:13]
    offs = words & 0x3FFFFFFF
    assert (np.diff(offs.astype(np.int64)) >= 0).all()


def test_cases_reach_their_shapes():
    by = {c[0]: c for c in rc.CASES}
    n = lambda name: len(by[name][2])  # noqa: E731
    assert (n("n0"), n("n12"), n("n13")) == (0, 12, 13) and len(rc.SETS[1][0]) == 13
    assert [n(f"n_{k}") for k in (31, 32, 33, 63, 64, 65, 127, 128, 129)] == [31, 32, 33, 63, 64, 65, 127, 128, 129]
    assert 19990 <= n("long_20000") <= 20010
    assert rc.PAL == R.revcomp(rc.PAL)
    # the occurrence cap: in U x 64 the 13-mers at offsets 0..7 of the unit occur 64 times, in U x 65 65 times
    for reps, kept in ((64, 20), (65, 12)):
        t = R.target_codes(rc.U * reps)
        occ: dict = {}
        for _, h in R.kmers(t):
            occ[h] = occ.get(h, 0) + 1
        assert len(occ) == 20 and max(occ.values()) == reps and sum(1 for v in occ.values() if v <= R.OCC) == kept
    # 40 occurrences in each of two targets
    for t in rc.SETS[6]:
        occ = {}
        for _, h in R.kmers(R.target_codes(t)):
            occ[h] = occ.get(h, 0) + 1
        assert max(occ.values()) == 40
    # the tie of two bins, and the votes of the two near-copy targets
    _, _, pairs = R.record(rc.SETS[0], by["two_bins_tie"][2], with_votes=True)
    v = R.seed(R.read_codes(by["two_bins_tie"][2]), R.target_codes(rc.T0))
    assert v == {3: 18, 4: 18} and pairs[(0, 0)] == (18, 3)
    # the band-edge cases: no vote at the diagonal of the alignment
    for name, d in (("band_first_cells", 112), ("band_last_cells", 624)):
        v = R.seed(R.read_codes(by[name][2]), R.target_codes(rc.T0))
        assert d // 32 not in v and max(v, key=v.get) == 368 // 32


@pytest.mark.parametrize("name", sorted(rc.REJECTED))
def test_rejected_sets(name):
    assert not R.set_ok(rc.REJECTED[name])
    with pytest.raises(ValueError):
        cx.RefSet(rc.REJECTED[name])
    with pytest.raises(ValueError):
        cx.ref_host(rc.REJECTED[name], b"ACGTACGTACGTACGT")


def test_accepted_edge_sets():
    for refs in ([b"N" * 13], [rc.rnd(50, 13)] * 64, [b"acgtnACGTNryk" * 2], [b"A" * (1 << 20)]):
        assert R.set_ok(refs)
        cx.RefSet(refs)


def test_ref_pass_at_its_thresholds():
    def rec(mat, aln, g=0):
        r = [0] * 15
        r[F["g"]], r[F["mat"]], r[F["aln"]] = g, mat, aln
        return tuple(r)
    for r, y, Y, want in ((rec(75, 100), 50, 75, True), (rec(74, 100), 50, 75, False), (rec(50, 50), 50, 75, True),
                          (rec(49, 49), 50, 75, False), (rec(38, 50), 50, 75, True), (rec(37, 50), 50, 75, False),
                          (rec(100, 100, g=-1), 0, 0, False), (rec(1, 1), 0, 100, True), (rec(0, 1), 0, 0, True),
                          (rec(21474837, 21474837 + 1), 0, 100, False)):
        assert cx.ref_pass(r, y, Y) is want is R.passes(r, y, Y), (r, y, Y)
    assert cx.ref_pass(rec(80, 100)) and not cx.ref_pass(R.UNMAPPED)


@pytest.mark.skipif(not os.path.exists(BIN), reason="host program not built")
def test_cli_usage_errors(tmp_path):
    """-g / -Y / -y without -G and a bad reference file end the program before
    the input or a device is opened: the input named here does not exist."""
    good, short, digit, many, big = (tmp_path / n for n in ("good.fa", "short.fa", "digit.fa", "many.fa", "big.fa"))
    good.write_text(">t0\nACGTACGTNACGTACGTTTGA\n>t1\nacgtacgtacgta\n")
    short.write_text(">t0\nACGTACGTACGT\n")
    digit.write_text(">t0\nACGTACGTACGT1ACGTACGT\n")
    many.write_text("".join(f">t{k}\nACGTACGTACGTA\n" for k in range(65)))
    big.write_text(">t0\n" + "A" * ((1 << 20) + 1) + "\n")
    absent_in, out = str(tmp_path / "absent.fa"), str(tmp_path / "out.fa")

    def run(*args):
        return subprocess.run([BIN, "-A", *args, absent_in, out], capture_output=True, timeout=60)

    for args in (("-g", str(tmp_path / "g")), ("-Y", "80"), ("-y", "10")):
        r = run(*args)
        assert r.returncode == 1 and b"need a reference file" in r.stderr
    for f in (short, digit, many, big, tmp_path / "none.fa"):
        r = run("-G", str(f))
        assert r.returncode == 1 and b"is not a reference file" in r.stderr
    for v in ("-1", "101"):
        r = run("-G", str(good), "-Y", v)
        assert r.returncode == 1 and b"-Y" in r.stderr
    r = run("-G", str(good), "-y", "-1")
    assert r.returncode == 1 and b"-y" in r.stderr
    # -G is checked first: a bad reference file is named before a bad barcode file
    r = run("-B", str(short), "-G", str(short))
    assert r.returncode == 1 and b"is not a reference file" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "g")
    # a good set gets as far as the input
    r = run("-G", str(good), "-g", str(tmp_path / "g"))
    assert r.returncode == 1 and b"Failed to open infile" in r.stderr
    assert cx.read_refs(str(good)) == [("t0", b"ACGTACGTNACGTACGTTTGA"), ("t1", b"acgtacgtacgta")]


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")] + \
        [os.path.join(ROOT, "ccsx_amd", "csrc", h) for h in ("ccsx_ref.h", "ccsx_align.h", "ccsx_polish.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ccsx_amd", "csrc"), "-o", EXE] + srcs, check=True)
    return EXE


def test_ref_host_clean_under_asan_ubsan(sanitized):
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized, "60"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, nz, mapped, refused = r.stdout.split()
    assert word == "ok" and int(nz) == 60 and int(refused) == 240 and int(mapped) >= 20


def check_accuracy(targets, planted, reads, records):
    """§18's condition on the records of the accuracy case's reads; prints the
    identities and the coordinates' deviations."""
    ident, devs = [], []
    for (g, o, b), ccs, rec in zip(planted, reads, records):
        r = dict(zip(cx.REF_FIELDS, rec))
        print(f"planted {(g, o, b)}: n = {len(ccs)}, {r}")
        assert (r["g"], r["o"]) == (g, o), (r, g, o)
        assert r["tb"] < b + 400 and b < r["te"]
        assert R.passes(rec) and cx.ref_pass(rec)
        ident.append(r["mat"] / r["aln"])
        devs += [abs(r["tb"] - b), abs(r["te"] - b - 400)]
    print(f"smallest identity {min(ident):.4f}, largest deviation of tb / te from the planted stretch {max(devs)}")


def test_accuracy_planted_target_and_strand():
    targets, planted, zmws = rc.accuracy_case(rc.ACCURACY_SEED)
    assert rc.ACCURACY_SEED == 0 and sorted({o for _, o, _ in planted}) == [0, 1]
    poa = Poa()
    reads = []
    for subs in zmws:
        p = prepare(subs)
        reads.append(poa.zmw(p.seqs, p.offs, p.lens, 0))
    want = [R.record(targets, ccs)[0] for ccs in reads]
    check_accuracy(targets, planted, reads, want)
    rs = cx.RefSet(targets)
    assert [cx.ref_host(rs, ccs)[0] for ccs in reads] == want
