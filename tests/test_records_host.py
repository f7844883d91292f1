"""The host program's record formatters (ccsx_amd/csrc/host/records.cpp) on the
CPU, through tools/records_sanitize.cpp, a stand-alone program built with
AddressSanitizer + UndefinedBehaviorSanitizer (only that program runs under
the sanitizers; no HIP code is involved):

* every formatter on constructed inputs with the edges its code branches on,
  each text compared inside the program with the one written out there;
* the -d / -D / -i / -S texts of a dozen synthetic reads of 200-600 bases,
  FASTA and FASTQ, byte for byte against tests/stage_format.py driven by the
  Python references (tests/barcode_ref.py, tests/scan_ref.py)."""
import os
import random
import subprocess

import pytest

from . import barcode_ref as BR
from . import scan_ref as SR
from . import stage_cases as st
from . import stage_format as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ccsx_amd", "csrc", "host")
EXE = os.path.join(ROOT, "build", "records_sanitize")
SRCS = ["tools/records_sanitize.cpp"] + [f"ccsx_amd/csrc/host/{f}.cpp" for f in
                                          ("records", "barcode", "scan", "quality", "passstat", "basemap", "pileup",
                                           "kinetics", "prepare", "pairwise", "ingest", "seqio")]
# (verify_asan_link_order=0: the run's environment may preload a library ahead of the ASan runtime)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
           UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(HOST, h) for h in ("records.h", "ingest.h")] + \
        [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "ccsx_amd", "csrc"), "-I", HOST, "-o", EXE] + srcs + ["-lz", "-lpthread"],
                       check=True)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, n = r.stdout.split()
    assert word == "ok"
    return int(n)


def test_formatters_on_constructed_inputs(sanitized):
    assert run(sanitized) >= 25


def family():
    """(barcodes, adapters, [(name, bases)]): twelve reads of 200-600 bases.
    Read k has a barcode at both ends (k % 4 in (0, 3)), at its start only
    (k % 4 == 1) or at neither (k % 4 == 2); and inside no adapter (k % 3 == 0),
    one (k % 3 == 1) or two adjacent ones in opposite orientations (k % 3 == 2)."""
    bcs, ads, _ = st.family()
    rng = random.Random(5)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))  # noqa: E731
    reads = []
    for k in range(12):
        body = rnd(168 + 36 * k)
        if k % 3 == 1:
            body = body[:80] + ads[k % len(ads)] + body[105:]
        if k % 3 == 2:
            body = body[:90] + ads[k % len(ads)] + BR.revcomp(ads[(k + 1) % len(ads)]) + body[140:]
        left = bcs[k % 12] if k % 4 != 2 else rnd(16)
        right = BR.revcomp(bcs[(5 * k + 1) % 12]) if k % 4 in (0, 3) else rnd(16)
        reads.append((f"syn/{k}/ccs", left + body + right))
    return bcs, ads, reads


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("records")
    bcs, ads, reads = family()
    bfa, afa = str(d / "bc.fa"), str(d / "ad.fa")
    for path, names, seqs in ((bfa, st.BC_NAMES, bcs), (afa, st.AD_NAMES, ads)):
        with open(path, "w") as f:
            f.write("".join(f">{nm} of the set\n{s.decode()}\n" for nm, s in zip(names, seqs)))
    rng = random.Random(6)
    recs = {False: [(name, seq.decode(), None) for name, seq in reads],
            True: [(f"{name} np={5 + k} rq={0.99 + k / 2000:.6f}", seq.decode(),
                    "".join(chr(33 + rng.randrange(2, 94)) for _ in seq)) for k, (name, seq) in enumerate(reads)]}
    paths = {}
    for fastq, rs in recs.items():
        paths[fastq] = str(d / ("reads.fq" if fastq else "reads.fa"))
        with open(paths[fastq], "w") as f:
            for head, seq, qual in rs:
                f.write(f"@{head}\n{seq}\n+\n{qual}\n" if fastq else f">{head}\n{seq}\n")
    return d, bfa, afa, recs, paths


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_stage_files_equal_the_references(sanitized, inputs, fastq):
    d, bfa, afa, recs, paths = inputs
    bcs, ads, reads = family()
    assert all(200 <= len(seq) <= 600 for _, seq in reads)
    want_d, want_D, rows = F.demux_files(recs[fastq], bcs, st.BC_NAMES, fastq, BR.score, BR.call)
    want_i, want_S, found = F.scan_files(recs[fastq], ads, st.AD_NAMES, fastq, SR.hits, SR.cut)
    # the family reaches what the comparison is for
    assert any(c[3] for _, c in rows) and any(not c[3] for _, c in rows)
    assert any(found) and any(not hs for hs in found)
    assert any(len(SR.cut(hs, len(seq))) >= 2 for hs, (_, seq) in zip(found, reads))
    prefix = str(d / ("q" if fastq else "a"))
    assert run(sanitized, paths[fastq], bfa, afa, prefix) == len(reads)
    for ext, want in ((".d", want_d), (".D", want_D), (".i", want_i), (".S", want_S)):
        with open(prefix + ext, "rb") as f:
            assert f.read() == want.encode(), ext
