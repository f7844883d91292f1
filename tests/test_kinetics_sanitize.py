"""The host C++ of the consensus kinetics (SPEC.md §13) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU build: tools/kinetics_sanitize.cpp, a
stand-alone program, drives the BAM aux parser (block sizes down to 1 byte; well
formed, missing, miscounted and cut-short ip / pw arrays), ccsx_prepare_apply_kin,
ccsx_kinetics_tags and the kinetics output's bookkeeping in side_out.h under all
32 masks.  Only that program runs under the sanitizer; what it read must agree
with the product library's reader."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import ccsx_amd as cx

from .kinetics_cases import aux_array, names, rand_seqs, tagged_records, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "kinetics_sanitize")
SRCS = ["tools/kinetics_sanitize.cpp"] + [f"ccsx_amd/csrc/host/{f}.cpp" for f in
                                           ("ingest", "seqio", "prepare", "pairwise", "kinetics")]


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "ccsx_amd", "csrc", h) for h in ("side_out.h", "ccsx_layout.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "ccsx_amd", "csrc"), "-I", os.path.join(ROOT, "ccsx_amd", "csrc", "host"),
                        "-o", EXE] + srcs + ["-lz", "-lpthread"], check=True)
    return EXE


def _bams(tmp_path):
    rng = np.random.default_rng(21)
    lens = [700, 650, 1, 720, 690, 0, 710]
    good, _ = tagged_records(list(zip(names(1, lens), rand_seqs(rng, lens))), seed=1)
    frames, _ = tagged_records(list(zip(names(2, lens), rand_seqs(rng, lens))), seed=2, sub=b"S")
    bad, _ = tagged_records(list(zip(names(3, lens), rand_seqs(rng, lens))), seed=3)
    n = lens[0]
    cuts = [
        aux_array(b"ip", b"C", [1] * n),                                           # no pw
        aux_array(b"ip", b"C", [1] * n) + aux_array(b"pw", b"C", [2] * (n + 1)),   # a wrong count
        aux_array(b"ip", b"C", [1] * n) + aux_array(b"pw", b"S", [2] * 9, count=n),  # the array cut short
        aux_array(b"ip", b"C", [1] * n) + b"pwB",                                  # ... before its subtype
        aux_array(b"ip", b"C", [1] * n) + b"pwBC\x01\x00",                         # ... inside its count
        aux_array(b"ip", b"C", [1] * n) + aux_array(b"pw", b"C", [2] * 3, count=0xFFFFFFFF),
        aux_array(b"ip", b"C", [1] * n) + b"xxZno terminator",                     # a string without its NUL
        aux_array(b"ip", b"C", [1] * n) + b"pw",                                   # a tag without a type
        aux_array(b"ip", b"C", [1] * n) + b"yy?\x00",                              # an unknown type
        aux_array(b"ip", b"C", [1] * n) + b"pwBQ\x00\x00\x00\x00",                 # an unknown subtype
        aux_array(b"ip", b"S", [1] * n)[:-1] + aux_array(b"pw", b"C", [2] * n),    # a 16-bit array one byte short
    ]
    paths = []
    for j, recs in enumerate([good, frames] + [[(bad[0][0], bad[0][1], c)] + bad[1:] for c in cuts]):
        p = str(tmp_path / f"k{j}.bam")
        write_bam(p, recs)
        paths.append(p)
    return paths


def test_kinetics_host_code_clean_under_asan_ubsan(sanitized, tmp_path):
    paths = _bams(tmp_path)
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("ok") and "side outputs 32 masks" in r.stdout
    want, with_kin = [], 0
    for p in paths:
        for movie, hole, subs, ipd, pw in cx.read_zmws(p, True, kinetics=True):
            s = b"".join(subs)
            ci = zlib.crc32(b"".join(ipd)) if ipd is not None else 0
            cp = zlib.crc32(b"".join(pw)) if pw is not None else 0
            with_kin += ipd is not None
            want.append(f"{p} {movie}/{hole} {len(subs)} {len(s)} {zlib.crc32(s):08x} {ci:08x} {cp:08x}")
    assert with_kin == 2  # the two well-formed files; every damaged record drops its ZMW's kinetics
    assert [x for x in r.stdout.splitlines() if x.startswith(str(tmp_path))] == want
