"""The resumable ccs_prepare (ccsx_prep_*) and the pairwise aligner's seed /
band split under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
build: tools/prepare_sanitize.cpp, a stand-alone program linked from
prepare.cpp and pairwise.cpp alone, drives them over synthetic ZMWs with
abnormal subreads, every request answered in full, and abandons walks while a
request is pending (the leak check).  Only that program runs under the
sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "prepare_sanitize")
SRCS = ["tools/prepare_sanitize.cpp"] + [f"ccsx_amd/csrc/host/{f}.cpp" for f in ("prepare", "pairwise")]


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", EXE] + srcs +
                       ["-lpthread"], check=True)
    return EXE


def test_resumable_prepare_clean_under_asan_ubsan(sanitized):
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized, "45"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, nz, requests, abandoned = r.stdout.split()
    # the abnormal paths ran.  Of every nine ZMWs three must ask at least once
    # whatever the random choices (the read-through, the one with N whose passes
    # are always fused, the one with two length groups): 15 requests over 45
    # ZMWs; the ZMWs 6, 24 and 42 (fused passes) are abandoned at their first
    # request
    assert word == "ok" and int(nz) == 45 and int(requests) >= 15 and int(abandoned) >= 3
