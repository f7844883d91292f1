"""ccsx_polish_host (SPEC.md §15 as a sequential loop, host/polish.cpp) against
tests/polish_ref.py on the constructed cases, byte for byte; §11's invariants
on every realigned map; what each case was built to reach; the host function
under AddressSanitizer + UndefinedBehaviorSanitizer (tools/polish_sanitize.cpp,
a stand-alone program; only that program runs under the sanitizer); and the
accuracy case: polishing must beat the draft on the synthetic truth.

Accuracy, measured on this reference (random.Random(1), 5 ZMWs of 2,000 bases,
8 subreads at 2 / 4 / 4 % with the last cut in half, shredded mode): the draft's
mean edit identity and the polished reads' are printed by the test and recorded
in DESIGN.md §19."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import Prepared, edit_identity

from . import basemap_ref as br
from . import polish_cases as pc
from . import polish_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "polish_sanitize")
SRCS = ["tools/polish_sanitize.cpp", "ccsx_amd/csrc/host/polish.cpp"]


@pytest.mark.parametrize("i", range(len(pc.CASES)), ids=pc.NAMES)
def test_host_equals_reference(i):
    _, ccs, segs, maps, expect = pc.CASES[i]
    want = pc.reference(i)
    got = cx.polish_host(ccs, segs, maps)
    assert pc.same(got, want)
    assert want[4] == expect.get("status", 0)
    if want[4] == 0:
        for s, m in zip(segs, got[3]):
            if ccs:
                R.check_map_invariants(ccs, s, m)
    # the situation the case was built for
    if "counts" in expect:
        assert tuple(want[2]) == expect["counts"]
    if "seq" in expect:
        assert want[0] == expect["seq"]
    if "tail" in expect:
        ts, tq = expect["tail"]
        assert want[0].endswith(ts) and want[1].endswith(tq)


def test_cases_reach_their_shapes():
    """The constructed maps do produce the pieces and shifts they are named for."""
    by = {c[0]: c for c in pc.CASES}

    def lo(name, k=0):
        _, ccs, _, maps, _ = by[name]
        return np.clip((maps[k].astype(np.int64) & R.OFFSET) - R.HALF, 0, max(len(ccs) - R.W, 0))

    assert set(np.diff(lo("shifts")).tolist()) >= {0, 1, 63}
    assert (np.diff(lo("break64")) >= 64).sum() == 1 and 64 in np.diff(lo("break64")).tolist()
    assert (np.diff(lo("break300")) >= 64).sum() == 2 and 300 in np.diff(lo("break300")).tolist()
    assert (np.diff(lo("onerow")) >= 64).sum() == 3
    assert (lo("tail200") == 200 - 64).all() and (lo("tail65") == 1).all()
    assert len(by["nseg70"][2]) == 70


@pytest.fixture(scope="module")
def sanitized():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    srcs = [os.path.join(ROOT, s) for s in SRCS]
    deps = srcs + [os.path.join(ROOT, "include", h) for h in ("ccsx_host.h", "ccsx_gpu.h")] + \
        [os.path.join(ROOT, "ccsx_amd", "csrc", h) for h in ("ccsx_polish.h", "ccsx_layout.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "ccsx_amd", "csrc"), "-o", EXE] + srcs, check=True)
    return EXE


def test_polish_host_clean_under_asan_ubsan(sanitized):
    # (verify_asan_link_order=0: the run's environment may preload a library
    # ahead of the ASan runtime)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sanitized, "40"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-3000:]
    word, nz, bad, pieces = r.stdout.split()
    # every fourth ZMW has a bad map; the jumping maps gave more pieces than segments
    assert word == "ok" and int(nz) == 40 and int(bad) == 10 and int(pieces) > 0


def test_polish_improves_on_the_draft():
    rng = random.Random(1)
    draft_id, pol_id = [], []
    for _ in range(5):
        ins = bytes(rng.choice(b"ACGT") for _ in range(2000))
        subs = [R.mutate(rng, ins, .02, .04, .04) for _ in range(8)]
        subs[-1] = subs[-1][:len(subs[-1]) // 2]
        lens = np.array([len(s) for s in subs], np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
        ccs, maps = br.reference(Prepared(b"".join(subs), offs, lens), 0)
        want = R.polish(ccs, subs, maps)
        got = cx.polish_host(ccs, subs, maps)
        assert pc.same(got, want) and want[4] == 0
        for s, m in zip(subs, got[3]):
            R.check_map_invariants(ccs, s, m)
        draft_id.append(edit_identity(ccs, ins))
        pol_id.append(edit_identity(got[0], ins))
    d, p = float(np.mean(draft_id)), float(np.mean(pol_id))
    print(f"draft identity {d:.5f} -> polished {p:.5f}; per ZMW {draft_id} -> {pol_id}")
    assert p > d
