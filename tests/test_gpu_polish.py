"""The polisher on the device (ccsx_polish.hip, ccsx_gpu_polish_*) against
tests/polish_ref.py, byte for byte: the constructed cases of
tests/polish_cases.py in one batch (bad maps among them), a batch cut into
several slices with one ZMW on the host, the engine's own drafts and maps of
synthetic ZMWs in both modes, and the host program's -p file."""
import os
import random
import subprocess

import pytest

import ccsx_amd as cx
from tests import polish_cases as pc
from tests import polish_ref as R
from tests.zmw_cases import synth
from tools.gen_synth import write

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")


@pytest.fixture(scope="module")
def polisher():
    p = cx.Polisher(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def constructed(polisher):
    """Every constructed case in one call: the bad maps sit among the others."""
    before = polisher.stats()
    got = polisher.polish([(ccs, segs, maps) for _, ccs, segs, maps, _ in pc.CASES])
    return got, before, polisher.stats()


@pytest.mark.parametrize("i", range(len(pc.CASES)), ids=pc.NAMES)
def test_constructed_equals_reference(constructed, i):
    want = pc.reference(i)
    assert want[4] == pc.CASES[i][4].get("status", 0)
    assert pc.same(constructed[0][i], want)


def test_constructed_stats(constructed):
    _, before, after = constructed
    d = {k: after[k] - before[k] for k in after}
    nbad = sum(1 for c in pc.CASES if c[4].get("status"))
    assert nbad == 2
    assert d == dict(zmws=len(pc.CASES), segments=sum(len(c[2]) for c in pc.CASES), slices=1, host_zmws=0, bad_maps=nbad)


def test_each_case_alone_equals_the_batch(polisher, constructed):
    """A ZMW's result does not depend on its neighbours in the slice (the
    counters and result words of a slice are zeroed per ZMW)."""
    for i in (0, 4, 12, len(pc.CASES) - 1):
        _, ccs, segs, maps, _ = pc.CASES[i]
        assert pc.same(polisher.polish([(ccs, segs, maps)])[0], constructed[0][i])


def test_slices_and_host_fallback():
    rng = random.Random(77)
    items = []
    for k in range(12):
        n = 2000 if k == 5 else 300
        d = pc.draft(500 + k, n)
        sm = [pc.noisy(rng, d) for _ in range(6 if k == 5 else 4)]
        items.append((d, [s for s, _ in sm], [m for _, m in sm]))
    # a 300-base ZMW of four segments takes ~55 kB of the arena, the 2,000-base one ~470 kB
    p = cx.Polisher(0, 200_000)
    try:
        got = p.polish(items)
        st = p.stats()
    finally:
        p.close()
    assert st["zmws"] == 12 and st["host_zmws"] == 1 and st["bad_maps"] == 0 and 3 <= st["slices"] <= 11
    for g, it in zip(got, items):
        assert pc.same(g, R.polish(*it))


@pytest.mark.parametrize("mode", [cx.MODE_SHRED, cx.MODE_PRIMITIVE])
def test_engine_drafts_and_maps(engine, polisher, mode):
    zs = [synth(h, 3000, 6) for h in range(3)]
    engine.set_base_map(True)
    try:
        res = engine.run(zs, mode)
        items = []
        for i, (z, (ccs, status, _)) in enumerate(zip(zs, res)):
            assert status == 0 and ccs
            segs = [z.seqs[int(o):int(o) + int(n)] for o, n in zip(z.offs, z.lens)]
            items.append((ccs, segs, engine.base_map(i)))
    finally:
        engine.set_base_map(False)
    got = polisher.polish(items)
    assert polisher.kernel_ms > 0
    for g, it in zip(got, items):
        want = R.polish(*it)
        assert want[4] == 0 and pc.same(g, want)
        for s, m in zip(it[1], g[3]):
            R.check_map_invariants(it[0], s, m)


@pytest.mark.parametrize("fastq", [False, True])
def test_cli_polish(tmp_path, engine, polisher, fastq):
    fa = str(tmp_path / "in.fa")
    write(fa, 12, 1500, 7)
    out_p, out_0, pol = str(tmp_path / "out_p"), str(tmp_path / "out_0"), str(tmp_path / "polished")
    # (an eighth of the device per context: the start-up reserves less)
    env = dict(os.environ, CCSX_DEV_SHARE="8")
    flags = ["-A", "-j", "2"] + (["-q"] if fastq else [])
    for extra, out in ((["-p", pol], out_p), ([], out_0)):
        r = subprocess.run([BIN] + flags + extra + [fa, out], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out_p, "rb").read() == open(out_0, "rb").read()
    # the Python path: prepare, the engine's draft and map, the polisher
    names, zs = [], []
    for movie, hole, subs in cx.read_zmws(fa, False):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        names.append(f"{movie}/{hole}/ccs/polished")
        zs.append(cx.prepare(subs))
    assert len(zs) == 12
    engine.set_base_map(True)
    try:
        res = engine.run(zs, cx.MODE_SHRED)
        items = [(ccs, [z.seqs[int(o):int(o) + int(n)] for o, n in zip(z.offs, z.lens)], engine.base_map(i))
                 for i, (z, (ccs, status, _)) in enumerate(zip(zs, res)) if status == 0 and ccs]
    finally:
        engine.set_base_map(False)
    assert len(items) == 12
    want = ""
    for name, (seq, qual, _, _, status) in zip(names, polisher.polish(items)):
        assert status == 0
        if fastq:
            want += f"@{name}\n{seq.decode()}\n+\n{bytes(q + 33 for q in qual).decode()}\n"
        else:
            want += f">{name}\n{seq.decode()}\n"
    assert open(pol).read() == want
