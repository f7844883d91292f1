"""The engine's six optional outputs (qualities, pass records, subread-to-CCS
map, strand pileup, consensus kinetics, per-strand consensus) in every
combination: each of the 64 subsets through run(), submit() / collect() with a
full-capacity re-run inside collect, and stage() / launch() / fetch(), on the
batch of tests/test_gpu_side_outputs.py (which keeps the 32 subsets of the first
five).  Every enabled output is compared exactly with its reference, every
disabled one is refused with its "ran with ... off" text, the CCS is the
oracle's, and the sizes of every subset are the empty subset's plus the
documented term of each enabled output."""
import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from tests import basemap_ref as br
from tests import kinetics_ref as kr
from tests import pass_ref as pr
from tests import pileup_ref as pu
from tests import quality_ref as qr
from tests import strand_ref as sr
from tests.kinetics_cases import with_kin
from tests.pileup_cases import edge
from tests.test_gpu_side_outputs import FAILED as FAILED5
from tests.test_gpu_side_outputs import OFF as OFF5
from tests.test_gpu_side_outputs import _outcap, _small, _terms
from tests.zmw_cases import synth

pytestmark = pytest.mark.gpu

NAMES = ("quality", "pass_stats", "base_map", "pileup", "kinetics", "by_strand")
SUBSETS = [tuple(n for k, n in enumerate(NAMES) if m >> k & 1) for m in range(64)]
OFF = dict(OFF5, by_strand="ran with the by-strand output off")
FAILED = dict(FAILED5, by_strand="that ZMW failed: it has no strand consensus")


def _ids(subset):
    return "+".join(subset) or "none"


def _terms6(z):
    return dict(_terms(z), by_strand=4 * _outcap(z) + len(z.lens) + 8)


@pytest.fixture(scope="module")
def zs():
    tiny, three, prepared = _small()
    zs = [synth(9100, 1500, 6), synth(9101, 1500, 6), edge()["ragged_lengths"], tiny, three, prepared]
    assert sum(_outcap(z) for z in zs) % 8
    return [with_kin(z, seed=j) for j, z in enumerate(zs)]


_REFS = {}


def _refs(zs, mode):
    """The oracle's CCS and the six references of the batch, once per mode."""
    if mode not in _REFS:
        s = [sr.reference(z, mode) for z in zs]
        _REFS[mode] = {"ccs": batch(zs, mode, 8)[0],
                       "quality": [qr.reference(z, mode)[1] for z in zs],
                       "pass_stats": [pr.reference(z, mode)[1] for z in zs],
                       "base_map": [br.reference(z, mode)[1] for z in zs],
                       "pileup": [pu.reference(z, mode)[1] for z in zs],
                       "kinetics": [kr.reference(z, mode)[1] for z in zs],
                       "by_strand": [(r.seq[0], r.qual[0], r.seq[1], r.qual[1]) for r in s]}
    return _REFS[mode]


def _apply(engine, subset):
    for n in NAMES:
        getattr(engine, "set_" + n)(n in subset)


@pytest.fixture
def sengine(engine):
    """The shared engine; every output, forced capacity and hook is switched
    back off afterwards."""
    try:
        yield engine
    finally:
        _apply(engine, ())
        engine.set_tight_out(0)
        engine.set_fault(-1)


def _same(name, got, want):
    if name == "quality":
        return got == want
    if name == "base_map":
        return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    if name == "by_strand":
        return got[0] == want[0] and got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    return got.shape == want.shape and np.array_equal(got, want)


def _check(engine, ref, subset, got, slot=-1, failed=None):
    """got = [(ccs, status, cells)] or None (the call raised: outputs only)."""
    for i in range(len(ref["ccs"])):
        if i == failed:
            assert got is None or (got[i][1] != 0 and got[i][0] == b"")
        elif got is not None:
            assert got[i][1] == 0 and got[i][0] == ref["ccs"][i], f"ZMW {i}: CCS differs from the oracle"
        for n in NAMES:
            read = getattr(engine, n)
            if n not in subset:
                with pytest.raises(cx.GpuError, match=OFF[n]):
                    read(i, slot)
            elif i == failed and n == "quality":
                assert read(i, slot) == b""
            elif i == failed:
                with pytest.raises(cx.GpuError, match=FAILED[n]):
                    read(i, slot)
            else:
                assert _same(n, read(i, slot), ref[n][i]), f"ZMW {i}: {n} differs from the reference"


@pytest.mark.parametrize("subset", SUBSETS, ids=_ids)
def test_every_subset(sengine, zs, subset):
    ref = _refs(zs, cx.MODE_SHRED)
    _apply(sengine, subset)
    # 1. run(): shredded, and -P for the full and the empty set
    _check(sengine, ref, subset, sengine.run(zs, cx.MODE_SHRED))
    if len(subset) in (0, 6):
        _check(sengine, _refs(zs, cx.MODE_PRIMITIVE), subset, sengine.run(zs, cx.MODE_PRIMITIVE))
    # 2. submit() / collect(), every CCS beyond 64 bytes re-run inside collect;
    # the settings flipped in between: the batch keeps those of its submit, and
    # collect leaves the context's as it found them
    others = tuple(n for n in NAMES if n not in subset)
    sengine.set_tight_out(64)
    before = sengine.rerun_count()
    slot = sengine.submit(zs, cx.MODE_SHRED)
    _apply(sengine, others)
    got = sengine.collect(slot)
    sengine.set_tight_out(0)
    left = sengine.zmw_bytes(zs[0])  # (under the settings collect left)
    assert sengine.rerun_count() - before >= 4
    _check(sengine, ref, subset, got, slot)
    _apply(sengine, ())
    assert left == sengine.zmw_bytes(zs[0]) + sum(_terms6(zs[0])[n] for n in others)
    # 3. stage() / launch() / fetch()
    _apply(sengine, subset)
    sengine.stage(zs, cx.MODE_SHRED)
    sengine.launch(cx.MODE_SHRED)
    _check(sengine, ref, subset, sengine.fetch())


@pytest.mark.parametrize("path", ["run", "submit"])
def test_failed_zmw_in_every_output(sengine, zs, path):
    """set_fault(1) with all six on: ZMW 1 reads as an empty quality and is
    refused by the other five; every other ZMW is exact."""
    ref = _refs(zs, cx.MODE_SHRED)
    _apply(sengine, NAMES)
    sengine.set_fault(1)
    if path == "run":
        with pytest.raises(cx.GpuError):
            sengine.run(zs, cx.MODE_SHRED)
        _check(sengine, ref, NAMES, None, -1, failed=1)
    else:
        slot = sengine.submit(zs, cx.MODE_SHRED)
        _check(sengine, ref, NAMES, sengine.collect(slot), slot, failed=1)


def test_sizes_of_every_subset(sengine, zs):
    """zmw_bytes and staged_bytes of each subset: the empty subset's plus the
    documented term of each enabled output."""
    sizes = {}
    for subset in SUBSETS:
        _apply(sengine, subset)
        per = [(sengine.zmw_bytes(z, cx.MODE_SHRED), sengine.zmw_bytes(z, cx.MODE_PRIMITIVE)) for z in zs]
        sengine.stage(zs, cx.MODE_SHRED)
        sizes[subset] = per, sengine.staged_bytes()
    per0, staged0 = sizes[()]
    for subset in SUBSETS:
        add = [sum(_terms6(z)[n] for n in subset) for z in zs]
        per, staged = sizes[subset]
        assert per == [(a + x, b + x) for (a, b), x in zip(per0, add)], _ids(subset)
        assert staged == staged0 + sum(add), _ids(subset)
