"""The engine's five optional outputs (qualities, pass records, subread-to-CCS
map, strand pileup, consensus kinetics) in every combination: each of the 32
subsets through run(), submit() / collect() with a full-capacity re-run inside
collect, and stage() / launch() / fetch().  Every enabled output is compared
exactly with its reference (tests/*_ref.py), every disabled one is refused with
its "ran with ... off" text, and the CCS is the oracle's.  The per-feature files
test each output through every kernel object and path; this one tests that the
outputs do not disturb each other in the host engine's shared bookkeeping, nor
in the one side-output kernel that writes whichever of them are on: subsets of
them on every kernel object and on the HBM-read instance."""
import random

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from tests import basemap_ref as br
from tests import kinetics_ref as kr
from tests import pass_ref as pr
from tests import pileup_ref as pu
from tests import quality_ref as qr
from tests.kinetics_cases import with_kin
from tests.pileup_cases import alternating, edge, with_rev
from tests.zmw_cases import edge_cases, mutate, raw, synth

pytestmark = pytest.mark.gpu

NAMES = ("quality", "pass_stats", "base_map", "pileup", "kinetics")
SUBSETS = [tuple(n for k, n in enumerate(NAMES) if m >> k & 1) for m in range(32)]
OFF = {"quality": "ran with quality off", "pass_stats": "ran with pass statistics off",
       "base_map": "ran with the base map off", "pileup": "ran with the pileup off", "kinetics": "ran with kinetics off"}
FAILED = {"pass_stats": "that ZMW failed: it has no pass statistics", "base_map": "that ZMW failed: it has no base map",
          "pileup": "that ZMW failed: it has no pileup", "kinetics": "that ZMW failed: it has no kinetics"}


def _ids(subset):
    return "+".join(subset) or "none"


def _outcap(z):
    # ccsx_layout.h zcaps, tight caps: min(S + 16, 2 x longest segment + 1,024)
    lens = [int(x) for x in z.lens]
    return min(sum(lens) + 16, 2 * max(lens) + 1024)


def _terms(z):
    """The bytes each output adds to a ZMW, as include/ccsx_gpu.h documents them."""
    S, n = sum(int(x) for x in z.lens), len(z.lens)
    return {"quality": _outcap(z), "pass_stats": 24 * n, "base_map": 4 * S, "pileup": 12 * _outcap(z) + n,
            "kinetics": 8 * _outcap(z) + 2 * S + n}


def _small():
    """The 49-base ZMW, the three-read ZMW and what ccs_prepare makes of the
    former's reads, with strand flags."""
    rng = random.Random(9100)
    T = bytes(rng.choice(b"ACGT") for _ in range(400))
    # 49 bases in five segments: an odd slab of 65 bytes, so the planes behind
    # the slabs need padding.  (Pushed as they are: ccs_prepare keeps only the
    # four 10-base subreads of this input, 40 bases and an even slab; that ZMW
    # is in the batch too.)
    reads = [b"ACGTACGTA"] + [b"ACGTACGTAC"] * 4
    tiny = with_rev(raw(reads), alternating(5))
    assert sum(int(x) for x in tiny.lens) == 49 and _outcap(tiny) == 65
    three = with_rev(raw([mutate(rng, T) for _ in range(3)]), alternating(3))
    return tiny, three, cx.prepare(reads)


@pytest.fixture(scope="module")
def zs():
    tiny, three, prepared = _small()
    zs = [synth(9100, 1500, 6), synth(9101, 1500, 6), edge()["ragged_lengths"], tiny, three, prepared]
    assert sum(_outcap(z) for z in zs) % 8
    return [with_kin(z, seed=j) for j, z in enumerate(zs)]


@pytest.fixture(scope="module")
def zs_objects():
    """The batch of test_subsets_on_every_kernel_object: 70 reads make two mask
    words, so the kinetics' sums cross words with the map's walk on or off beside
    them, and the pileup carries its dropped bases from chunk to chunk of columns
    with the kinetics on or off."""
    tiny, three, _ = _small()
    over = with_rev(edge_cases()["over_64_reads"], alternating(70))
    assert len(over.lens) == 70
    return [with_kin(z, seed=20 + j) for j, z in enumerate([synth(9110, 1500, 6), synth(9111, 1500, 6), tiny, three, over])]


@pytest.fixture(scope="module")
def zs_hbm():
    """4,200 segments of 60 bases, more than the 4,096 LDS shredding cursors:
    the slice runs the HBM-read kernel instance (66 mask words per column)."""
    rnd = random.Random(13)
    ins = bytes(rnd.choice(b"ACGT") for _ in range(60))
    segs = []
    for _ in range(4200):
        s = bytearray(ins)
        s[rnd.randrange(60)] = rnd.choice(b"ACGT")
        segs.append(bytes(s))
    return [with_kin(raw(segs), alternating(4200), seed=4)]


_REFS = {}


def _refs(zs, mode):
    """The oracle's CCS and the five references of the batch, once per batch and mode."""
    if (id(zs), mode) not in _REFS:
        r = {"ccs": batch(zs, mode, 8)[0],
             "quality": [qr.reference(z, mode)[1] for z in zs],
             "pass_stats": [pr.reference(z, mode)[1] for z in zs],
             "base_map": [br.reference(z, mode)[1] for z in zs],
             "pileup": [pu.reference(z, mode)[1] for z in zs],
             "kinetics": [kr.reference(z, mode)[1] for z in zs]}
        _REFS[id(zs), mode] = r, zs  # (zs held: its id stays its own)
    return _REFS[id(zs), mode][0]


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
        engine.set_kernel_cfg(-1)
        engine.set_tight_out(0)
        engine.set_tight_rows(0)
        engine.set_slot_budget(0)
        engine.set_fault(-1)


def _same(name, got, want):
    if name == "quality":
        return got == want
    if name == "base_map":
        return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
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
    if len(subset) in (0, 5):
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
    assert left == sengine.zmw_bytes(zs[0]) + sum(_terms(zs[0])[n] for n in others)
    # 3. stage() / launch() / fetch()
    _apply(sengine, subset)
    sengine.stage(zs, cx.MODE_SHRED)
    sengine.launch(cx.MODE_SHRED)
    _check(sengine, ref, subset, sengine.fetch())


@pytest.mark.parametrize("path", ["run", "submit"])
def test_failed_zmw_in_every_output(sengine, zs, path):
    """set_fault(1) with all five on: ZMW 1 reads as an empty quality and is
    refused by the other four; every other ZMW is exact."""
    ref = _refs(zs, cx.MODE_SHRED)
    _apply(sengine, NAMES)
    sengine.set_fault(1)
    if path == "run":
        # (run() raises on a failed ZMW; the call's other results stay with the context)
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
        add = [sum(_terms(z)[n] for n in subset) for z in zs]
        per, staged = sizes[subset]
        assert per == [(a + x, b + x) for (a, b), x in zip(per0, add)], _ids(subset)
        assert staged == staged0 + sum(add), _ids(subset)


R, A, S, K = "pass_stats", "base_map", "pileup", "kinetics"
# each of the side-output kernel's four branches taken and not taken beside each neighbour
KERNEL_SUBSETS = [(R,), (A,), (S,), (K,), (R, S), (A, K), NAMES]


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("subset", KERNEL_SUBSETS, ids=_ids)
def test_subsets_on_every_kernel_object(sengine, zs_objects, subset, cfg):
    _apply(sengine, subset)
    sengine.set_kernel_cfg(cfg)
    _check(sengine, _refs(zs_objects, cx.MODE_SHRED), subset, sengine.run(zs_objects, cx.MODE_SHRED))
    # (a forced 4 / 5 that the int16 ring cannot take runs 3)
    assert sengine.kernel_cfg() in ((3, cfg) if cfg >= 4 else (cfg,))


@pytest.mark.parametrize("subset", [(R,), (S,), (A, K), NAMES], ids=_ids)
def test_subsets_hbm_read_instance(sengine, zs_hbm, subset):
    _apply(sengine, subset)
    before = sengine.hbm_launches()
    _check(sengine, _refs(zs_hbm, cx.MODE_SHRED), subset, sengine.run(zs_hbm, cx.MODE_SHRED))
    assert sengine.hbm_launches() - before >= 1
