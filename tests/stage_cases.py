"""A family of ZMWs for the host program's post-collect stages (-p, -B / -d /
-D, -I / -i / -S) in which a swap shows: 96 ZMWs, each with an insert length, a
barcode pair and an adapter layout of its own, so that a record attached to
the wrong ZMW, or read from the wrong batch, slot or compacted index, differs
from the right one in every file.  96 is the smallest count that gives
tests/cli_batches.py's SPREAD chunks of 16, 64 and a rest of 16, cut into 4, 12
and 4 batches.

The pieces are built as barcode_cases.accuracy_case and
scan_cases.accuracy_case build theirs: 12 barcodes of 16 bases at edit distance
>= 7 from each other and from all reverse complements, 3 adapters of 25 bases
at edit distance >= 9, 8 subreads per ZMW at 2 / 4 / 4 % errors, the odd ones
reverse-complemented.  Hole h is bc[i0] + insert + rc(bc[i1]) with an insert
of 600 + 7 h bases and (i0, i1) = (h % 12, (5 h + 1) % 12) -- every 8th hole
has random ends instead -- and, written over the insert at places that depend
on h, no adapter (h % 3 == 0), one (h % 3 == 1) or two in opposite
orientations (h % 3 == 2).  Two more ZMWs lie among them in the input, one
with too few subreads and one below -m 1000: the program drops both as it
reads, so neither counts towards a chunk.

tests/test_stage_cases.py holds the family to its purpose on the reference
alone (no GPU); tests/test_gpu_cli_stages.py runs the host program on it.
"""
from __future__ import annotations

import functools
import random

from . import barcode_ref as BR
from .polish_ref import mutate

rc = BR.revcomp
N = 96
MIN_TOTAL = 1000            # the runs' -m
FAULT_HOLE = 50             # the hole CCSX_FAULT_HOLE names: inside the 64-ZMW chunk, inside its batch
FEW_HOLE, SHORT_HOLE = 900, 901
BC_NAMES = [f"bc{1001 + i}" for i in range(12)]
AD_NAMES = [f"ad{k}" for k in range(3)]


def pair_of(h: int):
    """The barcode pair hole h was built with; None for the holes with random ends."""
    return None if h % 8 == 7 else (h % 12, (5 * h + 1) % 12)


def adapters_of(h: int) -> list:
    """[(adapter, orient, offset in the insert)] of hole h, by offset."""
    a = (h // 3) % 3
    p = 120 + (11 * h) % 90
    if h % 3 == 0:
        return []
    if h % 3 == 1:
        return [(a, (h // 9) % 2, p)]
    o = (h // 9) % 2
    return [(a, o, p), ((a + 1) % 3, 1 - o, p + 25 + 180 + (7 * h) % 60)]


def _distinct(rng, count: int, n: int, dmin: int) -> list:
    out: list = []
    while len(out) < count:
        c = bytes(rng.choice(b"ACGT") for _ in range(n))
        if BR.edit_distance(c, rc(c)) >= dmin and all(
                BR.edit_distance(c, b) >= dmin and BR.edit_distance(c, rc(b)) >= dmin for b in out):
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def family(seed: int = 11):
    """(barcodes, adapters, [(hole, [subreads])] in input order)."""
    rng = random.Random(seed)
    bcs = _distinct(rng, 12, 16, 7)
    ads = _distinct(rng, 3, 25, 9)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))  # noqa: E731
    zmws = []
    for h in range(N):
        ins = rnd(600 + 7 * h)
        for a, o, p in adapters_of(h):
            w = rc(ads[a]) if o else ads[a]
            ins = ins[:p] + w + ins[p + 25:]
        assert len(ins) == 600 + 7 * h
        pr = pair_of(h)
        t = (bcs[pr[0]] if pr else rnd(16)) + ins + (rc(bcs[pr[1]]) if pr else rnd(16))
        subs = [mutate(rng, t, .02, .04, .04) for _ in range(8)]
        zmws.append((h, [s if k % 2 == 0 else rc(s) for k, s in enumerate(subs)]))
        if h == 37:    # too few subreads (-c 3 asks for five)
            zmws.append((FEW_HOLE, [rnd(700) for _ in range(3)]))
        if h == 70:    # below -m
            t = rnd(100)
            zmws.append((SHORT_HOLE, [t if k % 2 == 0 else rc(t) for k in range(8)]))
    return bcs, ads, zmws


def kept() -> list:
    """[(hole, subreads)] the program keeps (its -c and -m filters), in input order."""
    return [(h, subs) for h, subs in family()[2] if len(subs) >= 5 and sum(map(len, subs)) >= MIN_TOTAL]


def write_inputs(d) -> tuple:
    """The subread FASTA, the barcode FASTA and the adapter FASTA under directory d."""
    bcs, ads, zmws = family()
    fa, bfa, afa = (str(d / n) for n in ("in.fa", "bc.fa", "ad.fa"))
    with open(fa, "wb") as f:
        for h, subs in zmws:
            qs = 0
            for s in subs:
                f.write(b">synth/%d/%d_%d\n%s\n" % (h, qs, qs + len(s), s))
                qs += len(s)
    with open(bfa, "w") as f:
        for nm, b in zip(BC_NAMES, bcs):
            f.write(f">{nm} sample\n{b.decode()}\n")
    with open(afa, "w") as f:
        for nm, a in zip(AD_NAMES, ads):
            f.write(f">{nm} adapter\n{a.decode()}\n")
    return fa, bfa, afa


@functools.lru_cache(maxsize=None)
def oracle_ccs() -> tuple:
    """([prepared ZMW], [CCS]) of the kept ZMWs by the oracle alone, computed once."""
    from oracle.oracle import batch
    from oracle.oracle import prepare as oracle_prepare
    ps = [oracle_prepare(subs) for _, subs in kept()]
    ccs, _, _ = batch(ps, 0, 16)
    return ps, ccs


def fault_batch(cx, nparts: int = 12, min_batch: int = 4) -> tuple:
    """(the holes of FAULT_HOLE's batch in the order the device gets them, its
    position among them) under SPREAD: the second chunk is the kept ZMWs 16 ..
    79, cut by ccsx_partition on ccsx_zmw_cost of the prepared segments."""
    ks = kept()[16:80]
    costs = [cx.zmw_cost(cx.prepare(subs).lens) for _, subs in ks]
    _, batches = cx.partition(costs, nparts, min_batch)
    at = [h for h, _ in ks].index(FAULT_HOLE)
    b = next(b for b in batches if at in b)
    return [ks[i][0] for i in b], b.index(at)
