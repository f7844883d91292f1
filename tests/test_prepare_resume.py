"""ccs_prepare's two new seams (include/ccsx_host.h), CPU only: the pairwise
aligner split into its seed and its band (ccsx_pairwise_seed /
ccsx_pairwise_band, SPEC.md §8), and the resumable walk (ccsx_prep_*) that
hands out strand_match's alignments as requests -- what the batched driver
(ccsx_prepare_batch) and the device's band aligner build on.  The references
are the oracle's own aligner and ccs_prepare (oracle/prep_oracle.c); every
comparison is exact."""
import random

import numpy as np
import pytest

import ccsx_amd as cx
from oracle import oracle as orc

from .test_prepare_oracle import KINDS, _mutants

ZERO = {k: 0 for k in ("qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln", "score")}


def family():
    """The 180 abnormal-subread ZMWs the resumable and the batched prepare are
    pinned on: 20 of each kind of tests/test_prepare_oracle.py."""
    rng = random.Random(20261020)
    zs = []
    for k in range(180):
        L = rng.randint(1000, 2500)
        passes = rng.randint(5, 10)
        subs, _ = cx.synth_zmw(20261020, 900_000 + k, L, passes)
        kind = KINDS[k % 9]
        if kind != "plain":
            subs = _mutants(rng, subs, kind)
        zs.append(subs)
    return zs


_REF = {}


def family_reference():
    """(ZMWs, the oracle's push lists), computed once; the vacuity guard: the
    lists drop subreads and trim them often enough to mean something."""
    if not _REF:
        zs = family()
        ref = [orc.prepare_segments(z) for z in zs]
        shorter = sum(1 for z, (o, l, r) in zip(zs, ref) if len(l) < len(z))
        trimmed = 0
        for z, (o, l, r) in zip(zs, ref):
            whole, at = set(), 0
            for s in z:
                whole.add((at, len(s)))
                at += len(s)
            trimmed += any((int(a), int(b)) not in whole for a, b in zip(o, l))
        assert shorter >= 60 and trimmed >= 60, (shorter, trimmed)
        _REF["zs"], _REF["ref"] = zs, ref
    return _REF["zs"], _REF["ref"]


def same_lists(got, ref):
    for i, (g, w) in enumerate(zip(got, ref)):
        assert [list(map(int, x)) for x in g] == [list(map(int, x)) for x in w], i
    assert len(got) == len(ref)


@pytest.mark.parametrize("seed", range(6))
def test_seed_then_band_matches_the_oracle(seed):
    """pairwise_seed + pairwise_band == the oracle's pairwise on the pair kinds
    of test_pairwise_matches_spec (noisy window, reverse complement, overhang,
    unrelated, with N), and pairwise is exactly their composition."""
    rng = np.random.default_rng(seed)
    seeded = 0
    for _ in range(25):
        t = rng.integers(0, 4, int(rng.integers(5, 4000))).astype(np.uint8)
        kind = rng.integers(0, 5)
        if kind == 0:
            a = int(rng.integers(0, max(1, len(t) // 3)))
            b = int(rng.integers(a + 1, len(t) + 1))
            q = t[a:b].copy()
            m = rng.random(len(q))
            q[m < 0.05] = rng.integers(0, 4, int((m < 0.05).sum()))
            q = np.delete(q, np.where(rng.random(len(q)) < 0.04)[0])
            q = np.insert(q, np.where(rng.random(len(q)) < 0.06)[0], rng.integers(0, 4, 1)[0])
        elif kind == 1:
            q = (3 - t[::-1]).copy()
        elif kind == 2:
            q = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 400))), t[: len(t) // 2]]).astype(np.uint8)
        elif kind == 3:
            q = rng.integers(0, 4, int(rng.integers(5, 3000))).astype(np.uint8)
        else:
            q = t.copy()
            q[rng.random(len(q)) < 0.03] = 4
        qb, tb = q.astype(np.uint8).tobytes(), t.tobytes()
        d0 = cx.pairwise_seed(qb, tb)
        got = cx.pairwise_band(qb, tb, d0) if d0 is not None else dict(ZERO)
        seeded += d0 is not None
        assert got == orc.pairwise(qb, tb), (kind, d0)
        assert got == cx.pairwise(qb, tb)
    assert seeded >= 10


def test_seed_refuses_short_and_voteless_pairs():
    assert cx.pairwise_seed(bytes(12), bytes(500)) is None
    assert cx.pairwise_seed(bytes(500), bytes(12)) is None
    assert cx.pairwise_seed(bytes([0, 1] * 50), bytes([2, 3] * 50)) is None
    assert cx.pairwise_seed(bytes(range(4)) * 10, bytes(range(4)) * 10) is not None


def test_resumable_prepare_matches_the_oracle():
    """ccsx_prep_* driven from here, cx.pairwise as the answerer and the second
    pair of every request answered too (the walk must discard it where the
    first is accepted): the push lists equal the oracle's on the family."""
    zs, ref = family_reference()
    got, requests, unused = [], 0, 0
    for z in zs:
        p = cx.Prep(z)
        while True:
            want = p.pending()
            if want is None:
                break
            assert len(want) == 2
            p.answer([cx.pairwise(q, t) for q, t in want])
            requests += 1
        unused += p.unused()
        got.append(p.end())
    same_lists(got, ref)
    assert requests > 180 and 0 < unused < requests


def test_resumable_prepare_edges():
    # no subread, one subread: no request, the oracle's lists
    for subs in ([], [b"ACGT" * 300]):
        p = cx.Prep(subs)
        assert p.pending() is None
        same_lists([p.end()], [orc.prepare_segments(subs)])
    # a walk abandoned while a request is pending gives no list
    zs, _ = family_reference()
    n = 0
    for z in zs:
        p = cx.Prep(z)
        if p.pending() is not None:
            assert [len(x) for x in p.end()] == [0, 0, 0]
            n += 1
    assert n >= 60
