"""Constructed inputs of the polish step (SPEC.md §15): hand-written drafts,
segments and §11 maps, none from a POA, at the smallest shapes where the
kernels can go wrong.  cases() -> [(name, ccs, segs, maps, expect)]; expect
holds what the case was built to reach, as fields of the reference's result
(tests/test_polish_host.py asserts them on polish_ref, so a case that no longer
reaches its situation fails there).  Shared by the host and the GPU tests;
reference() computes polish_ref once per case.
"""
from __future__ import annotations

import random

import numpy as np

from . import polish_ref as R

INS = R.INS


def draft(seed: int, n: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def noisy(rng, d: bytes, lo: int = 0, hi: int | None = None, ps=.02, pi=.04, pd=.04):
    """A subread of d[lo:hi] with errors, and the anchors a POA would give it:
    the draft offset of a kept base, the next offset for an inserted one."""
    hi = len(d) if hi is None else hi
    out, an = bytearray(), []
    for p in range(lo, hi):
        r = rng.random()
        if r < pd:
            continue
        out.append(rng.choice([c for c in b"ACGT" if c != d[p]]) if r < pd + ps else d[p])
        an.append(p)
        while rng.random() < pi:
            out.append(rng.choice(b"ACGT"))
            an.append(p + 1 | INS)
    return bytes(out), np.array(an, np.uint32)


def ident(lo: int, m: int) -> np.ndarray:
    return np.arange(lo, lo + m, dtype=np.uint32)


def at(d: bytes, anchors) -> tuple:
    """The segment that has the draft's base at every anchor (clamped to the draft)."""
    a = np.array(anchors, np.uint32)
    return bytes(d[min(int(x), len(d) - 1)] for x in a), a


def cases():
    out = []

    def add(name, ccs, sm, **expect):
        out.append((name, ccs, [s for s, _ in sm], [m for _, m in sm], expect))

    # draft lengths: invalid cells, both clamp edges
    for n in (1, 63, 64, 65, 200):
        rng, d = random.Random(100 + n), draft(n, n)
        add(f"n{n}", d, [noisy(rng, d), noisy(rng, d), (d, ident(0, n))])
    for n in (65, 200):
        d = draft(7, n)
        add(f"tail{n}", d, [(d[n - 10:], ident(n - 10, 10)), (d, ident(0, n))])
    # segment lengths: the 64-row blocks' edges
    d = draft(8, 200)
    for m in (1, 63, 64, 65, 129):
        rng = random.Random(m)
        add(f"m{m}", d, [(d[10:10 + m], ident(10, m)), noisy(rng, d, 0, 180)])
    # row shifts 0, 1 and 63 inside a piece
    d = draft(9, 400)
    add("shifts", d, [at(d, [100, 100, 101, 164, 165, 166, 166, 229]), (d, ident(0, 400))])
    # piece breaks: a shift of 64 (two pieces), of 64 and 300 (three), pieces of one row
    d = draft(10, 700)
    add("break64", d, [at(d, [100, 101, 102, 166, 167, 168])])
    add("break300", d, [at(d, [100, 101, 102, 166, 167, 467, 468, 469]), noisy(random.Random(3), d)])
    add("onerow", d, [at(d, [100, 200, 300, 301, 600]), (d[:650], ident(0, 650))])
    # a segment whose input map has insertion entries only; an empty segment among others
    d = draft(11, 120)
    add("allins", d, [(d[45:55], np.full(10, INS | 50, np.uint32)), (d, ident(0, 120))])
    add("empty", d, [(d, ident(0, 120)), (b"", np.zeros(0, np.uint32)), (d[5:50], ident(5, 45)),
                     (b"", np.zeros(0, np.uint32))])
    # homopolymers: direction ties in the order diag, up, left
    h = b"A" * 40
    add("homo", h, [(b"A" * 39, ident(0, 39)), (b"A" * 41, np.minimum(ident(0, 41), 40)), (b"A" * 40, ident(0, 40))])
    # vote ties, on exact copies of a draft without repeats around position 50
    d = bytearray(draft(12, 100))
    d[48:53] = b"ACGTA"
    d = bytes(d)
    full = (d, ident(0, 100))
    sub = lambda ch: (d[:50] + bytes([ch]) + d[51:], ident(0, 100))  # noqa: E731
    dele = (d[:50] + d[51:], np.concatenate([ident(0, 50), ident(51, 49)]))
    insr = lambda s: (d[:51] + s + d[51:], np.concatenate([ident(0, 51), np.full(len(s), INS | 51, np.uint32),  # noqa: E731
                                                            ident(51, 49)]))
    # d[50] = G: two reads say C, two say T -> C, the smallest; a substitution
    add("tie2v2", d, [sub(ord("T")), sub(ord("C")), sub(ord("T")), sub(ord("C"))], counts=(1, 0, 0), seq=d[:50] + b"C" + d[51:])
    add("gap_keep", d, [full, dele, full, dele], counts=(0, 0, 0), seq=d)
    add("gap_drop", d, [full, dele, full, dele, dele], counts=(0, 0, 1), seq=d[:50] + d[51:])
    add("ins_half", d, [full, insr(b"C"), full, insr(b"C")], counts=(0, 0, 0), seq=d)
    add("ins_more", d, [full, insr(b"C"), insr(b"C"), insr(b"C"), full], counts=(0, 1, 0), seq=d[:51] + b"C" + d[51:])
    # (counted twice, the one read's two insertions would outvote the two others)
    add("ins_once", d, [insr(b"CC"), full, full], counts=(0, 0, 0), seq=d)
    # segment counts
    d = draft(13, 100)
    rng = random.Random(13)
    for k in (1, 2, 70):
        sm = []
        for _ in range(k):
            lo = rng.randrange(0, 70)
            sm.append(noisy(rng, d, lo, lo + 30))
        add(f"nseg{k}", d, sm)
    # positions no piece covers keep the draft base with kQMin
    d = draft(14, 200)
    add("uncovered", d, [(d[:50], ident(0, 50)), (d[10:40], ident(10, 30))], tail=(d[50:], bytes([R.Q_MIN]) * 150))
    # an empty draft
    add("n0", b"", [(b"ACG", np.full(3, INS, np.uint32))], counts=(0, 0, 0), seq=b"")
    # bad maps: a decreasing anchor, an anchor past the draft
    d = draft(15, 80)
    bad = ident(0, 80).copy()
    bad[40] = 38
    add("bad_decreasing", d, [(d, ident(0, 80)), (d, bad)], status=R.BAD_MAP)
    add("bad_beyond", d, [(d + b"A", ident(1, 81))], status=R.BAD_MAP)
    add("after_bad", d, [(d, ident(0, 80)), noisy(random.Random(4), d)])
    return out


_ref: dict = {}


def reference(i: int):
    """polish_ref's result of case i, computed once and left unchanged."""
    if i not in _ref:
        _, ccs, segs, maps, _ = CASES[i]
        _ref[i] = R.polish(ccs, segs, maps)
    return _ref[i]


def same(got, want) -> bool:
    return (got[0], got[1], tuple(got[2]), got[4]) == (want[0], want[1], tuple(want[2]), want[4]) and \
        len(got[3]) == len(want[3]) and all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))


CASES = cases()
NAMES = [c[0] for c in CASES]
