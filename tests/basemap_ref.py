"""Reference for the subread-to-CCS coordinate map (SPEC.md §11): a numpy
restatement of ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's
Poa.poa(reads), one call per pushed window, as tests/pass_ref.py is.
Everything is computed from the returned MSA matrix alone.  Per emitted column
c < i of a call with ol CCS bases emitted before it, and per read k with a base
in c (has(c,k)), that base's entry is

    t(c) = ol + |{c' < c : cons[c'] < 4}|          bits 0..29
    MISMATCH (bit 30)   cons[c] < 4 and not eq(c,k)
    INS      (bit 31)   cons[c] = 4

A read's bases lie in increasing columns, and the rounds take them in order, so
appending per round and per column gives the read's map in base order.

It proves itself before it judges anything: reference() asserts its CCS against
pass_ref.reference (which checks the oracle's CCS and breakpoint log) and that
every segment got exactly seg_len entries.  cigar() states the derived
alignment of SPEC.md §11 in Python, independently of ccsx_map_cigar.
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import Poa

from . import pass_ref as pr
from .quality_ref import ADDLEN, INITLEN, MINLEN, _breakpoint, column_quals

OFFSET, MISMATCH, INS = (1 << 30) - 1, 1 << 30, 1 << 31

_cache: dict = {}


def round_map(cons, eq, has, i: int, ol: int, maps: list) -> int:
    """Append the entries of columns [0, i) of one POA call to maps[k]; ol =
    CCS bases emitted before this call.  Returns the CCS bases this call emits."""
    base = cons[:i] < 4
    t = ol + np.cumsum(base) - base  # consensus-base columns before c
    for k in range(has.shape[1]):
        cols = np.nonzero(has[:i, k])[0]
        w = t[cols].astype(np.int64)
        w |= np.where(~base[cols], INS, np.where(~eq[cols, k], MISMATCH, 0))
        maps[k].append(w)
    return int(base.sum())


def _run(z, mode: int):
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    ccs = bytearray()
    maps = [[] for _ in range(n)]

    def take(cons, eq, has, i):
        round_map(cons, eq, has, i, len(ccs), maps)
        ccs.extend(b"ACGT"[c] for c in cons[:i][cons[:i] < 4])

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, _, eq, has = column_quals(msa, n)
        take(cons, eq, has, len(cons))
    else:
        colrate = 60 if n < 10 else 80
        pos = [0] * n
        flag = True
        while flag:
            ws = INITLEN
            while True:
                fin = n < 3 or any(pos[k] + ws + MINLEN >= lens[k] for k in range(n))
                if fin:
                    flag = False
                    reads = [z.seqs[offs[k] + pos[k]:offs[k] + lens[k]] for k in range(n)]
                else:
                    reads = [z.seqs[offs[k] + pos[k]:offs[k] + pos[k] + ws] for k in range(n)]
                _, msa = poa.poa(reads)
                cons, _, _, _, eq, has = column_quals(msa, n)
                if not flag:
                    i = len(cons)
                    break
                i = _breakpoint(cons, eq, n, colrate)
                if i >= 1:
                    break
                ws += ADDLEN
            if flag:
                adv = has[:i].sum(0)
                pos = [pos[k] + int(adv[k]) for k in range(n)]
            take(cons, eq, has, i)
    out = []
    for k in range(n):
        m = (np.concatenate(maps[k]) if maps[k] else np.zeros(0, np.int64)).astype(np.uint32)
        m.setflags(write=False)
        out.append(m)
    return bytes(ccs), out


def reference(z, mode: int):
    """(ccs, [uint32 map per segment]) of a prepared ZMW; computed once per
    (ZMW, mode) and checked against pass_ref's CCS (hence the oracle's)."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), mode)
    if key not in _cache:
        ccs, maps = _run(z, mode)
        assert ccs == pr.reference(z, mode)[0], "basemap_ref: CCS differs from pass_ref's"
        assert [len(m) for m in maps] == [int(x) for x in z.lens], "basemap_ref: a base without exactly one entry"
        _cache[key] = (ccs, maps)
    return _cache[key]


def cigar(m):
    """The alignment derived from one segment's map (SPEC.md §11): a dict with
    qs, qe, ts, te, n_eq, n_x, n_ins, n_del, cigar; None without an aligned entry."""
    m = [int(x) for x in m]
    al = [j for j, w in enumerate(m) if not w & INS]
    if not al:
        return None
    qs, qe = al[0], al[-1] + 1
    ops = []  # [op, run]

    def add(op, k):
        if ops and ops[-1][0] == op:
            ops[-1][1] += k
        else:
            ops.append([op, k])

    prev = None
    for j in range(qs, qe):
        w = m[j]
        if w & INS:
            add("I", 1)
            continue
        t = w & OFFSET
        if prev is not None and t - prev - 1 > 0:
            add("D", t - prev - 1)
        add("X" if w & MISMATCH else "=", 1)
        prev = t
    cnt = {o: sum(r for p, r in ops if p == o) for o in "=XID"}
    return dict(qs=qs, qe=qe, ts=m[qs] & OFFSET, te=(m[qe - 1] & OFFSET) + 1, n_eq=cnt["="], n_x=cnt["X"],
                n_ins=cnt["I"], n_del=cnt["D"], cigar="".join(f"{r}{o}" for o, r in ops))


def check_invariants(z, mode: int):
    """The invariants of SPEC.md §11 on the reference's maps of z."""
    ccs, maps = reference(z, mode)
    rec = pr.reference(z, mode)[1].astype(np.int64)
    for k, m in enumerate(maps):
        w = m.astype(np.int64)
        off, ins, mis = w & OFFSET, (w & INS) != 0, (w & MISMATCH) != 0
        assert len(w) == int(z.lens[k])
        assert not (ins & mis).any()
        assert (np.diff(off) >= 0).all()
        assert (np.diff(off[~ins]) > 0).all()
        assert (off <= len(ccs)).all() and (off[~ins] < len(ccs)).all()
        assert [int((~ins & ~mis).sum()), int(mis.sum()), int(ins.sum())] == rec[k, :3].tolist()
        # "mismatch flag clear" <=> the base's 2-bit code equals the CCS base's
        seg = z.seqs[int(z.offs[k]):int(z.offs[k]) + int(z.lens[k])]
        code = lambda b: {99: 1, 103: 2, 116: 3, 117: 3}.get(b | 0x20, 0)  # noqa: E731  (SPEC.md §1)
        for j in np.nonzero(~ins)[0]:
            assert (code(seg[j]) == code(ccs[off[j]])) == (not mis[j])
    return maps
