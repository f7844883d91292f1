"""Reference for the per-pass alignment statistics (SPEC.md §10): a numpy
restatement of ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's
Poa.poa(reads), one call per pushed window, as tests/quality_ref.py is.
Everything is computed from the returned MSA matrix alone.  Per emitted column
c < i of a call and per read k:

    has(c,k)   read k has a base in c
    eq(c,k)    cons[c] < 4 and read k carries the consensus base
    span(c,k)  first column with a base of k <= c <= last one

    match     cons < 4 and eq             ins  cons == 4 and has
    mismatch  cons < 4 and has, not eq    del  cons < 4 and span, not has

cbeg / cend: the CCS offsets (over all rounds) of the first spanned emitted
consensus-base column and one past the last; 0, 0 if there is none.

It proves itself before it judges anything: reference() asserts that its CCS
equals Poa.zmw() and, in shredded mode, that its breakpoint log equals
Poa.zmw_breakpoints().
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import Poa

from .quality_ref import ADDLEN, INITLEN, MINLEN, _breakpoint, column_quals

MATCH, MISMATCH, INS, DEL, CBEG, CEND = range(6)
FIELDS = ("match", "mismatch", "ins", "del", "cbeg", "cend")

_cache: dict = {}


def identity(rec) -> float:
    """match / (match + mismatch + ins + del) in double; 0.0 for an empty record."""
    m, x, i, d = (int(v) for v in rec[:4])
    return m / (m + x + i + d) if m + x + i + d else 0.0


def round_stats(cons, eq, has, i: int, ol: int, st: np.ndarray) -> int:
    """Add the counts of columns [0, i) of one POA call to st [n, 6] (int64),
    extend cbeg / cend; ol = CCS bases emitted before this call.  Returns the
    CCS bases this call emits."""
    ncols, n = has.shape
    base = cons < 4
    some = has.any(0)
    first = np.where(some, has.argmax(0), ncols)
    last = np.where(some, ncols - 1 - has[::-1].argmax(0), -1)
    col = np.arange(ncols)[:, None]
    span = (col >= first[None, :]) & (col <= last[None, :])
    b, g = base[:i, None], ~base[:i, None]
    st[:, MATCH] += (eq[:i] & b).sum(0)
    st[:, MISMATCH] += (has[:i] & ~eq[:i] & b).sum(0)
    st[:, INS] += (has[:i] & g).sum(0)
    st[:, DEL] += (span[:i] & ~has[:i] & b).sum(0)
    off = ol + np.cumsum(base[:i]) - 1  # CCS offset of a consensus-base column
    for k in range(n):
        cols = np.nonzero(span[:i, k] & base[:i])[0]
        if len(cols) == 0:
            continue
        if st[k, CEND] == 0:  # (cend >= 1 once a column was spanned)
            st[k, CBEG] = off[cols[0]]
        st[k, CEND] = off[cols[-1]] + 1
    return int(base[:i].sum())


def _run(z, mode: int):
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    ccs, log = bytearray(), []
    st = np.zeros((n, 6), np.int64)

    def take(cons, eq, has, i):
        round_stats(cons, eq, has, i, len(ccs), st)
        ccs.extend(b"ACGT"[c] for c in cons[:i][cons[:i] < 4])

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, _, eq, has = column_quals(msa, n)
        take(cons, eq, has, len(cons))
        return bytes(ccs), st, log
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
        log.append((i, len(cons)))
        if flag:
            adv = has[:i].sum(0)
            pos = [pos[k] + int(adv[k]) for k in range(n)]
        take(cons, eq, has, i)
    return bytes(ccs), st, log


def reference(z, mode: int):
    """(ccs, records uint32 [nseg, 6], breakpoint log) of a prepared ZMW;
    computed once per (ZMW, mode) and checked against the oracle's own loop."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), mode)
    if key not in _cache:
        ccs, st, log = _run(z, mode)
        o = Poa()
        if mode == 0:
            want, wlog = o.zmw_breakpoints(z.seqs, z.offs, z.lens)
            assert log == [(int(a), int(b)) for a, b in wlog], "pass_ref: breakpoint log differs from the oracle's"
        else:
            want = o.zmw(z.seqs, z.offs, z.lens, mode)
        assert ccs == want, "pass_ref: CCS differs from the oracle's"
        rec = st.astype(np.uint32)
        rec.setflags(write=False)
        _cache[key] = (ccs, rec, log)
    return _cache[key]
