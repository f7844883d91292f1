"""Reference for the per-base consensus qualities (SPEC.md §9): a numpy
restatement of ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's
Poa.poa(reads), one call per pushed window.  Everything is computed from the
returned MSA matrix alone: per column `match` = reads carrying the consensus
base, `cov` = reads whose first..last column with a base contains the column,
Q = clamp(3 * (2 * match - cov), 2, 93).

It proves itself before it judges anything: reference() asserts that its CCS
equals Poa.zmw() and, in shredded mode, that its breakpoint log equals
Poa.zmw_breakpoints().
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import Poa

Q_STEP, Q_MIN, Q_MAX = 3, 2, 93
WINDOW, ADDLEN, MINLEN, INITLEN, MINWIN, ROWRATE = 10, 2000, 1000, 2000, 5, 80

_cache: dict = {}


def phred(match, cov):
    """The SPEC §9 formula (scalars or arrays)."""
    return np.clip(Q_STEP * (2 * np.asarray(match, np.int64) - np.asarray(cov, np.int64)), Q_MIN, Q_MAX).astype(np.uint8)


def rq(qual) -> float:
    """1 - mean(10^(-Q/10)) over raw quality bytes; 0.0 for none."""
    q = np.frombuffer(bytes(qual), np.uint8).astype(np.float64)
    return float(1.0 - np.mean(10.0 ** (-q / 10.0))) if len(q) else 0.0


def column_quals(msa: np.ndarray, n: int):
    """(cons codes, match, cov, Q) per column of an MSA [ncols, n + 4]."""
    ncols = msa.shape[0]
    cons = msa[:, n + 1]
    reads = msa[:, 1:n + 1]
    has = reads < 4
    eq = (reads == cons[:, None]) & (cons[:, None] < 4)
    match = eq.sum(1)
    some = has.any(0)
    first = np.where(some, has.argmax(0), ncols)
    last = np.where(some, ncols - 1 - has[::-1].argmax(0), -1)
    col = np.arange(ncols)[:, None]
    cov = ((col >= first[None, :]) & (col <= last[None, :])).sum(1)
    return cons, match, cov, phred(match, cov), eq, has


def _breakpoint(cons, eq, n, colrate) -> int:
    """main.c:580-612: the largest i >= 1 whose 10-column window is clean; an
    MSA of <= 10 columns has none (SPEC.md §7)."""
    ncols = len(cons)
    if ncols <= WINDOW:
        return 0
    base = cons < 4
    colok = eq.sum(1) * 100 >= colrate * n
    for i in range(ncols - WINDOW, 0, -1):
        nogwin, ok = 0, True
        rowcnt = np.zeros(n, np.int64)
        for j in range(i, i + WINDOW):
            if not base[j]:
                if nogwin:
                    continue
                ok = False
                break
            nogwin += 1
            rowcnt += eq[j]
            if not colok[j]:
                ok = False
                break
        if not ok or nogwin < MINWIN:
            continue
        if (rowcnt * 100 >= ROWRATE * nogwin).all():
            return i
    return 0


def _run(z, mode: int):
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    ccs, qual, log = bytearray(), bytearray(), []

    def take(cons, q, i):
        keep = cons[:i] < 4
        ccs.extend(b"ACGT"[c] for c in cons[:i][keep])
        qual.extend(q[:i][keep].tobytes())

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, q, _, _ = column_quals(msa, n)
        take(cons, q, len(cons))
        return bytes(ccs), bytes(qual), log
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
            cons, _, _, q, eq, has = column_quals(msa, n)
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
        take(cons, q, i)
    return bytes(ccs), bytes(qual), log


def reference(z, mode: int):
    """(ccs, raw quality bytes, breakpoint log) of a prepared ZMW; computed
    once per (ZMW, mode) and checked against the oracle's own loop."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), mode)
    if key not in _cache:
        ccs, qual, log = _run(z, mode)
        assert len(ccs) == len(qual)
        o = Poa()
        if mode == 0:
            want, wlog = o.zmw_breakpoints(z.seqs, z.offs, z.lens)
            assert log == [(int(a), int(b)) for a, b in wlog], "quality_ref: breakpoint log differs from the oracle's"
        else:
            want = o.zmw(z.seqs, z.offs, z.lens, mode)
        assert ccs == want, "quality_ref: CCS differs from the oracle's"
        _cache[key] = (ccs, qual, log)
    return _cache[key]
