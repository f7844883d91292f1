"""Reference for the per-base consensus kinetics (SPEC.md §13): a numpy
restatement of ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's
Poa.poa(reads), one call per pushed window, as tests/basemap_ref.py is.
Everything is computed from the returned MSA matrix, the strand flags and the
two code planes alone.  Per emitted column c < i with cons[c] < 4 and per strand
s (the reads k with rev(k) = s):

    K  = the reads of s with eq(c,k)             n = |K|
    mi = (sum_K frames(ipd) + n // 2) // n       mp likewise from pw

over the base each read of K has in the column: base pos[k] + (the read's bases
in the columns up to c) - 1 of the segment as pushed, pos[k] the bases the
earlier rounds consumed.  The record is code(mi), code(mp), min(n, 255) per
strand (0, 0, 0 for n = 0) and two zero bytes.

It proves itself before it judges anything: reference() asserts its CCS against
quality_ref.reference (which checks the oracle's CCS and breakpoint log).
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import Poa

from . import quality_ref as qr
from .quality_ref import ADDLEN, INITLEN, MINLEN, _breakpoint, column_quals

MAXF = 952
_cache: dict = {}
_msa: dict = {}


def frames(b):
    """frames(b) of SPEC.md §13 (scalars or arrays)."""
    b = np.asarray(b, np.int64)
    g = b >> 6
    return ((b & 63) << g) + (64 << g) - 64


FRAMES = frames(np.arange(256))


def code(f: int) -> int:
    """code(f): the byte whose frames are nearest to min(f, 952), the lower on a
    tie (np.argmin takes the first minimum; FRAMES is increasing)."""
    return int(np.argmin(np.abs(FRAMES - min(int(f), MAXF))))


CODE = np.array([code(f) for f in range(MAXF + 1)], np.int64)


def flags(z) -> np.ndarray:
    n = len(z.lens)
    r = getattr(z, "rev", None)
    return np.zeros(n, np.uint8) if r is None else np.asarray(r, np.uint8).reshape(n)


def round_kin(cons, eq, has, i: int, rev, pos, offs, ipd, pw, recs: list, match: list) -> None:
    """Append the records of the consensus-base columns among [0, i) of one POA
    call to recs ([8] ints, n unsaturated) and their §9 match to `match`."""
    base = np.nonzero(cons[:i] < 4)[0]
    out = np.zeros((len(base), 8), np.int64)
    if len(base) and ipd is not None:
        n = has.shape[1]
        idx = (np.cumsum(has, 0) - 1)[base]  # the read's base in the column, within the pushed window
        at = np.asarray(offs, np.int64)[None, :] + np.asarray(pos, np.int64)[None, :] + idx
        e = eq[base]
        at = np.where(e, at, 0)
        fi = FRAMES[np.frombuffer(ipd, np.uint8)[at.reshape(-1)]].reshape(-1, n)
        fp = FRAMES[np.frombuffer(pw, np.uint8)[at.reshape(-1)]].reshape(-1, n)
        for s, o in ((0, 0), (1, 3)):
            m = e & (rev == s)[None, :]
            cnt = m.sum(1)
            d = np.maximum(cnt, 1)
            mi, mp = ((fi * m).sum(1) + cnt // 2) // d, ((fp * m).sum(1) + cnt // 2) // d
            out[:, o] = np.where(cnt > 0, CODE[mi], 0)
            out[:, o + 1] = np.where(cnt > 0, CODE[mp], 0)
            out[:, o + 2] = cnt
    recs.extend(out.tolist())
    match.extend(int(x) for x in eq[base].sum(1))


def _rounds(z, mode: int):
    """(ccs, [(cons, eq, has, i, pos)]) of the POA calls that emit: the MSA of
    each with the columns [0, i) it emits and the cursors it found.  Computed
    once per (ZMW, mode): the strand flags and the planes do not move the MSA."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), mode)
    if key in _msa:
        return _msa[key]
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    ccs, rounds = bytearray(), []
    pos = [0] * n

    def take(cons, eq, has, i):
        rounds.append((cons, eq, has, i, list(pos)))
        ccs.extend(b"ACGT"[c] for c in cons[:i][cons[:i] < 4])

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, _, eq, has = column_quals(msa, n)
        take(cons, eq, has, len(cons))
    else:
        colrate = 60 if n < 10 else 80
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
            take(cons, eq, has, i)
            if flag:
                adv = has[:i].sum(0)
                for k in range(n):
                    pos[k] += int(adv[k])
    assert bytes(ccs) == qr.reference(z, mode)[0], "kinetics_ref: CCS differs from quality_ref's"
    _msa[key] = (bytes(ccs), rounds)
    return _msa[key]


def _run(z, mode: int):
    ccs, rounds = _rounds(z, mode)
    offs = [int(x) for x in z.offs]
    rev = flags(z)
    ipd, pw = getattr(z, "ipd", None), getattr(z, "pw", None)
    if ipd is None or pw is None:
        ipd = pw = None
    recs, match = [], []
    for cons, eq, has, i, pos in rounds:
        round_kin(cons, eq, has, i, rev, pos, offs, ipd, pw, recs, match)
    return ccs, recs, match


def reference(z, mode: int):
    """(ccs, records uint8 [len, 8], unsaturated per-strand n int64 [len, 2],
    §9 match per CCS base) of a prepared ZMW with its strand flags and planes;
    computed once per (ZMW, flags, planes, mode), its CCS checked against
    quality_ref's (hence the oracle's)."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), flags(z).tobytes(),
           getattr(z, "ipd", None), getattr(z, "pw", None), mode)
    if key not in _cache:
        ccs, recs, match = _run(z, mode)
        assert len(recs) == len(ccs)
        full = np.array(recs, np.int64).reshape(-1, 8)
        r = full.copy()
        r[:, 2] = np.minimum(r[:, 2], 255)
        r[:, 5] = np.minimum(r[:, 5], 255)
        r = r.astype(np.uint8)
        r.setflags(write=False)
        _cache[key] = (ccs, r, full[:, [2, 5]].copy(), np.array(match, np.int64))
    return _cache[key]


def tags(recs) -> str:
    """The four SAM array tags of a ZMW's records, in Python."""
    r = np.asarray(recs, np.int64).reshape(-1, 8)
    cols = (("fi", r[:, 0]), ("fp", r[:, 1]), ("ri", r[::-1, 3]), ("rp", r[::-1, 4]))
    return "\t".join(t + ":B:C" + "".join(",%d" % v for v in a) for t, a in cols)


def segs_per_strand(z):
    rev = flags(z)
    return int((rev == 0).sum()), int((rev != 0).sum())


def sam_line(name: str, z, mode: int, qual: bytes | None = None, rq: float | None = None) -> str | None:
    """The -k line of one ZMW (None without a CCS); the array tags only where
    the ZMW has planes."""
    ccs, recs, _, _ = reference(z, mode)
    if not ccs:
        return None
    fn, rn = segs_per_strand(z)
    f = [name, "4", "*", "0", "255", "*", "*", "0", "0", ccs.decode(),
         "*" if qual is None else bytes(q + 33 for q in qual).decode(), "np:i:%d" % len(z.lens)]
    if rq is not None:
        f.append("rq:f:%.6f" % rq)
    f += ["fn:i:%d" % fn, "rn:i:%d" % rn]
    if getattr(z, "ipd", None) is not None and getattr(z, "pw", None) is not None:
        f.append(tags(recs))
    return "\t".join(f) + "\n"
