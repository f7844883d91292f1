"""Reference for the per-base strand pileup (SPEC.md §12): a numpy restatement
of ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's Poa.poa(reads), one
call per pushed window, as tests/pass_ref.py is.  Everything is computed from
the returned MSA matrix and the strand flags alone.  Per emitted column c < i of
a call and per strand s (the reads k with rev(k) = s):

    cnt_s[b]  reads with base b in c          cov_s  reads spanning c
    gap_s     cov_s - sum_b cnt_s[b]          tot_s  sum_b cnt_s[b]

A column with cons < 4 gives the next CCS base its record: per strand cnt_s[0..3],
gap_s and ins_s = the tot_s of the gap-consensus columns emitted since the
previous CCS base's column, over all rounds; every field min(., 255).

It proves itself before it judges anything: reference() asserts that its CCS
equals Poa.zmw() and, in shredded mode, that its breakpoint log equals
Poa.zmw_breakpoints().
"""
from __future__ import annotations

import numpy as np

from oracle.oracle import Poa

from .quality_ref import ADDLEN, INITLEN, MINLEN, _breakpoint, column_quals

A, C, G, T, GAP, INS = range(6)
FWD, REV = 0, 6

_cache: dict = {}


def flags(z) -> np.ndarray:
    """rev(k) per pushed segment: z.rev, or all forward where it has none."""
    n = len(z.lens)
    r = getattr(z, "rev", None)
    return np.zeros(n, np.uint8) if r is None else np.asarray(r, np.uint8).reshape(n)


def call(rec, strand: int) -> int:
    """SPEC.md §12's strand call from one 12-byte record: strand 0 fwd, 1 rev,
    2 both (the sum of the stored bytes); -1 without evidence, 0..3, or 4 (gap)."""
    r = np.asarray(rec, np.int64).reshape(12)
    c = r[FWD:FWD + 5] if strand == 0 else r[REV:REV + 5] if strand == 1 else r[FWD:FWD + 5] + r[REV:REV + 5]
    if c.sum() == 0:
        return -1
    best = int(np.argmax(c[:4]))  # (the first maximum: ties go to the smallest base)
    return best if c[best] >= c[GAP] else 4


def sites(recs) -> list:
    """The discordant positions of a ZMW's records: (p, fwd call, rev call)."""
    out = []
    for p, r in enumerate(recs):
        f, v = call(r, 0), call(r, 1)
        if f >= 0 and v >= 0 and f != v:
            out.append((p, f, v))
    return out


def site_lines(name: str, ccs: bytes, recs) -> str:
    """The -s report of one ZMW (the CLI's columns)."""
    return "".join("%s\t%d\t%c\t%c\t%c\t%s\n" % (name, p, ccs[p], "ACGT-"[f], "ACGT-"[v], "\t".join(str(int(x)) for x in recs[p]))
                   for p, f, v in sites(recs))


def round_pileup(msa, cons, has, i: int, rev, carry: np.ndarray, recs: list) -> None:
    """Append the records of the consensus-base columns among [0, i) of one POA
    call to recs (int64 [12], unsaturated); carry [2] = the bases of the
    gap-consensus columns emitted since the last CCS base, updated in place."""
    ncols, n = has.shape
    reads = msa[:, 1:n + 1]
    some = has.any(0)
    first = np.where(some, has.argmax(0), ncols)
    last = np.where(some, ncols - 1 - has[::-1].argmax(0), -1)
    col = np.arange(ncols)[:, None]
    span = (col >= first[None, :]) & (col <= last[None, :])
    out = np.zeros((i, 12), np.int64)
    for s, o in ((0, FWD), (1, REV)):
        m = (rev == s)[None, :]
        for b in range(4):
            out[:, o + b] = ((reads[:i] == b) & m).sum(1)
        out[:, o + GAP] = (span[:i] & m).sum(1) - out[:, o:o + 4].sum(1)
    for c in range(i):
        for s, o in ((0, FWD), (1, REV)):
            if cons[c] < 4:
                out[c, o + INS] = carry[s]
                carry[s] = 0
            else:
                carry[s] += out[c, o:o + 4].sum()
        if cons[c] < 4:
            recs.append(out[c])


def _run(z, mode: int):
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    rev = flags(z)
    ccs, log, recs = bytearray(), [], []
    carry = np.zeros(2, np.int64)
    seen = 0  # the largest carry a round handed to the next one (both strands)

    def take(msa, cons, has, i):
        round_pileup(msa, cons, has, i, rev, carry, recs)
        ccs.extend(b"ACGT"[c] for c in cons[:i][cons[:i] < 4])

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, _, eq, has = column_quals(msa, n)
        take(msa, cons, has, len(cons))
        return bytes(ccs), recs, int(carry.sum()), log, seen
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
        take(msa, cons, has, i)
        if flag:
            seen = max(seen, int(carry.sum()))
    return bytes(ccs), recs, int(carry.sum()), log, seen


def reference(z, mode: int):
    """(ccs, records uint8 [len, 12], tail, breakpoint log, largest cross-round
    carry) of a prepared ZMW with its strand flags; computed once per (ZMW,
    flags, mode) and checked against the oracle's own loop.  tail = the bases of
    the gap-consensus columns emitted after the last CCS base (not reported)."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), flags(z).tobytes(), mode)
    if key not in _cache:
        ccs, recs, tail, log, seen = _run(z, mode)
        o = Poa()
        if mode == 0:
            want, wlog = o.zmw_breakpoints(z.seqs, z.offs, z.lens)
            assert log == [(int(a), int(b)) for a, b in wlog], "pileup_ref: breakpoint log differs from the oracle's"
        else:
            want = o.zmw(z.seqs, z.offs, z.lens, mode)
        assert ccs == want, "pileup_ref: CCS differs from the oracle's"
        assert len(recs) == len(ccs)
        r = (np.minimum(np.array(recs, np.int64), 255) if recs else np.zeros((0, 12), np.int64)).astype(np.uint8).reshape(-1, 12)
        r.setflags(write=False)
        _cache[key] = (ccs, r, tail, log, seen)
    return _cache[key]
