"""Reference for the per-strand consensus (SPEC.md §14): a numpy restatement of
ccs_for / ccs_for2 (SPEC.md §7) driven by the oracle's Poa.poa(reads), one call
per pushed window, as tests/pileup_ref.py is.  Everything is computed from the
returned MSA matrix and the strand flags alone.  Per emitted column c < i of a
call and per strand s (the reads k with rev(k) = s):

    cnt_s[b]  reads with base b in c          cov_s  reads spanning c
    gap_s     cov_s - sum_b cnt_s[b]          best   argmax cnt_s (first maximum)
    call_s    -1 if cov_s = 0, best if cnt_s[best] >= gap_s, else 4

The consensus of strand s is the bases call_s < 4 over all emitted columns in
emission order, each with Q_s = clamp(3 * (2 * cnt_s[best] - cov_s), 2, 93).

It proves itself before it judges anything: reference() asserts that its CCS
equals Poa.zmw() and, in shredded mode, that its breakpoint log equals
Poa.zmw_breakpoints().
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.oracle import Poa

from .pileup_ref import flags
from .quality_ref import ADDLEN, INITLEN, MINLEN, _breakpoint, column_quals, phred

_cache: dict = {}


@dataclass(frozen=True)
class StrandRef:
    ccs: bytes
    seq: tuple      # (forward bases, reverse bases), ASCII
    qual: tuple     # (forward, reverse) uint8 arrays, raw quality bytes
    calls: np.ndarray  # int8 [emitted columns, 2]: call_s of every emitted column, over all rounds
    cov: np.ndarray    # int64 [emitted columns, 2]: cov_s
    base_col: np.ndarray  # per CCS base: the index of its column among the emitted columns
    log: list       # shredded mode: (i, ncols) per round
    carry: int      # the strand bases called in the gap-consensus columns behind a round's last CCS base,
                    # summed over the rounds that another round follows
    pushed: tuple   # (forward, reverse) pushed bases


def round_calls(msa, has, i: int, rev):
    """(call int8 [i, 2], Q uint8 [i, 2], cov int64 [i, 2]) of the columns [0, i) of one POA call."""
    ncols, n = has.shape
    reads = msa[:, 1:n + 1]
    some = has.any(0)
    first = np.where(some, has.argmax(0), ncols)
    last = np.where(some, ncols - 1 - has[::-1].argmax(0), -1)
    col = np.arange(ncols)[:, None]
    span = (col >= first[None, :]) & (col <= last[None, :])
    call = np.zeros((i, 2), np.int8)
    q = np.zeros((i, 2), np.uint8)
    cov = np.zeros((i, 2), np.int64)
    for s in (0, 1):
        m = (rev == s)[None, :]
        cnt = np.stack([((reads[:i] == b) & m).sum(1) for b in range(4)], 1).astype(np.int64).reshape(i, 4)
        cov[:, s] = (span[:i] & m).sum(1)
        gap = cov[:, s] - cnt.sum(1)
        best = cnt.argmax(1)  # (the first maximum: ties go to the smallest base)
        bc = cnt[np.arange(i), best]
        call[:, s] = np.where(cov[:, s] == 0, -1, np.where(bc >= gap, best, 4))
        q[:, s] = phred(bc, cov[:, s])
    return call, q, cov


def _run(z, mode: int):
    poa = Poa()
    n = len(z.lens)
    offs = [int(x) for x in z.offs]
    lens = [int(x) for x in z.lens]
    rev = flags(z)
    ccs, log = bytearray(), []
    calls, quals, covs, base_col = [], [], [], []
    state = {"cols": 0, "carry": 0}

    def take(msa, cons, has, i, more):
        call, q, cov = round_calls(msa, has, i, rev)
        calls.append(call), quals.append(q), covs.append(cov)
        keep = np.nonzero(cons[:i] < 4)[0]
        base_col.extend(int(c) + state["cols"] for c in keep)
        ccs.extend(b"ACGT"[c] for c in cons[:i][keep])
        if more:
            t0 = int(keep[-1]) + 1 if len(keep) else 0
            state["carry"] += int(((call[t0:] >= 0) & (call[t0:] < 4)).sum())
        state["cols"] += i

    if mode == 1:
        _, msa = poa.poa([z.seqs[o:o + ln] for o, ln in zip(offs, lens)])
        cons, _, _, _, eq, has = column_quals(msa, n)
        take(msa, cons, has, len(cons), False)
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
            log.append((i, len(cons)))
            if flag:
                adv = has[:i].sum(0)
                pos = [pos[k] + int(adv[k]) for k in range(n)]
            take(msa, cons, has, i, flag)
    call = np.concatenate(calls) if calls else np.zeros((0, 2), np.int8)
    q = np.concatenate(quals) if quals else np.zeros((0, 2), np.uint8)
    cov = np.concatenate(covs) if covs else np.zeros((0, 2), np.int64)
    seq, qual = [], []
    for s in (0, 1):
        keep = (call[:, s] >= 0) & (call[:, s] < 4)
        seq.append(bytes(b"ACGT"[c] for c in call[keep, s]))
        a = q[keep, s].copy()
        a.setflags(write=False)
        qual.append(a)
    for a in (call, cov):
        a.setflags(write=False)
    pushed = tuple(int(sum(ln for ln, r in zip(lens, rev) if r == s)) for s in (0, 1))
    return StrandRef(bytes(ccs), tuple(seq), tuple(qual), call, cov, np.array(base_col, np.int64), log, state["carry"], pushed)


def reference(z, mode: int) -> StrandRef:
    """The strand consensuses of a prepared ZMW with its strand flags; computed
    once per (ZMW, flags, mode) and checked against the oracle's own loop."""
    key = (z.seqs, tuple(int(x) for x in z.offs), tuple(int(x) for x in z.lens), flags(z).tobytes(), mode)
    if key not in _cache:
        r = _run(z, mode)
        o = Poa()
        if mode == 0:
            want, wlog = o.zmw_breakpoints(z.seqs, z.offs, z.lens)
            assert r.log == [(int(a), int(b)) for a, b in wlog], "strand_ref: breakpoint log differs from the oracle's"
        else:
            want = o.zmw(z.seqs, z.offs, z.lens, mode)
        assert r.ccs == want, "strand_ref: CCS differs from the oracle's"
        assert len(r.base_col) == len(r.ccs)
        _cache[key] = r
    return _cache[key]


def fasta(name: str, r: StrandRef, fastq: bool, rev, rq) -> str:
    """The -b records of one ZMW (the CLI's layout); rev = its strand flags, rq
    = the function giving a record's rq from its raw quality bytes."""
    out = ""
    for s, tag in ((0, "fwd"), (1, "rev")):
        if not r.seq[s]:
            continue
        if fastq:
            out += "@%s/%s np=%d rq=%.6f\n%s\n+\n%s\n" % (name, tag, int((np.asarray(rev) == s).sum()), rq(r.qual[s]),
                                                        r.seq[s].decode(), bytes(int(x) + 33 for x in r.qual[s]).decode())
        else:
            out += ">%s/%s\n%s\n" % (name, tag, r.seq[s].decode())
    return out
