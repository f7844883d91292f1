"""Reference for the polish step (SPEC.md §15): an independent numpy restatement
of the realignment of every pushed segment to the draft CCS in a 64-cell band
guided by its §11 map, the per-position vote and the polished read.  The
in-row chain is the sequential cell loop of the definition, not a scan; the
votes are counted piece by piece from the definition's f and l.

polish(ccs, segs, maps) -> (seq, qual, (nsub, nins, ndel), [realigned map per
segment], status), the tuple ccsx_amd.Polisher.polish and ccsx_amd.polish_host
return.  mutate() is the deterministic subread generator of the accuracy case.
"""
from __future__ import annotations

import numpy as np

OFFSET, MISMATCH, INS = (1 << 30) - 1, 1 << 30, 1 << 31
W, HALF, NEG = 64, 32, -(1 << 29)
Q_STEP, Q_MIN, Q_MAX = 3, 2, 93  # SPEC.md §9
BAD_MAP = 1

_LUT = np.zeros(256, np.int64)
for _ch, _v in (("c", 1), ("g", 2), ("t", 3), ("u", 3)):
    _LUT[ord(_ch)] = _LUT[ord(_ch.upper())] = _v


def codes(s: bytes) -> np.ndarray:
    return _LUT[np.frombuffer(s, np.uint8)]


def mutate(rng, s, ps, pi, pd):      # rng = random.Random(seed)
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < pd: continue
        out.append(rng.choice([c for c in b"ACGT" if c != ch]) if r < pd + ps else ch)
        while rng.random() < pi: out.append(rng.choice(b"ACGT"))
    return bytes(out)


def qual(match: int, cov: int) -> int:
    return min(max(Q_STEP * (2 * match - cov), Q_MIN), Q_MAX)


def map_ok(maps, n: int) -> bool:
    for w in maps:
        a = (np.asarray(w, np.int64) & OFFSET)
        if len(a) and ((np.diff(a) < 0).any() or (a > n).any()):
            return False
    return True


def realign(c: np.ndarray, r: np.ndarray, w) -> tuple:
    """One non-empty segment r (codes) against the draft c (codes, n >= 1) with
    anchors from w: (realigned map, [(first row, last row)] of its pieces)."""
    n, m = len(c), len(r)
    lo = np.clip((np.asarray(w, np.int64) & OFFSET) - HALF, 0, max(n - W, 0))
    cpad = np.concatenate([c, np.full(W, 4, np.int64)])
    tt = np.arange(W)
    dirs = np.zeros((m, W), np.uint8)
    pieces = []  # [first row, last row, end cell]
    prev = None
    for i in range(m):
        first = i == 0 or lo[i] - lo[i - 1] >= W
        if first:
            if i:
                pieces[-1][1:] = [i - 1, int(np.argmax(prev))]
            pieces.append([i, i, 0])
            pu = pd = np.zeros(W, np.int64)
        else:
            d = int(lo[i] - lo[i - 1])
            ext = np.concatenate([[NEG], prev, np.full(W, NEG, np.int64)])  # ext[k + 1] = H(i-1, k)
            pu, pd = ext[1 + tt + d], ext[tt + d]
        j = lo[i] + tt
        diag = pd + np.where(cpad[j] == r[i], 1, -2)
        up = pu - 2
        e = np.where(up > diag, up, diag).tolist()
        dr = np.where(up > diag, 2, 1).tolist()
        nv = int(min(W, n - lo[i]))  # the valid cells are the first nv
        h = [NEG] * W
        left = NEG
        for t in range(nv):
            v = e[t]
            if left > v:
                v, dr[t] = left, 3
            h[t] = v
            left = v - 2
        dr[nv:] = [0] * (W - nv)
        dirs[i] = dr
        prev = np.array(h, np.int64)
    pieces[-1][1:] = [m - 1, int(np.argmax(prev))]
    out = np.zeros(m, np.int64)
    for first, last, t in pieces:
        i, j = last, int(lo[last]) + t
        while i >= first:
            d = dirs[i, j - lo[i]]
            assert d in (1, 2, 3) and 0 <= j - lo[i] < W, "polish_ref: the path left the band"
            if d == 1:
                out[i] = j | (MISMATCH if r[i] != c[j] else 0)
                i, j = i - 1, j - 1
            elif d == 2:
                out[i] = INS | (j + 1)
                i -= 1
            else:
                j -= 1
    return out.astype(np.uint32), [(f, l) for f, l, _ in pieces]


def polish(ccs: bytes, segs, maps):
    n = len(ccs)
    if not map_ok(maps, n):
        return b"", b"", (0, 0, 0), [], BAD_MAP
    if n == 0:
        return b"", b"", (0, 0, 0), [np.full(len(s), INS, np.uint32) for s in segs], 0
    c = codes(ccs)
    cnt = np.zeros((n + 1, 4), np.int64)
    insb = np.zeros((n + 1, 4), np.int64)
    cov, covs, insn = (np.zeros(n + 1, np.int64) for _ in range(3))
    outmaps = []
    for s, w in zip(segs, maps):
        if not len(s):
            outmaps.append(np.zeros(0, np.uint32))
            continue
        r = codes(s)
        wo, pieces = realign(c, r, w)
        outmaps.append(wo)
        for first, last in pieces:
            ent = [(int(wo[i]), int(r[i])) for i in range(first, last + 1)]
            al = [e & OFFSET for e, _ in ent if not e & INS]
            if not al:
                continue
            f, l = al[0], al[-1]
            cov[f:l + 1] += 1
            covs[f + 1:l + 1] += 1
            slots = set()
            for e, x in ent:
                g = e & OFFSET
                if not e & INS:
                    cnt[g, x] += 1
                elif f < g <= l and g not in slots:
                    slots.add(g)
                    insn[g] += 1
                    insb[g, x] += 1
    seq, q = bytearray(), bytearray()
    nsub = nins = ndel = 0
    for g in range(n + 1):
        if 2 * insn[g] > covs[g]:
            x = int(np.argmax(insb[g]))
            seq.append(b"ACGT"[x])
            q.append(qual(int(insb[g, x]), int(covs[g])))
            nins += 1
        if g == n:
            break
        if cov[g] == 0:
            seq.append(b"ACGT"[c[g]])
            q.append(Q_MIN)
            continue
        best = int(np.argmax(cnt[g]))
        gap = int(cov[g] - cnt[g].sum())
        if cnt[g, best] >= gap:
            seq.append(b"ACGT"[best])
            q.append(qual(int(cnt[g, best]), int(cov[g])))
            nsub += int(best != c[g])
        else:
            ndel += 1
    return bytes(seq), bytes(q), (nsub, nins, ndel), outmaps, 0


def check_map_invariants(ccs: bytes, seg: bytes, m) -> None:
    """SPEC.md §11's invariants on one realigned map."""
    w = np.asarray(m, np.int64)
    off, ins, mis = w & OFFSET, (w & INS) != 0, (w & MISMATCH) != 0
    assert len(w) == len(seg)
    assert not (ins & mis).any()
    assert (np.diff(off) >= 0).all()
    assert (np.diff(off[~ins]) > 0).all()
    assert (off <= len(ccs)).all() and (off[~ins] < len(ccs)).all()
    c, r = codes(ccs), codes(seg)
    al = np.nonzero(~ins)[0]
    assert ((r[al] == c[off[al]]) == ~mis[al]).all()
