"""SPEC.md §18 restated in numpy and plain Python, sharing no code with the host
or the device: the coding of a reference set, the seed over every (target,
orientation) pair (§8 step 1 with dictionaries), the ±256 band (§8 step 2, a row
at a time: the in-row chain H(k) = max(E(k), H(k-1) - 2) as a running maximum
of E(k') + 2 k'), the traceback (§8 step 3) and the §11 words of its path.
record() gives the fifteen fields in cx.REF_FIELDS' order and the words."""
from __future__ import annotations

import numpy as np

K, BIN, HALF, OCC = 13, 32, 256, 64
BW = 2 * HALF + 1
MISMATCH, INS = 0x40000000, 0x80000000
UNMAPPED = (-1,) + (0,) * 14


def revcomp(s: bytes) -> bytes:
    return bytes(s)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def read_codes(ccs: bytes) -> np.ndarray:
    """§1's coding of a read: C 1, G 2, T / U 3, anything else 0."""
    lut = np.zeros(256, np.uint8)
    for ch, c in ((b"c", 1), (b"g", 2), (b"t", 3), (b"u", 3)):
        lut[ch[0]] = lut[ch.upper()[0]] = c
    return lut[np.frombuffer(bytes(ccs), np.uint8)]


def target_codes(t: bytes):
    """ACGT in either case 0..3, another letter 4; None for anything else."""
    out = np.zeros(len(t), np.uint8)
    for i, ch in enumerate(bytes(t).upper()):
        if not 65 <= ch <= 90:
            return None
        out[i] = b"ACGT".index(ch) if ch in b"ACGT" else 4
    return out


def set_ok(refs) -> bool:
    return (1 <= len(refs) <= 64 and all(len(t) >= K for t in refs) and sum(len(t) for t in refs) <= 1 << 20
            and all(target_codes(t) is not None for t in refs))


def kmers(c) -> list:
    """(position, k-mer) of every window of 13 codes below 4."""
    out, h, valid = [], 0, 0
    for i, x in enumerate(c):
        if x > 3:
            valid = 0
            continue
        h = ((h << 2) | int(x)) & ((1 << 2 * K) - 1)
        valid += 1
        if valid >= K:
            out.append((i + 1 - K, h))
    return out


def seed(q, t) -> dict:
    """§8 step 1 of one pair: votes per bin of 32 diagonals (floored)."""
    idx: dict = {}
    for p, h in kmers(t):
        idx.setdefault(h, []).append(p)
    votes: dict = {}
    for qp, h in kmers(q):
        ps = idx.get(h, ())
        if len(ps) > OCC:
            continue
        for tp in ps:
            b = (tp - qp) // BIN  # Python's // floors
            votes[b] = votes.get(b, 0) + 1
    return votes


def pair_best(votes: dict):
    """(votes, bin) of a pair: the most votes, then the smallest bin; None without a vote."""
    if not votes:
        return None
    b = min(votes, key=lambda x: (-votes[x], x))
    return votes[b], b


def band(q, t, d0: int):
    """§8 steps 2 and 3: the ten fields and the path's words; None for no
    positive cell."""
    n, m = len(q), len(t)
    q = np.asarray(q, np.int64)
    t = np.asarray(t, np.int64)
    lo = d0 - HALF
    ks = np.arange(BW)
    dirs = np.zeros((n, BW), np.uint8)
    prev = np.zeros(BW + 2, np.int64)  # prev[k + 1] = H(i - 1, k)
    best, bi, bk = 0, -1, -1
    for i in range(n):
        j = i + lo + ks
        ok = (j >= 0) & (j < m)
        tj = t[np.clip(j, 0, max(m - 1, 0))] if m else np.zeros(BW, np.int64)
        same = ok & (q[i] < 4) & (tj == q[i])
        diag = np.where((i > 0) & (j > 0), prev[1:BW + 1], 0) + np.where(same, 1, -2)
        up = np.where((i > 0) & (ks + 1 < BW), prev[2:BW + 2], 0) - 2
        e = np.maximum(0, np.maximum(diag, up))
        e = np.where(ok, e, 0)
        # H(k) = max over k' <= k of E(k') - 2 (k - k'); cells outside the target hold 0, which never wins
        h = np.maximum.accumulate(e + 2 * ks) - 2 * ks
        h = np.where(ok, np.maximum(h, e), 0)
        left = np.concatenate(([0], h[:-1])) - 2
        d = np.where(diag > 0, 1, 0)
        d = np.where(up > np.maximum(0, diag), 2, d)
        d = np.where(left > e, 3, d)
        dirs[i] = np.where(ok & (h > 0), d, 0)
        prev[1:BW + 1] = h
        k = int(np.argmax(h))  # the first of the row's largest
        if h[k] > best:
            best, bi, bk = int(h[k]), i, k
    if bi < 0:
        return None
    words = [INS] * n
    i, k = bi, bk
    qe, te = bi + 1, bi + lo + bk + 1
    qb = tb = 0
    mat = mis = ins = dele = 0
    while True:
        d = dirs[i, k]
        if d == 0:
            break
        j = i + lo + k
        if d == 1:
            s = q[i] < 4 and q[i] == t[j]
            mat, mis = mat + bool(s), mis + (not s)
            words[i] = j | (0 if s else MISMATCH)
            qb, tb = i, j
            i -= 1
        elif d == 2:
            ins += 1
            words[i] = INS | (j + 1)
            qb = i
            i, k = i - 1, k + 1
        else:
            dele += 1
            tb = j
            k -= 1
        if i < 0 or k < 0 or k >= BW:
            break
    for w in range(qb):
        words[w] = INS | tb
    for w in range(qe, n):
        words[w] = INS | te
    return (qb, qe, tb, te, mat, mis, ins, dele, mat + mis + ins + dele, best), np.array(words, np.uint32)


def record(refs, ccs: bytes, with_votes: bool = False):
    """§18 of one read: (the fifteen fields, the words of the read in
    orientation o).  with_votes: also {(g, o): (votes, bin)}."""
    ts = [target_codes(t) for t in refs]
    n = len(ccs)
    c = read_codes(ccs)
    qs = (c, (3 - c[::-1]).astype(np.uint8))
    pairs = {}
    for g, t in enumerate(ts):
        for o in (0, 1):
            pb = pair_best(seed(qs[o], t))
            if pb:
                pairs[(g, o)] = pb
    unmapped = (UNMAPPED, np.full(n, INS, np.uint32))
    out = unmapped
    if pairs:
        g, o = min(pairs, key=lambda p: (-pairs[p][0], 2 * p[0] + p[1]))
        votes, b = pairs[(g, o)]
        votes2 = max([v for (g2, _), (v, _) in pairs.items() if g2 != g], default=0)
        d0 = b * BIN + BIN // 2
        r = band(qs[o], ts[g], d0)
        if r:
            out = ((g, o, d0, votes, votes2) + r[0], r[1])
    return out + (pairs,) if with_votes else out


def cigar(words, n: int):
    """§11's alignment of a word list, restated: (qs, qe, ts, te, n_eq, n_x,
    n_ins, n_del, cigar) or None without an aligned word."""
    al = [i for i in range(n) if not int(words[i]) & INS]
    if not al:
        return None
    qs, qe = al[0], al[-1] + 1
    ops: list = []

    def put(op, k=1):
        if ops and ops[-1][0] == op:
            ops[-1][1] += k
        else:
            ops.append([op, k])

    prev = None
    for i in range(qs, qe):
        w = int(words[i])
        if w & INS:
            put("I")
            continue
        off = w & 0x3FFFFFFF
        if prev is not None and off - prev - 1 > 0:
            put("D", off - prev - 1)
        put("X" if w & MISMATCH else "=")
        prev = off
    cnt = {op: sum(k for o, k in ops if o == op) for op in "=XID"}
    return (qs, qe, int(words[qs]) & 0x3FFFFFFF, (int(words[qe - 1]) & 0x3FFFFFFF) + 1, cnt["="], cnt["X"], cnt["I"], cnt["D"],
            "".join(f"{k}{op}" for op, k in ops))


def passes(rec, y: int = 50, Y: int = 75) -> bool:
    return rec[0] >= 0 and rec[13] >= y and 100 * rec[9] >= Y * rec[13]


def paf_line(name: str, ccs: bytes, rec, words, tname: str, tlen: int) -> str:
    """The -g line of a reported read (SPEC.md §18)."""
    n = len(ccs)
    g, o, d0, votes, votes2, qb, qe, tb, te, mat, mis, ins, dele, aln, score = rec
    qs, qend = (n - qe, n - qb) if o else (qb, qe)
    return (f"{name}\t{n}\t{qs}\t{qend}\t{'-' if o else '+'}\t{tname}\t{tlen}\t{tb}\t{te}\t{mat}\t{aln}\t255\t"
            f"AS:i:{score}\tsv:i:{votes}\ts2:i:{votes2}\tcg:Z:{cigar(words, n)[8]}\n")
