"""SPEC.md §17 restated with numpy, independent of host/scan.cpp: the full
(L + 1) x (n + 1) matrix per pattern, filled row by row (a row's in-row chain
H(i, j) = max(E(j), H(i, j - 1) - 2) is a running maximum of E + 2 j), the
bottom rows folded into V_a / O_a, the hit rule by brute force over every
column, the start by the anchored matrix backwards from the end, and the cut.
"""
from __future__ import annotations

import numpy as np

MATCH, PEN = 1, 2
MAX_SET, MAX_LEN = 64, 64
_CODE = np.zeros(256, np.int64)
for _ch, _c in ((b"C", 1), (b"G", 2), (b"T", 3), (b"U", 3)):
    _CODE[_ch[0]] = _CODE[_ch.lower()[0]] = _c


def codes(s: bytes) -> np.ndarray:
    """§1's coding: C 1, G 2, T / U 3, anything else 0."""
    return _CODE[np.frombuffer(bytes(s), np.uint8)]


def set_ok(adapters, T: int = 75) -> bool:
    return 1 <= len(adapters) <= MAX_SET and 1 <= T <= 100 and all(
        1 <= len(a) <= MAX_LEN and all(ch in b"ACGTacgt" for ch in a) for a in adapters)


def patterns(adapters) -> list:
    """p = 2 a + o: the adapter's codes, and those of its reverse complement."""
    out = []
    for a in adapters:
        c = codes(a)
        out += [c, 3 - c[::-1]]
    return out


def matrix(x: np.ndarray, y: np.ndarray, anchored: bool = False) -> np.ndarray:
    """H of pattern x (rows) against y (columns); row 0 is 0 (free start), or
    -2 j if anchored."""
    L, w = len(x), len(y)
    H = np.zeros((L + 1, w + 1), np.int64)
    H[:, 0] = -PEN * np.arange(L + 1)
    ramp = PEN * np.arange(w + 1)
    if anchored:
        H[0] = -ramp
    for i in range(1, L + 1):
        E = np.empty(w + 1, np.int64)
        E[0] = H[i, 0]
        if w:
            s = np.where(x[i - 1] == y, MATCH, -PEN)
            E[1:] = np.maximum(H[i - 1, :-1] + s, H[i - 1, 1:] - PEN)
        H[i] = np.maximum.accumulate(E + ramp) - ramp
    return H


def tracks(adapters, ccs: bytes) -> np.ndarray:
    """S_p(j): shape (2 A, n + 1)."""
    y = codes(ccs)
    return np.stack([matrix(x, y)[-1] for x in patterns(adapters)])


def start(adapter: bytes, orient: int, ccs: bytes, end: int) -> tuple:
    """(start, max_k G(L, k)) of a hit ending at column `end`."""
    x = patterns([adapter])[orient][::-1]
    K = min(end, 2 * len(x))
    y = codes(ccs)[end - K:end][::-1]
    last = matrix(x, y, anchored=True)[-1]
    return end - int(last.argmax()), int(last.max())  # (argmax: the smallest k)


def hits(adapters, ccs: bytes, T: int = 75) -> list:
    """[(adapter, orient, start, end, score)] by (end, adapter)."""
    assert set_ok(adapters, T)
    S = tracks(adapters, ccs)
    n = len(ccs)
    out = []
    for a, ad in enumerate(adapters):
        L = len(ad)
        V = np.maximum(S[2 * a], S[2 * a + 1])
        O = (S[2 * a] < S[2 * a + 1]).astype(int)
        cand = 100 * V >= T * L
        cand[0] = False
        for j in np.flatnonzero(cand):
            j = int(j)
            hit = True
            for k in range(max(1, j - L), min(n, j + L) + 1):
                if k != j and cand[k] and (V[k] > V[j] or (V[k] == V[j] and k < j)):
                    hit = False
                    break
            if hit:
                st, best = start(ad, int(O[j]), ccs, j)
                assert best == V[j], (a, j, best, V[j])
                out.append((a, int(O[j]), st, j, int(V[j])))
    return sorted(out, key=lambda h: (h[3], h[0]))


def cut(hit_list, n: int, lmin: int = 50) -> list:
    """[(b, e, left, right)]: the pieces and the indices of their flanking hits
    (-1 at the read's end)."""
    if not hit_list:
        return [(0, n, -1, -1)]
    covered = np.zeros(n + 1, bool)  # base k is inside a hit (covered[n]: a sentinel)
    for _, _, s, e, _ in hit_list:
        covered[s:e] = True
    covered[n] = True
    out, k = [], 0
    while k < n:
        if covered[k]:
            k += 1
            continue
        b = k
        while not covered[k]:
            k += 1
        e = k
        if e - b < max(lmin, 1):
            continue
        # the merged interval ending at b: walk back over covered bases
        left = right = -1
        if b > 0:
            lo = b
            while lo > 0 and covered[lo - 1]:
                lo -= 1
            inside = [i for i, h in enumerate(hit_list) if lo <= h[2] and h[3] <= b]
            top = max(hit_list[i][3] for i in inside)
            left = min(i for i in inside if hit_list[i][3] == top)
        if e < n:
            hi = e
            while hi < n and covered[hi]:
                hi += 1
            inside = [i for i, h in enumerate(hit_list) if e <= h[2] and h[3] <= hi]
            low = min(hit_list[i][2] for i in inside)
            right = min(i for i in inside if hit_list[i][2] == low)
        out.append((b, e, left, right))
    return out


def revcomp(s: bytes) -> bytes:
    return bytes(s)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def edit_distance(a: bytes, b: bytes) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[-1] + 1))
        prev = cur
    return prev[-1]
