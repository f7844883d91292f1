"""SPEC.md §16 restated with numpy, independent of host/barcode.cpp: the full
(L + 1) x (w + 1) matrix per (pattern, end), filled row by row (a row's in-row
chain H(i, j) = max(E(j), H(i, j - 1) - 2) is a running maximum of E + 2 j),
the five values per end from all patterns' scores, and the call.
"""
from __future__ import annotations

import numpy as np

NONE = -(1 << 31)
MATCH, PEN = 1, 2
MAX_SET, MAX_LEN, MAX_WIN = 2048, 64, 256
_CODE = np.zeros(256, np.int64)
for _ch, _c in ((b"C", 1), (b"G", 2), (b"T", 3), (b"U", 3)):
    _CODE[_ch[0]] = _CODE[_ch.lower()[0]] = _c


def codes(s: bytes) -> np.ndarray:
    """§1's coding: C 1, G 2, T / U 3, anything else 0."""
    return _CODE[np.frombuffer(bytes(s), np.uint8)]


def set_ok(barcodes) -> bool:
    return 1 <= len(barcodes) <= MAX_SET and all(
        1 <= len(b) <= MAX_LEN and all(ch in b"ACGTacgt" for ch in b) for b in barcodes)


def patterns(barcodes) -> list:
    """p = 2 b + o: the barcode's codes, and those of its reverse complement."""
    out = []
    for b in barcodes:
        c = codes(b)
        out += [c, 3 - c[::-1]]
    return out


def ends(ccs: bytes, window: int) -> tuple:
    c = codes(ccs)
    w = min(len(c), window)
    return c[:w], (3 - c[::-1])[:w]


def matrix(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    L, w = len(x), len(y)
    H = np.zeros((L + 1, w + 1), np.int64)
    H[:, 0] = -PEN * np.arange(L + 1)
    ramp = PEN * np.arange(w + 1)
    for i in range(1, L + 1):
        E = np.empty(w + 1, np.int64)
        E[0] = H[i, 0]
        if w:
            s = np.where(x[i - 1] == y, MATCH, -PEN)
            E[1:] = np.maximum(H[i - 1, :-1] + s, H[i - 1, 1:] - PEN)
        H[i] = np.maximum.accumulate(E + ramp) - ramp
    return H


def align(x: np.ndarray, y: np.ndarray) -> tuple:
    last = matrix(x, y)[-1]
    return int(last.max()), int(last.argmax())  # (argmax: the first maximum)


def score_end(pats, y: np.ndarray) -> tuple:
    """(pattern, score, end, second, second_pattern) of one end."""
    se = [align(x, y) for x in pats]
    sc = np.array([s for s, _ in se])
    p = int(sc.argmax())
    other = np.arange(len(pats)) >> 1 != p >> 1
    if not other.any():
        return p, int(sc[p]), se[p][1], NONE, -1
    masked = np.where(other, sc, sc.min() - 1)
    q = int(masked.argmax())
    return p, int(sc[p]), se[p][1], int(sc[q]), q


def score(barcodes, ccs: bytes, window: int = 96) -> tuple:
    assert set_ok(barcodes) and 1 <= window <= MAX_WIN
    pats = patterns(barcodes)
    e0, e1 = ends(ccs, window)
    return score_end(pats, e0), score_end(pats, e1)


def call(result, lens, n: int, T: int = 60, D: int = 3) -> tuple:
    """(cl, cr, (called0, called1), assigned, reason) as cx.barcode_call gives."""
    called = []
    for p, s, _, second, _ in result:
        called.append(100 * s >= T * int(lens[p >> 1]) and (len(lens) == 1 or s - second >= D))
    cl = result[0][2] if called[0] else 0
    cr = result[1][2] if called[1] else 0
    if not called[0] and not called[1]:
        reason = 3
    elif not called[0]:
        reason = 1
    elif not called[1]:
        reason = 2
    else:
        reason = 4 if cl + cr >= n else 0
    return cl, cr, (called[0], called[1]), reason == 0, reason


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
