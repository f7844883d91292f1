"""Inputs of the kinetics tests (SPEC.md §13), seeded and deterministic: per-base
code planes over all 256 values, the strand patterns, a planted signal, and a
BAM writer with aux tags (tools/gen_synth.write_bam plus the ip / pw arrays)."""
from __future__ import annotations

import struct

import numpy as np

import ccsx_amd as cx
from tools.gen_synth import _NT16, _bgzf_block


def codes(n: int, seed: int):
    """(ipd, pw): n seeded bytes each, every value 0..255 occurring (n >= 256)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    if n >= 256:
        a[rng.permutation(n)[:256]] = np.arange(256, dtype=np.uint8)
        b[rng.permutation(n)[:256]] = np.arange(256, dtype=np.uint8)
    return a.tobytes(), b.tobytes()


def alternating(n: int) -> np.ndarray:
    return (np.arange(n) & 1).astype(np.uint8)


def all_reverse(n: int) -> np.ndarray:
    return np.ones(n, np.uint8)


def at_63_64(n: int) -> np.ndarray:
    """Flags set only at reads 63 and 64: the last bit of mask word 0, the first of word 1."""
    r = np.zeros(n, np.uint8)
    r[[63, 64]] = 1
    return r


def patterns(n: int) -> dict:
    """Every strand pattern that fits n segments (None: all forward via NULL)."""
    p = {"alternating": alternating(n), "null": None, "all_reverse": all_reverse(n)}
    if n >= 65:
        p["at_63_64"] = at_63_64(n)
    return p


def with_kin(z, rev="keep", seed: int = 1, planes: bool = True) -> cx.Prepared:
    """z with strand flags (rev; "keep": its own) and seeded planes (planes=False: none)."""
    r = getattr(z, "rev", None) if isinstance(rev, str) else rev
    ipd, pw = codes(len(z.seqs), seed) if planes else (None, None)
    return cx.Prepared(z.seqs, z.offs, z.lens, None if r is None else np.asarray(r, np.uint8), ipd, pw)


PLANT = {ord("A"): 10, ord("C"): 70, ord("G"): 130, ord("T"): 200}


def planted_pw(seq: bytes) -> bytes:
    """A pw code fixed by the base's letter (upper case ACGT)."""
    return bytes(PLANT[c] for c in seq)


def aux_array(tag: bytes, sub: bytes, values, count=None) -> bytes:
    """One B-typed aux field; count overrides the stored element count."""
    fmt = {b"C": "B", b"S": "H", b"c": "b", b"s": "h", b"I": "I", b"i": "i", b"f": "f"}[sub]
    v = list(values)
    return tag + b"B" + sub + struct.pack("<I", len(v) if count is None else count) + struct.pack("<%d%s" % (len(v), fmt), *v)


def write_bam(path, recs):
    """Unaligned BAM of (name, seq, aux bytes) records (gen_synth.write_bam with
    aux data behind the qualities; aux may be any bytes, also a field cut short)."""
    text = b"@HD\tVN:1.5\tSO:unknown\n"
    raw = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0))
    out = bytearray()

    def flush(final=False):
        nonlocal raw
        while len(raw) >= 0xFF00 or (final and raw):
            out.extend(_bgzf_block(bytes(raw[:0xFF00])))
            del raw[:0xFF00]

    for name, seq, aux in recs:
        rn = name + b"\0"
        n = len(seq)
        cs = [_NT16.get(c, 15) for c in seq.upper()]
        if n & 1:
            cs.append(0)
        packed = bytes((cs[i] << 4) | cs[i + 1] for i in range(0, len(cs), 2))
        core = struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | (255 << 8) | len(rn), 4 << 16, n, -1, -1, 0)
        rec = core + rn + packed + bytes([20]) * n + aux
        raw += struct.pack("<i", len(rec)) + rec
        flush()
    flush(final=True)
    out.extend(_bgzf_block(b""))
    with open(path, "wb") as f:
        f.write(out)


def names(hole: int, lens) -> list:
    """Subread names movie/hole/qs_qe of one ZMW."""
    out, q = [], 0
    for ln in lens:
        out.append(b"mv/%d/%d_%d" % (hole, q, q + ln))
        q += ln
    return out


def rand_seqs(rng, lens) -> list:
    return [bytes(b"ACGT"[x] for x in rng.integers(0, 4, ln)) for ln in lens]


def tagged_records(recs, seed: int = 5, sub: bytes = b"C"):
    """(name, seq) records -> (name, seq, aux) with seeded ip / pw arrays (B:C
    codes, or with sub = b"S" frames up to 1,200) and a few other tags around
    them; also returns the codes each record must be read as."""
    rng = np.random.default_rng(seed)
    out, want = [], []
    from tests.kinetics_ref import code
    for name, seq in recs:
        n = len(seq)
        if sub == b"C":
            ip, pw = rng.integers(0, 256, n), rng.integers(0, 256, n)
            want.append((bytes(int(x) for x in ip), bytes(int(x) for x in pw)))
        else:
            ip, pw = rng.integers(0, 1201, n), rng.integers(0, 1201, n)
            want.append((bytes(code(int(x)) for x in ip), bytes(code(int(x)) for x in pw)))
        aux = b"zmi\x07\x00\x00\x00" + b"RGZgroup\0" + aux_array(b"ip", sub, ip) + b"snBf" + struct.pack("<I4f", 4, 1, 2, 3, 4) + \
            aux_array(b"pw", sub, pw) + b"cxC\x03"
        out.append((name, seq, aux))
    return out, want
