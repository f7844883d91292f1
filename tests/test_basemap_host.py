"""Subread-to-CCS coordinate map, CPU side (SPEC.md §11): the reference's
self-check against the oracle and the invariants of the definition on the edge
cases and multi-round ZMWs, the exported ccsx_map_cigar against the Python
statement of the derived alignment (on those maps and on hand-written ones),
anchor alignments from the band cases, and the CLI's help text.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from ccsx_amd.build import BIN

from . import basemap_ref as br
from .zmw_cases import band_cases, edge_cases, raw, synth

CASES = edge_cases()
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
MULTI = [(5000, 5), (9000, 3), (3500, 11)]
I, X = br.INS, br.MISMATCH

# band_cases() in -P mode: read -> (qs, qe, ts, te), CIGAR
ANCHORS = {
    "del64": {2: ((0, 436, 0, 500), "200=64D236="), 3: ((0, 436, 0, 500), "200=64D236=")},
    "inner_64": {2: ((0, 372, 64, 436), "372=")},
    # (read 1's 200 trailing insertions lie outside its alignment)
    "bubble_100_lost": {4: ((0, 400, 0, 500), "198=100D202="), 1: ((0, 200, 0, 200), "200=")},
}


def _same(m):
    got, want = cx.map_cigar(m), br.cigar(m)
    assert got == want
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_invariants_edge_cases(name, mode):
    # reference() asserts its CCS against pass_ref's, which asserts the oracle's
    for m in br.check_invariants(CASES[name], mode):
        _same(m)


@pytest.mark.parametrize("L,passes", MULTI)
def test_reference_invariants_multi_round(L, passes):
    z = synth(3, L, passes)
    assert len(br.pr.reference(z, cx.MODE_SHRED)[2]) >= 2
    for mode in MODES:
        for m in br.check_invariants(z, mode):
            a = _same(m)
            # the CIGAR consumes the alignment's query and CCS bases
            assert a["n_eq"] + a["n_x"] + a["n_ins"] == a["qe"] - a["qs"]
            assert a["n_eq"] + a["n_x"] + a["n_del"] == a["te"] - a["ts"]


def test_empty_segment_has_an_empty_map():
    z = CASES["with_empty_segment"]
    empty = [k for k, ln in enumerate(z.lens) if int(ln) == 0]
    assert empty
    for mode in MODES:
        maps = br.reference(z, mode)[1]
        assert all(len(maps[k]) == 0 and cx.map_cigar(maps[k]) is None for k in empty)


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_band_case_anchors(name):
    z = raw(band_cases()[name])
    for mode in MODES:  # (shredded mode gives the same maps: one final round)
        maps = br.check_invariants(z, mode)
        for k, (coords, cg) in ANCHORS[name].items():
            a = _same(maps[k])
            assert (a["qs"], a["qe"], a["ts"], a["te"]) == coords and a["cigar"] == cg, (k, a)
    if name == "bubble_100_lost":
        # read 1 is 200 + 100 + 200 bases: the lost branch and the rest of the read, 300 entries
        tail = br.reference(z, cx.MODE_PRIMITIVE)[1][1][200:]
        assert len(tail) == 300 and (tail & I).all()


HAND = [
    ([], None),
    ([I | 0, I | 0, I | 3], None),
    ([5], dict(qs=0, qe=1, ts=5, te=6, n_eq=1, n_x=0, n_ins=0, n_del=0, cigar="1=")),
    # leading and trailing insertions lie outside the alignment
    ([I | 2, I | 2, 2, 3, I | 4, 4, I | 5, I | 5],
     dict(qs=2, qe=6, ts=2, te=5, n_eq=3, n_x=0, n_ins=1, n_del=0, cigar="2=1I1=")),
    # a deletion of 1, adjacent merges across it, a mismatch run
    ([0, 1, 3, X | 4, X | 5, 6], dict(qs=0, qe=6, ts=0, te=7, n_eq=4, n_x=2, n_ins=0, n_del=1, cigar="2=1D1=2X1=")),
    # a deletion of 2^20
    ([7, 7 + (1 << 20) + 1], dict(qs=0, qe=2, ts=7, te=9 + (1 << 20), n_eq=2, n_x=0, n_ins=0, n_del=1 << 20,
                                 cigar="1=1048576D1=")),
    # insertions between two aligned bases that are adjacent in the CCS; two deletions around an insertion
    ([X | 0, I | 1, I | 1, 1, 4, I | 5, 7],
     dict(qs=0, qe=7, ts=0, te=8, n_eq=3, n_x=1, n_ins=3, n_del=4, cigar="1X2I1=2D1=1I2D1=")),
    # the largest offset
    ([(1 << 30) - 2, I | (1 << 30) - 1], dict(qs=0, qe=1, ts=(1 << 30) - 2, te=(1 << 30) - 1, n_eq=1, n_x=0, n_ins=0,
                                              n_del=0, cigar="1=")),
]


@pytest.mark.parametrize("m,want", HAND)
def test_map_cigar_hand_written(m, want):
    assert br.cigar(m) == want
    assert cx.map_cigar(np.asarray(m, np.uint32)) == want


def test_map_cigar_small_cap():
    """The length is computed whatever cap is; nothing is written beyond cap."""
    L = cx.lib()
    m = np.asarray([0, 1, 3, X | 4, X | 5, 6], np.uint32)
    full = b"2=1D1=2X1="
    aln = (C.c_uint32 * 8)()
    for cap in range(0, len(full) + 3):
        buf = C.create_string_buffer(b"#" * 32, 32)
        n = L.ccsx_map_cigar(m.ctypes.data, len(m), aln, buf if cap else None, cap)
        assert n == len(full) and list(aln) == [0, 6, 0, 7, 4, 2, 0, 1]
        raw_ = buf.raw
        assert raw_[cap:] == b"#" * (32 - cap)
        if cap:
            k = min(cap - 1, len(full))
            assert raw_[:k] == full[:k] and raw_[k] == 0
    # no aligned entry: -1, the record zeroed, an empty string
    ins = np.asarray([I | 1, I | 1], np.uint32)
    buf = C.create_string_buffer(b"#" * 8, 8)
    aln[0] = 9
    assert L.ccsx_map_cigar(ins.ctypes.data, 2, aln, buf, 8) == -1 and list(aln) == [0] * 8 and buf.raw[0] == 0
    assert L.ccsx_map_cigar(None, 0, None, None, 0) == -1


def test_cli_help_lists_a():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True, timeout=30)
    assert any(line.startswith("-a") for line in r.stdout.splitlines()), r.stdout
