"""ctypes bindings of oracle/liboracle.so -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use
this module, as the checker.  The product (ccsx_amd/) never imports it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboracle.so")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            import sys
            sys.path.insert(0, os.path.dirname(_HERE))
            from ccsx_amd.build import build_oracle
            build_oracle()
        L = C.CDLL(LIB_PATH)
        L.opoa_init.argtypes = [C.c_int] * 5
        L.opoa_init.restype = C.c_void_p
        L.opoa_free.argtypes = [C.c_void_p]
        L.opoa_beg.argtypes = [C.c_void_p]
        L.opoa_push.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
        L.opoa_end.argtypes = [C.c_void_p]
        L.opoa_tidy_msa.argtypes = [C.c_void_p]
        L.opoa_cns.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.opoa_cns.restype = C.c_uint32
        L.opoa_msa.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.opoa_msa.restype = C.c_uint32
        L.opoa_cells.argtypes = [C.c_void_p]
        L.opoa_cells.restype = C.c_uint64
        L.opoa_nrows.argtypes = [C.c_void_p]
        L.opoa_nrows.restype = C.c_uint32
        L.opoa_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.ocsx_zmw.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                               C.c_uint32, C.c_char_p]
        L.ocsx_zmw.restype = C.c_size_t
        if True:
            L.ocsx_batch.argtypes = [C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_char_p),
                                     C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_uint64)]
        L.ocsx_zmw_log.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        L.ocsx_zmw_log.restype = C.c_size_t
        L.ocsx_edit_distance.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32]
        L.ocsx_edit_distance.restype = C.c_int64
        L.oprep_prepare.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
        L.oprep_prepare.restype = C.c_uint32
        L.oprep_prepare_apply.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]
        L.oprep_prepare_apply.restype = C.c_uint32
        L.oprep_pairwise.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
        L.oprep_pairwise.restype = OprepAln
        for f in ("opoa_row_kinds", "opoa_tb_moves", "opoa_tb_hist", "opoa_band_hist", "opoa_tb_events",
                  "opoa_tie_hist", "opoa_shred_hist"):
            getattr(L, f).argtypes = [C.POINTER(C.c_uint64), C.c_int]
            getattr(L, f).restype = None
        L.opoa_shred_bins.argtypes = []
        L.opoa_set_counting.argtypes = [C.c_int]
        L.opoa_set_counting.restype = None
        _lib = L
    return _lib


# ------------------------------------------------------- debug counters
# Process-wide counters of oracle/poa_oracle.c, summed over every DP and
# traceback since the last reset.  Read them single-threaded, around Poa calls
# (never around batch(), whose threads would race on them).  tb_hist,
# band_hist, tb_events, tie_hist and shred_hist count only inside `with counting():`.
TB_STATES = ("M", "D")
TB_CLASSES = ("np1", "np2", "np3_4", "np5+")  # the moved-from row's predecessor count
TB_RES = 32                                   # ... its index mod 32
TB_DIST = 35                                  # distance bins: d for 1..33, 34 = longer
BAND_BINS = ("shift_neg", "shift_0", "shift_1", "shift_2", "shift_3_63", "shift_ge64", "clamp_lo", "clamp_hi",
             "clamp_short", "partial", "rows", "dps")
TB_EVENTS = ("tracebacks", "lead", "msrc0", "trail_ins", "iext_chain", "dext_chain")
TIES = ("rmax", "rarg", "mh", "src", "dpred", "dext", "dm", "ins", "iext", "end", "best", "gap")
# opoa_shred_hist (the enum of oracle/poa_oracle.c, in its order)
SHRED_BINS = (("rounds_1", "rounds_2", "rounds_3_5", "rounds_ge6",
               "fin_n_lt3", "fin_empty", "fin_exact", "fin_read0_only", "fin_last_only", "fin_ragged", "notfin_by1",
               "grow_0", "grow_1", "grow_2", "grow_ge3", "grow_found", "grow_final", "push_gt4096",
               "d0", "d1_62", "d63", "d64", "d65", "d66_126", "d127", "d128", "d_ge129", "d_gt1000",
               "i_le16", "i_1", "i_2", "none_mult64", "none_lt64",
               "rej_leadgap", "gap_skip", "rej_nog_lt5", "acc_nog5", "acc_nog6_9", "acc_nog10",
               "rej_col_by1", "acc_col_eq_n5", "acc_col_eq_n10", "acc_n9_c6", "acc_n9_c7", "rej_n10_c6", "rej_n10_c7",
               "rej_row_by1", "acc_row_eq_nog5", "acc_row_eq_nog10") +
              tuple(f"rej_col_off{x}" for x in range(10)) +
              ("adv_differ", "gapcol_base", "rows_i_ge2", "rows_im1_ge2", "colrow_mod0", "colrow_mod1", "colrow_mod63",
               "i_mod0", "i_mod1", "i_mod63", "n3", "n9", "n10", "n63", "n64", "n65", "n128", "n129", "nobase",
               "next_exact", "fin_i_mod0", "fin_i_mod1", "fin_i_mod63",
               "ccs_cross64", "span_end_edge", "span_beg_edge", "fin_nobase"))


def _counter(fn: str, n: int, reset: bool) -> np.ndarray:
    out = np.zeros(n, np.uint64)
    getattr(lib(), fn)(out.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if reset else 0)
    return out


def tb_hist(reset: bool = False) -> np.ndarray:
    """Traceback predecessor moves, uint64 [state, class, row mod 32, distance
    bin] (TB_STATES, TB_CLASSES, TB_RES, TB_DIST)."""
    return _counter("opoa_tb_hist", len(TB_STATES) * len(TB_CLASSES) * TB_RES * TB_DIST, reset).reshape(
        len(TB_STATES), len(TB_CLASSES), TB_RES, TB_DIST)


def band_hist(reset: bool = False) -> dict:
    """DP rows by band shift off_r - off_{r-1}, by the §3.1 clamp that acted
    (at 0, at m - W, at 0 from above for reads within one band), rows whose
    band holds cells with j >= m, all rows, DPs (BAND_BINS)."""
    return dict(zip(BAND_BINS, (int(x) for x in _counter("opoa_band_hist", len(BAND_BINS), reset))))


def tb_events(reset: bool = False) -> dict:
    """Tracebacks, and those with LEAD events (MSRC at j > 0), MSRC at j = 0,
    trailing INS after the end cell; iext and D-ext chains of length >= 2
    (TB_EVENTS)."""
    return dict(zip(TB_EVENTS, (int(x) for x in _counter("opoa_tb_events", len(TB_EVENTS), reset))))


def tie_hist(reset: bool = False) -> dict:
    """Comparisons with equal operands, by the SPEC.md tie rule that settles
    them (TIES): §3.1 rmax / rarg, §3.2 mh / src / dpred / dext / dm, §3.4
    ins / iext, §3.5 end, §6 best / gap."""
    return dict(zip(TIES, (int(x) for x in _counter("opoa_tie_hist", len(TIES), reset))))


def shred_hist(reset: bool = False) -> dict:
    """What the shredding loop of Poa.zmw / Poa.zmw_breakpoints met (SHRED_BINS;
    oracle/poa_oracle.c says per bin what is counted): rounds and why the last
    one is final, window growths, the accepted candidate's depth
    (ncols - 10) - i, the rule that rejected or accepted each candidate window,
    the cursor advance and the emitted columns of each round."""
    assert lib().opoa_shred_bins() == len(SHRED_BINS)
    return dict(zip(SHRED_BINS, (int(x) for x in _counter("opoa_shred_hist", len(SHRED_BINS), reset))))


class counting:
    """Context manager: zero every debug counter and count until the exit."""

    def __enter__(self):
        reset_counters()
        lib().opoa_set_counting(1)
        return self

    def __exit__(self, *exc):
        lib().opoa_set_counting(0)
        return False


def reset_counters() -> None:
    """Zero every debug counter."""
    _counter("opoa_row_kinds", 8, True)
    _counter("opoa_tb_moves", 12, True)
    tb_hist(True), band_hist(True), tb_events(True), tie_hist(True), shred_hist(True)


class OprepAln(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("qb", "qe", "tb", "te", "score", "mat", "mis", "ins", "del_", "aln")]


class Prepared:
    """One ZMW after the oracle's ccs_prepare + strand flip (the same fields as
    ccsx_amd.Prepared: segments are slices of seqs)."""

    def __init__(self, seqs: bytes, offs, lens):
        self.seqs, self.offs, self.lens = seqs, offs, lens


def _p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def prepare_segments(subreads: list[bytes]):
    """The oracle's ccs_prepare (main.c:344-453): (offs, lens, reverse flags)
    of the push list into the concatenated subreads, template first."""
    seqs = b"".join(subreads)
    lens = np.ascontiguousarray([len(s) for s in subreads], dtype=np.uint32)
    n = len(subreads)
    so = np.zeros(max(n, 1), np.uint32)
    sl = np.zeros(max(n, 1), np.uint32)
    rv = np.zeros(max(n, 1), np.uint8)
    ns = lib().oprep_prepare(seqs, _p32(lens), n, _p32(so), _p32(sl), rv.ctypes.data_as(C.POINTER(C.c_uint8)))
    return so[:ns].copy(), sl[:ns].copy(), rv[:ns].copy()


def prepare(subreads: list[bytes]) -> Prepared:
    """The oracle's ccs_prepare + in-place reverse complement of the reverse
    segments (seqio.h:138-148): what the POA is pushed."""
    seqs = b"".join(subreads)
    buf = C.create_string_buffer(seqs, len(seqs) + 1)
    lens = np.ascontiguousarray([len(s) for s in subreads], dtype=np.uint32)
    n = len(subreads)
    so = np.zeros(max(n, 1), np.uint32)
    sl = np.zeros(max(n, 1), np.uint32)
    ns = lib().oprep_prepare_apply(buf, _p32(lens), n, _p32(so), _p32(sl))
    return Prepared(buf.raw[:len(seqs)], so[:ns].copy(), sl[:ns].copy())


def pairwise(q: bytes, t: bytes) -> dict:
    """SPEC.md §8's aligner as the oracle restates it (2-bit codes in q, t)."""
    r = lib().oprep_pairwise(q, len(q), t, len(t))
    return {n if n != "del_" else "del": getattr(r, n) for n, _ in OprepAln._fields_}


def edit_identity(a: bytes, b: bytes, band: int = 1024) -> float:
    """1 - (banded) edit distance / max length: a lower bound of the identity
    (accuracy sanity check vs synthetic truth; not parity)."""
    if not a or not b:
        return 0.0
    d = lib().ocsx_edit_distance(a, len(a), b, len(b), band)
    return 0.0 if d < 0 else 1.0 - d / max(len(a), len(b))


class Poa:
    """The oracle's bspoa-like object (SPEC.md) with main.c's parameters."""

    def __init__(self, M=2, X=-6, O=-3, E=-2, W=128):
        self._L = lib()
        self._g = self._L.opoa_init(M, X, O, E, W)

    def __del__(self):
        try:
            self._L.opoa_free(self._g)
        except Exception:
            pass

    def poa(self, reads: list[bytes]):
        """beg + push* + end + tidy: returns (cns codes, msa [ncols, nseq+4] uint8)."""
        L = self._L
        L.opoa_beg(self._g)
        for r in reads:
            L.opoa_push(self._g, r, len(r))
        L.opoa_end(self._g)
        L.opoa_tidy_msa(self._g)
        p = C.c_void_p()
        n = L.opoa_cns(self._g, C.byref(p))
        cns = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n,)).copy() if n else np.zeros(0, np.uint8)
        ip, cp, mrow = C.c_void_p(), C.c_void_p(), C.c_uint32()
        nc = L.opoa_msa(self._g, C.byref(ip), C.byref(cp), C.byref(mrow))
        if nc:
            msa = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint8)), (nc * mrow.value,)).copy()
            msa = msa.reshape(nc, mrow.value)
        else:
            msa = np.zeros((0, len(reads) + 4), np.uint8)
        return cns, msa

    def zmw(self, seqs: bytes, offs, lens, mode: int = 0) -> bytes:
        """ccs_for2 (mode 0) / ccs_for (mode 1) on strand-normalised segments."""
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        out = C.create_string_buffer(int(lens.sum()) + 16)
        n = self._L.ocsx_zmw(self._g, mode, seqs, offs.ctypes.data_as(C.POINTER(C.c_uint32)),
                             lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(lens), out)
        return out.raw[:n]

    def zmw_breakpoints(self, seqs: bytes, offs, lens) -> tuple[bytes, list[tuple[int, int]]]:
        """ccs_for2 plus, per shredding round, (breakpoint, MSA columns): the
        values main.c:619-620 prints at -v >= 3."""
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        out = C.create_string_buffer(int(lens.sum()) + 16)
        cap = int(lens.sum()) + 2
        log = (C.c_uint32 * (2 * cap))()
        nbp = C.c_uint32(0)
        n = self._L.ocsx_zmw_log(self._g, 0, seqs, offs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 lens.ctypes.data_as(C.POINTER(C.c_uint32)), len(lens), out, log, cap, C.byref(nbp))
        return out.raw[:n], [(log[2 * i], log[2 * i + 1]) for i in range(nbp.value)]

    def cells(self) -> int:
        return int(self._L.opoa_cells(self._g))

    def nrows(self) -> int:
        return int(self._L.opoa_nrows(self._g))

    def max_indegree(self) -> int:
        """Largest predecessor count of the current graph (after poa())."""
        h = (C.c_uint64 * 8)()
        self._L.opoa_graph_stats(self._g, h)
        return int(h[2])


def batch(zmws, mode: int = 0, nthreads: int = 1):
    """Run ocsx_zmw over prepared ZMWs on nthreads pthreads.

    zmws: objects with .seqs (bytes), .offs, .lens.  Returns (list of CCS bytes,
    list of cells, wall seconds)."""
    import time
    L = lib()
    n = len(zmws)
    keep = []
    seqs = (C.c_char_p * n)()
    offs = (C.POINTER(C.c_uint32) * n)()
    lens = (C.POINTER(C.c_uint32) * n)()
    nseg = (C.c_uint32 * n)()
    outs = (C.c_char_p * n)()
    bufs = []
    for i, z in enumerate(zmws):
        o = np.ascontiguousarray(z.offs, dtype=np.uint32)
        ln = np.ascontiguousarray(z.lens, dtype=np.uint32)
        keep += [o, ln, z.seqs]
        seqs[i] = z.seqs
        offs[i] = o.ctypes.data_as(C.POINTER(C.c_uint32))
        lens[i] = ln.ctypes.data_as(C.POINTER(C.c_uint32))
        nseg[i] = len(ln)
        b = C.create_string_buffer(int(ln.sum()) + 16)
        bufs.append(b)
        outs[i] = C.cast(b, C.c_char_p)
    olen = (C.c_size_t * n)()
    cells = (C.c_uint64 * n)()
    t = time.perf_counter()
    L.ocsx_batch(mode, nthreads, n, seqs, offs, lens, nseg, outs, olen, cells)
    dt = time.perf_counter() - t
    return [bufs[i].raw[:olen[i]] for i in range(n)], [int(cells[i]) for i in range(n)], dt
