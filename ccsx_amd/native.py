"""ctypes bindings of libccsx_amd.so (include/ccsx_gpu.h, ccsx_host.h, ccsx_seqio.h).

The GPU engine has no CPU fallback: if the library is missing, or no GPU is
present, every call that needs it raises.  Host-side helpers (ccs_prepare,
reverse complement, the synthetic ZMW source, the subread reader) run on the
CPU and work without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("CCSX_LIB", "libccsx_amd.so"))

MODE_SHRED = 0
MODE_PRIMITIVE = 1

# every symbol the public headers declare (checked by tests/test_abi.py)
EXPORTS = {
    "ccsx_gpu.h": ["ccsx_gpu_device_count", "ccsx_gpu_open", "ccsx_gpu_close", "ccsx_gpu_error", "ccsx_gpu_status_str", "ccsx_gpu_run",
                   "ccsx_gpu_stage", "ccsx_gpu_launch", "ccsx_gpu_fetch", "ccsx_gpu_staged_bytes",
                   "ccsx_gpu_set_profiling", "ccsx_gpu_profile", "ccsx_gpu_profile_zmw", "ccsx_gpu_set_tight_rows", "ccsx_gpu_set_tight_out", "ccsx_gpu_set_tight_far", "ccsx_gpu_set_stage_piece",
                   "ccsx_gpu_set_mem_share", "ccsx_gpu_set_prealloc", "ccsx_gpu_set_fault",
                   "ccsx_gpu_set_kernel_cfg", "ccsx_gpu_kernel_cfg", "ccsx_gpu_rerun_count", "ccsx_gpu_hbm_launches",
                   "ccsx_gpu_set_bp_log", "ccsx_gpu_bp_log", "ccsx_gpu_stage_for",
                   "ccsx_gpu_run_stats", "ccsx_gpu_zmw_bytes", "ccsx_gpu_set_slot_budget", "ccsx_gpu_set_wg_cap",
                   "ccsx_gpu_set_shred_read_cap", "ccsx_gpu_set_mem_frac", "ccsx_gpu_set_mem_wait",
                   "ccsx_gpu_slot_bytes", "ccsx_gpu_submit", "ccsx_gpu_collect", "ccsx_gpu_reserve_staging",
                   "ccsx_gpu_set_quality", "ccsx_gpu_quality", "ccsx_gpu_set_pass_stats", "ccsx_gpu_pass_stats",
                   "ccsx_gpu_set_base_map", "ccsx_gpu_base_map", "ccsx_gpu_set_pileup", "ccsx_gpu_pileup",
                   "ccsx_gpu_set_kinetics", "ccsx_gpu_kinetics", "ccsx_gpu_set_by_strand", "ccsx_gpu_by_strand",
                   "ccsx_gpu_aln_open", "ccsx_gpu_aln_close", "ccsx_gpu_aln_error", "ccsx_gpu_band_align",
                   "ccsx_gpu_aln_stats",
                   "ccsx_gpu_polish_open", "ccsx_gpu_polish_close", "ccsx_gpu_polish_error", "ccsx_gpu_polish",
                   "ccsx_gpu_polish_stats",
                   "ccsx_gpu_bc_open", "ccsx_gpu_bc_close", "ccsx_gpu_bc_error", "ccsx_gpu_bc_set", "ccsx_gpu_bc_score",
                   "ccsx_gpu_bc_stats",
                   "ccsx_gpu_scan_open", "ccsx_gpu_scan_close", "ccsx_gpu_scan_error", "ccsx_gpu_scan_set", "ccsx_gpu_scan",
                   "ccsx_gpu_scan_tracks", "ccsx_gpu_scan_tile", "ccsx_gpu_scan_stats",
                   "ccsx_gpu_ref_open", "ccsx_gpu_ref_close", "ccsx_gpu_ref_error", "ccsx_gpu_ref_set", "ccsx_gpu_ref_map",
                   "ccsx_gpu_ref_vote_cap", "ccsx_gpu_ref_stats"],
    "ccsx_bspoa.h": ["init_bspoa", "beg_bspoa", "push_bspoa", "end_bspoa", "tidy_msa_bspoa", "free_bspoa"],
    "ccsx_host.h": ["ccsx_revcomp", "ccsx_prepare", "ccsx_prepare_apply", "ccsx_pairwise", "ccsx_synth_zmw",
                    "ccsx_zmw_cost", "ccsx_partition", "ccsx_qual_phred", "ccsx_qual_rq", "ccsx_pass_identity",
                    "ccsx_map_cigar", "ccsx_pileup_call", "ccsx_polish_host",
                    "ccsx_barcode_check", "ccsx_barcode_host", "ccsx_barcode_call", "ccsx_barcode_read",
                    "ccsx_barcode_set_get", "ccsx_barcode_set_free",
                    "ccsx_scan_check", "ccsx_scan_host", "ccsx_scan_start", "ccsx_scan_cut",
                    "ccsx_pairwise_band_path", "ccsx_ref_set_make", "ccsx_ref_set_free", "ccsx_ref_host", "ccsx_ref_pass",
                    "ccsx_prepare_apply_kin", "ccsx_kin_frames", "ccsx_kin_code", "ccsx_kinetics_tags",
                    "ccsx_synth_batch_kinetics",
                    "ccsx_pairwise_seed", "ccsx_pairwise_band", "ccsx_prep_begin", "ccsx_prep_pending",
                    "ccsx_prep_answer", "ccsx_prep_unused", "ccsx_prep_end", "ccsx_prepare_batch",
                    "ccsx_synth_batch_make", "ccsx_synth_batch_zmws", "ccsx_synth_batch_free"],
    "ccsx_seqio.h": ["ccsx_reader_open", "ccsx_reader_next", "ccsx_reader_next_kin", "ccsx_reader_close"],
}


class ZmwIn(C.Structure):
    _fields_ = [("seqs", C.c_char_p), ("seg_off", C.POINTER(C.c_uint32)), ("seg_len", C.POINTER(C.c_uint32)),
                ("nseg", C.c_uint32), ("seg_rev", C.POINTER(C.c_uint8)),
                ("ipd", C.POINTER(C.c_uint8)), ("pw", C.POINTER(C.c_uint8))]


class ZmwOut(C.Structure):
    _fields_ = [("ccs", C.c_void_p), ("len", C.c_uint32), ("status", C.c_int32), ("cells", C.c_uint64)]


class PairAln(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("qb", "qe", "tb", "te", "mat", "mis", "ins", "del_", "aln", "score")]


class Pair(C.Structure):
    _fields_ = [("q", C.c_void_p), ("qlen", C.c_uint32), ("t", C.c_void_p), ("tlen", C.c_uint32)]


class BandJob(C.Structure):
    _fields_ = [("q", C.c_char_p), ("t", C.c_char_p), ("qlen", C.c_uint32), ("tlen", C.c_uint32), ("d0", C.c_int32)]


class PolishIn(C.Structure):
    _fields_ = [("ccs", C.c_char_p), ("len", C.c_uint32), ("seqs", C.c_char_p), ("seg_off", C.POINTER(C.c_uint32)),
                ("seg_len", C.POINTER(C.c_uint32)), ("nseg", C.c_uint32), ("map", C.POINTER(C.c_uint32))]


class PolishOut(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("len", C.c_uint32), ("nsub", C.c_uint32),
                ("nins", C.c_uint32), ("ndel", C.c_uint32), ("map", C.POINTER(C.c_uint32)), ("status", C.c_int32)]


class BcIn(C.Structure):
    _fields_ = [("ccs", C.c_char_p), ("len", C.c_uint32)]


class BcOut(C.Structure):
    # e[2] x (pattern, score, end, second, second_pattern)
    _fields_ = [("v", C.c_int32 * 10)]


class BcCall(C.Structure):
    _fields_ = [("cl", C.c_uint32), ("cr", C.c_uint32), ("called", C.c_uint8 * 2), ("assigned", C.c_uint8),
                ("reason", C.c_uint8)]


class ScanHit(C.Structure):
    _fields_ = [("read", C.c_uint32), ("adapter", C.c_uint32), ("orient", C.c_uint32), ("start", C.c_uint32),
                ("end", C.c_uint32), ("score", C.c_int32)]


class RefRec(C.Structure):
    # g, o, d0, votes, votes2, then the ten fields of ccsx_pairaln
    _fields_ = [("v", C.c_int32 * 15)]


class ScanPiece(C.Structure):
    _fields_ = [("b", C.c_uint32), ("e", C.c_uint32), ("left", C.c_int32), ("right", C.c_int32)]


class BatchInfo(C.Structure):
    _fields_ = [("rounds", C.c_uint64), ("jobs", C.c_uint64), ("seed_ms", C.c_double), ("device_ms", C.c_double),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.ccsx_gpu_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.ccsx_gpu_close.argtypes = [C.c_void_p]
        L.ccsx_gpu_error.argtypes = [C.c_void_p]
        L.ccsx_gpu_error.restype = C.c_char_p
        L.ccsx_gpu_status_str.argtypes = [C.c_int32]
        L.ccsx_gpu_status_str.restype = C.c_char_p
        L.ccsx_gpu_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(ZmwIn), C.c_size_t, C.POINTER(ZmwOut)]
        L.ccsx_gpu_stage.argtypes = [C.c_void_p, C.POINTER(ZmwIn), C.c_size_t]
        L.ccsx_gpu_stage_for.argtypes = [C.c_void_p, C.c_int, C.POINTER(ZmwIn), C.c_size_t]
        L.ccsx_gpu_launch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.ccsx_gpu_fetch.argtypes = [C.c_void_p, C.POINTER(ZmwOut)]
        L.ccsx_gpu_staged_bytes.argtypes = [C.c_void_p]
        L.ccsx_gpu_staged_bytes.restype = C.c_uint64
        L.ccsx_gpu_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.ccsx_gpu_profile.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        if hasattr(L, "ccsx_gpu_profile_zmw"):  # diagnostics; absent from older builds used in A/B runs
            L.ccsx_gpu_profile_zmw.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32]
        L.ccsx_gpu_set_tight_rows.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_set_tight_out.argtypes = [C.c_void_p, C.c_uint32]
        if hasattr(L, "ccsx_gpu_set_tight_far"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_tight_far.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_set_stage_piece.argtypes = [C.c_void_p, C.c_uint64]
        L.ccsx_gpu_set_prealloc.argtypes = [C.c_void_p, C.c_int]
        L.ccsx_gpu_set_kernel_cfg.argtypes = [C.c_void_p, C.c_int]
        L.ccsx_gpu_kernel_cfg.argtypes = [C.c_void_p]
        L.ccsx_gpu_rerun_count.argtypes = [C.c_void_p]
        L.ccsx_gpu_rerun_count.restype = C.c_int64
        L.ccsx_gpu_hbm_launches.argtypes = [C.c_void_p]
        L.ccsx_gpu_hbm_launches.restype = C.c_int64
        L.ccsx_gpu_run_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        L.ccsx_gpu_zmw_bytes.argtypes = [C.c_void_p, C.c_int, C.POINTER(ZmwIn)]
        L.ccsx_gpu_zmw_bytes.restype = C.c_uint64
        L.ccsx_gpu_set_slot_budget.argtypes = [C.c_void_p, C.c_uint64]
        L.ccsx_gpu_set_wg_cap.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_set_shred_read_cap.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_set_mem_share.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_set_mem_frac.argtypes = [C.c_void_p, C.c_float]
        if hasattr(L, "ccsx_gpu_set_mem_wait"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_mem_wait.argtypes = [C.c_void_p, C.c_uint32]
        L.ccsx_gpu_slot_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.ccsx_gpu_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(ZmwIn), C.c_size_t, C.POINTER(C.c_int)]
        L.ccsx_gpu_collect.argtypes = [C.c_void_p, C.c_int, C.POINTER(ZmwOut)]
        L.ccsx_gpu_set_fault.argtypes = [C.c_void_p, C.c_int64]
        L.ccsx_gpu_set_bp_log.argtypes = [C.c_void_p, C.c_int]
        L.ccsx_gpu_bp_log.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint32)),
                                      C.POINTER(C.c_uint32)]
        if hasattr(L, "ccsx_gpu_set_quality"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_quality.argtypes = [C.c_void_p, C.c_int]
            L.ccsx_gpu_quality.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_uint32)]
            L.ccsx_qual_phred.argtypes = [C.c_uint32, C.c_uint32]
            L.ccsx_qual_phred.restype = C.c_uint8
            L.ccsx_qual_rq.argtypes = [C.c_void_p, C.c_uint32]
            L.ccsx_qual_rq.restype = C.c_double
        if hasattr(L, "ccsx_gpu_set_pass_stats"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_pass_stats.argtypes = [C.c_void_p, C.c_int]
            L.ccsx_gpu_pass_stats.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_uint32)]
            L.ccsx_pass_identity.argtypes = [C.c_void_p]
            L.ccsx_pass_identity.restype = C.c_double
        if hasattr(L, "ccsx_gpu_set_base_map"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_base_map.argtypes = [C.c_void_p, C.c_int]
            L.ccsx_gpu_base_map.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_uint32,
                                            C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
            L.ccsx_map_cigar.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
            L.ccsx_map_cigar.restype = C.c_long
        L.ccsx_gpu_set_pileup.argtypes = [C.c_void_p, C.c_int]
        L.ccsx_gpu_pileup.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.ccsx_pileup_call.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "ccsx_gpu_set_by_strand"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_by_strand.argtypes = [C.c_void_p, C.c_int]
            L.ccsx_gpu_by_strand.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        if hasattr(L, "ccsx_gpu_set_kinetics"):  # (absent from the older builds used in A/B runs)
            L.ccsx_gpu_set_kinetics.argtypes = [C.c_void_p, C.c_int]
            L.ccsx_gpu_kinetics.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
            L.ccsx_kin_frames.argtypes = [C.c_uint8]
            L.ccsx_kin_frames.restype = C.c_uint32
            L.ccsx_kin_code.argtypes = [C.c_uint32]
            L.ccsx_kin_code.restype = C.c_uint8
            L.ccsx_kinetics_tags.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
            L.ccsx_kinetics_tags.restype = C.c_long
            L.ccsx_prepare_apply_kin.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32,
                                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
            L.ccsx_prepare_apply_kin.restype = C.c_uint32
            L.ccsx_synth_batch_kinetics.argtypes = [C.c_void_p, C.c_uint64]
            L.ccsx_reader_next_kin.argtypes = [C.c_void_p] + [C.POINTER(C.c_char_p)] * 2 + [
                C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.ccsx_revcomp.argtypes = [C.c_char_p, C.c_uint32]
        L.ccsx_prepare.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
        L.ccsx_prepare.restype = C.c_uint32
        L.ccsx_prepare_apply.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]
        L.ccsx_prepare_apply.restype = C.c_uint32
        L.ccsx_pairwise.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
        L.ccsx_pairwise.restype = PairAln
        if hasattr(L, "ccsx_gpu_band_align"):  # (absent from the older builds used in A/B runs)
            L.ccsx_pairwise_seed.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_int32)]
            L.ccsx_pairwise_band.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int32]
            L.ccsx_pairwise_band.restype = PairAln
            L.ccsx_prep_begin.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
            L.ccsx_prep_begin.restype = C.c_void_p
            L.ccsx_prep_pending.argtypes = [C.c_void_p, C.POINTER(Pair)]
            L.ccsx_prep_pending.restype = C.c_uint32
            L.ccsx_prep_answer.argtypes = [C.c_void_p, C.POINTER(PairAln)]
            L.ccsx_prep_answer.restype = None
            L.ccsx_prep_unused.argtypes = [C.c_void_p]
            L.ccsx_prep_unused.restype = C.c_uint32
            L.ccsx_prep_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
            L.ccsx_prep_end.restype = C.c_uint32
            L.ccsx_gpu_aln_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
            L.ccsx_gpu_aln_close.argtypes = [C.c_void_p]
            L.ccsx_gpu_aln_close.restype = None
            L.ccsx_gpu_aln_error.argtypes = [C.c_void_p]
            L.ccsx_gpu_aln_error.restype = C.c_char_p
            L.ccsx_gpu_band_align.argtypes = [C.c_void_p, C.POINTER(BandJob), C.c_size_t, C.POINTER(PairAln),
                                              C.POINTER(C.c_float)]
            L.ccsx_gpu_aln_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
            L.ccsx_prepare_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_uint32)),
                                             C.POINTER(C.c_uint32), C.c_size_t, C.c_int,
                                             C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)),
                                             C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32),
                                             C.POINTER(BatchInfo)]
        if hasattr(L, "ccsx_gpu_polish"):  # (absent from the older builds used in A/B runs)
            L.ccsx_polish_host.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p,
                                           C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            L.ccsx_polish_host.restype = C.c_int32
            L.ccsx_gpu_polish_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
            L.ccsx_gpu_polish_close.argtypes = [C.c_void_p]
            L.ccsx_gpu_polish_close.restype = None
            L.ccsx_gpu_polish_error.argtypes = [C.c_void_p]
            L.ccsx_gpu_polish_error.restype = C.c_char_p
            L.ccsx_gpu_polish.argtypes = [C.c_void_p, C.POINTER(PolishIn), C.c_size_t, C.POINTER(PolishOut),
                                          C.POINTER(C.c_float)]
            L.ccsx_gpu_polish_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        if hasattr(L, "ccsx_gpu_bc_score"):  # (absent from the older builds used in A/B runs)
            bset = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
            L.ccsx_barcode_check.argtypes = bset
            L.ccsx_barcode_check.restype = C.c_int32
            L.ccsx_barcode_host.argtypes = bset + [C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(BcOut)]
            L.ccsx_barcode_host.restype = C.c_int32
            L.ccsx_barcode_call.argtypes = [C.POINTER(BcOut), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int32,
                                            C.c_int32, C.POINTER(BcCall)]
            L.ccsx_barcode_call.restype = None
            L.ccsx_barcode_read.argtypes = [C.c_char_p]
            L.ccsx_barcode_read.restype = C.c_void_p
            L.ccsx_barcode_set_get.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_char_p))]
            L.ccsx_barcode_set_get.restype = C.c_uint32
            L.ccsx_barcode_set_free.argtypes = [C.c_void_p]
            L.ccsx_barcode_set_free.restype = None
            L.ccsx_gpu_bc_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
            L.ccsx_gpu_bc_close.argtypes = [C.c_void_p]
            L.ccsx_gpu_bc_close.restype = None
            L.ccsx_gpu_bc_error.argtypes = [C.c_void_p]
            L.ccsx_gpu_bc_error.restype = C.c_char_p
            L.ccsx_gpu_bc_set.argtypes = [C.c_void_p] + bset + [C.c_uint32]
            L.ccsx_gpu_bc_score.argtypes = [C.c_void_p, C.POINTER(BcIn), C.c_size_t, C.POINTER(BcOut), C.POINTER(C.c_float)]
            L.ccsx_gpu_bc_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        if hasattr(L, "ccsx_gpu_scan"):  # (absent from the older builds used in A/B runs)
            aset = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
            L.ccsx_scan_check.argtypes = aset
            L.ccsx_scan_check.restype = C.c_int32
            L.ccsx_scan_host.argtypes = aset + [C.c_char_p, C.c_uint32, C.POINTER(ScanHit), C.c_uint64]
            L.ccsx_scan_host.restype = C.c_int64
            L.ccsx_scan_start.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_int32)]
            L.ccsx_scan_start.restype = C.c_int32
            L.ccsx_scan_cut.argtypes = [C.POINTER(ScanHit), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(ScanPiece), C.c_uint64]
            L.ccsx_scan_cut.restype = C.c_int64
            L.ccsx_gpu_scan_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
            L.ccsx_gpu_scan_close.argtypes = [C.c_void_p]
            L.ccsx_gpu_scan_close.restype = None
            L.ccsx_gpu_scan_error.argtypes = [C.c_void_p]
            L.ccsx_gpu_scan_error.restype = C.c_char_p
            L.ccsx_gpu_scan_set.argtypes = [C.c_void_p] + aset
            L.ccsx_gpu_scan.argtypes = [C.c_void_p, C.POINTER(BcIn), C.c_size_t, C.POINTER(C.POINTER(ScanHit)),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
            L.ccsx_gpu_scan_tracks.argtypes = [C.c_void_p, C.POINTER(BcIn), C.c_size_t, C.c_void_p, C.c_uint64]
            L.ccsx_gpu_scan_tile.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            L.ccsx_gpu_scan_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        if hasattr(L, "ccsx_gpu_ref_map"):  # (absent from the older builds used in A/B runs)
            L.ccsx_ref_set_make.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
            L.ccsx_ref_set_make.restype = C.c_void_p
            L.ccsx_ref_set_free.argtypes = [C.c_void_p]
            L.ccsx_ref_set_free.restype = None
            L.ccsx_ref_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(RefRec), C.c_void_p]
            L.ccsx_ref_host.restype = C.c_int32
            L.ccsx_ref_pass.argtypes = [C.POINTER(RefRec), C.c_int32, C.c_int32]
            L.ccsx_ref_pass.restype = C.c_int32
            L.ccsx_gpu_ref_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
            L.ccsx_gpu_ref_close.argtypes = [C.c_void_p]
            L.ccsx_gpu_ref_close.restype = None
            L.ccsx_gpu_ref_error.argtypes = [C.c_void_p]
            L.ccsx_gpu_ref_error.restype = C.c_char_p
            L.ccsx_gpu_ref_set.argtypes = [C.c_void_p, C.c_void_p]
            L.ccsx_gpu_ref_map.argtypes = [C.c_void_p, C.POINTER(BcIn), C.c_size_t, C.POINTER(RefRec), C.c_void_p,
                                           C.POINTER(C.c_float)]
            L.ccsx_gpu_ref_vote_cap.argtypes = [C.c_void_p, C.c_uint32]
            L.ccsx_gpu_ref_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
        L.ccsx_synth_zmw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p,
                                     C.POINTER(C.c_uint32), C.c_char_p]
        L.ccsx_synth_zmw.restype = C.c_uint64
        L.ccsx_zmw_cost.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
        L.ccsx_zmw_cost.restype = C.c_uint64
        L.ccsx_partition.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.ccsx_partition.restype = C.c_uint32
        L.ccsx_synth_batch_make.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint32), C.c_uint32, C.c_int]
        L.ccsx_synth_batch_make.restype = C.c_void_p
        L.ccsx_synth_batch_zmws.argtypes = [C.c_void_p]
        L.ccsx_synth_batch_zmws.restype = C.POINTER(ZmwIn)
        L.ccsx_synth_batch_free.argtypes = [C.c_void_p]
        L.ccsx_reader_open.argtypes = [C.c_char_p, C.c_int]
        L.ccsx_reader_open.restype = C.c_void_p
        L.ccsx_reader_next.argtypes = [C.c_void_p] + [C.POINTER(C.c_char_p)] * 2 + [C.POINTER(C.c_void_p),
                                                                                     C.POINTER(C.POINTER(C.c_uint32))]
        L.ccsx_reader_close.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def _p32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


# ---------------------------------------------------------------- host helpers
def revcomp(seq: bytes) -> bytes:
    b = C.create_string_buffer(bytes(seq), len(seq))
    lib().ccsx_revcomp(b, len(seq))
    return b.raw[:len(seq)]


def synth_zmw(seed: int, hole: int, L: int, passes: int):
    """Synthetic ZMW: returns (list of subread bytes, true insert bytes)."""
    cap = passes * (2 * L + 16) + 16
    out = C.create_string_buffer(cap)
    lens = np.zeros(passes, dtype=np.uint32)
    ins = C.create_string_buffer(L + 1)
    lib().ccsx_synth_zmw(seed, hole, L, passes, out, _p32(lens), ins)
    raw = out.raw
    subs, o = [], 0
    for n in lens:
        subs.append(raw[o:o + int(n)])
        o += int(n)
    return subs, ins.raw[:L]


@dataclass
class Prepared:
    """One ZMW after ccs_prepare + strand flip: segments are slices of seqs;
    rev = ccs_prepare's strand flag per segment (None: all forward), read by the
    engine only with the strand pileup, the kinetics or the by-strand output on; ipd / pw = one 8-bit
    kinetics code per byte of seqs in the orientation the segments are pushed in
    (SPEC.md §13; None: the ZMW has none), read only with the kinetics on."""
    seqs: bytes
    offs: np.ndarray
    lens: np.ndarray
    rev: np.ndarray | None = None
    ipd: bytes | None = None
    pw: bytes | None = None


def prepare(subreads: list[bytes], ipd=None, pw=None) -> Prepared:
    """ccs_prepare (main.c:344-453) + in-place reverse complement of reverse
    segments; with ipd and pw (one bytes of codes per subread, parallel to its
    bases) also their reversal over each reverse segment (ccsx_prepare_apply_kin)."""
    if ipd is not None or pw is not None:
        if ipd is None or pw is None or [len(x) for x in ipd] != [len(s) for s in subreads] or \
                [len(x) for x in pw] != [len(s) for s in subreads]:
            raise ValueError("ipd and pw need one code per base of every subread")
        seqs = b"".join(subreads)
        buf = C.create_string_buffer(seqs, len(seqs) + 1)
        bi = C.create_string_buffer(b"".join(bytes(x) for x in ipd), len(seqs) + 1)
        bp = C.create_string_buffer(b"".join(bytes(x) for x in pw), len(seqs) + 1)
        lens = _u32([len(s) for s in subreads])
        n = len(subreads)
        so, sl = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        rv = np.zeros(max(n, 1), dtype=np.uint8)
        ns = lib().ccsx_prepare_apply_kin(buf, bi, bp, _p32(lens), n, _p32(so), _p32(sl),
                                          rv.ctypes.data_as(C.POINTER(C.c_uint8)))
        return Prepared(buf.raw[:len(seqs)], so[:ns].copy(), sl[:ns].copy(), rv[:ns].copy(),
                        bi.raw[:len(seqs)], bp.raw[:len(seqs)])
    seqs = b"".join(subreads)
    buf = C.create_string_buffer(seqs, len(seqs) + 1)
    lens = _u32([len(s) for s in subreads])
    n = len(subreads)
    so = np.zeros(max(n, 1), dtype=np.uint32)
    sl = np.zeros(max(n, 1), dtype=np.uint32)
    rv = np.zeros(max(n, 1), dtype=np.uint8)
    # (ccsx_prepare_apply, keeping the flags)
    L = lib()
    ns = L.ccsx_prepare(buf, _p32(lens), n, _p32(so), _p32(sl), rv.ctypes.data_as(C.POINTER(C.c_uint8)))
    out = bytearray(buf.raw[:len(seqs)])
    for k in range(ns):
        if rv[k]:
            o, ln = int(so[k]), int(sl[k])
            out[o:o + ln] = revcomp(bytes(out[o:o + ln]))
    return Prepared(bytes(out), so[:ns].copy(), sl[:ns].copy(), rv[:ns].copy())


def prepare_segments(subreads: list[bytes]):
    """ccs_prepare only: (offs, lens, reverse flags) into the concatenated subreads."""
    seqs = b"".join(subreads)
    lens = _u32([len(s) for s in subreads])
    n = len(subreads)
    so = np.zeros(max(n, 1), dtype=np.uint32)
    sl = np.zeros(max(n, 1), dtype=np.uint32)
    rv = np.zeros(max(n, 1), dtype=np.uint8)
    ns = lib().ccsx_prepare(seqs, _p32(lens), n, _p32(so), _p32(sl), rv.ctypes.data_as(C.POINTER(C.c_uint8)))
    return so[:ns].copy(), sl[:ns].copy(), rv[:ns].copy()


def zmw_cost(seg_len) -> int:
    """ccsx_zmw_cost: estimated POA work of a prepared ZMW (host/dispatch.cpp)."""
    a = _u32(seg_len)
    return int(lib().ccsx_zmw_cost(_p32(a), len(a)))


def partition(costs, nparts: int, min_batch: int):
    """ccsx_partition: (LPT order, list of batches as index lists into the input)."""
    c = np.ascontiguousarray(np.asarray(costs, dtype=np.uint64))
    n = len(c)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    bounds = np.zeros(n + 1, dtype=np.uint32)
    nb = lib().ccsx_partition(c.ctypes.data_as(C.POINTER(C.c_uint64)), n, nparts, min_batch, _p32(order), _p32(bounds))
    return order[:n].tolist(), [order[bounds[b]:bounds[b + 1]].tolist() for b in range(nb)]


def pairwise(q: bytes, t: bytes) -> dict:
    r = lib().ccsx_pairwise(q, len(q), t, len(t))
    return {n if n != "del_" else "del": getattr(r, n) for n, _ in PairAln._fields_}


def _aln_dict(r) -> dict:
    return {n if n != "del_" else "del": getattr(r, n) for n, _ in PairAln._fields_}


def pairwise_seed(q: bytes, t: bytes):
    """ccsx_pairwise_seed: the 13-mer diagonal vote of SPEC.md §8; the winning
    diagonal d0, or None when either is shorter than 13 or nothing votes."""
    d0 = C.c_int32(0)
    return int(d0.value) if lib().ccsx_pairwise_seed(q, len(q), t, len(t), C.byref(d0)) else None


def pairwise_band(q: bytes, t: bytes, d0: int) -> dict:
    """ccsx_pairwise_band: the banded local alignment around diagonal d0 and
    its traceback (SPEC.md §8 steps 2-3), on the host."""
    return _aln_dict(lib().ccsx_pairwise_band(q, len(q), t, len(t), d0))


class Prep:
    """The resumable ccs_prepare of one ZMW (ccsx_prep_*): pending() gives the
    open request as [(q, t), (q, t)] of 2-bit code bytes or None when the walk
    has finished, answer() takes the two alignments (dicts as pairwise()
    returns), end() returns the push list (offs, lens, reverse flags)."""

    def __init__(self, subreads: list[bytes]):
        self._L = lib()
        self._seqs = C.create_string_buffer(b"".join(subreads), sum(len(s) for s in subreads) + 1)
        self._lens = _u32([len(s) for s in subreads])
        self._n = len(subreads)
        self._p = self._L.ccsx_prep_begin(self._seqs, _p32(self._lens), self._n)

    def pending(self):
        w = (Pair * 2)()
        if not self._L.ccsx_prep_pending(self._p, w):
            return None
        return [(C.string_at(x.q, x.qlen), C.string_at(x.t, x.tlen)) for x in w]

    def answer(self, res) -> None:
        r = (PairAln * 2)()
        for k in range(2):
            for n, _ in PairAln._fields_:
                setattr(r[k], n, res[k]["del" if n == "del_" else n])
        self._L.ccsx_prep_answer(self._p, r)

    def unused(self) -> int:
        return int(self._L.ccsx_prep_unused(self._p))

    def end(self):
        n = max(self._n, 1)
        so, sl, rv = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        ns = self._L.ccsx_prep_end(self._p, _p32(so), _p32(sl), rv.ctypes.data_as(C.POINTER(C.c_uint8)))
        self._p = None
        return so[:ns].copy(), sl[:ns].copy(), rv[:ns].copy()

    def __del__(self):
        try:
            if self._p:
                self._L.ccsx_prep_end(self._p, None, None, None)
        except Exception:
            pass


def qual_phred(match: int, cov: int) -> int:
    """ccsx_qual_phred: the quality of a column whose consensus base `match`
    of the `cov` reads spanning it carry (SPEC.md §9)."""
    return int(lib().ccsx_qual_phred(match, cov))


def qual_rq(qual) -> float:
    """ccsx_qual_rq: predicted accuracy 1 - mean(10^(-Q/10)) of a read's raw
    quality bytes (0.0 for none)."""
    q = np.ascontiguousarray(np.frombuffer(qual, dtype=np.uint8) if isinstance(qual, (bytes, bytearray)) else
                             np.asarray(qual, dtype=np.uint8))
    return float(lib().ccsx_qual_rq(q.ctypes.data, len(q)))


def pass_identity(rec) -> float:
    """ccsx_pass_identity: match / (match + mismatch + ins + del) of one pass
    record (match, mismatch, ins, del, cbeg, cend; SPEC.md §10), 0.0 for an
    empty one."""
    r = np.ascontiguousarray(np.asarray(rec, dtype=np.uint32).reshape(6))
    return float(lib().ccsx_pass_identity(r.ctypes.data))


def map_cigar(m):
    """ccsx_map_cigar: the alignment of one segment to the CCS derived from its
    map (Engine.base_map; SPEC.md §11): a dict with qs, qe, ts, te, n_eq, n_x,
    n_ins, n_del and cigar (=/X/I/D, in CCS order), or None for a map without
    an aligned entry."""
    a = np.ascontiguousarray(np.asarray(m, dtype=np.uint32).reshape(-1))
    aln = (C.c_uint32 * 8)()
    L = lib()
    need = L.ccsx_map_cigar(a.ctypes.data, len(a), aln, None, 0)
    if need < 0:
        return None
    buf = C.create_string_buffer(need + 1)
    if L.ccsx_map_cigar(a.ctypes.data, len(a), aln, buf, need + 1) != need:
        raise RuntimeError("ccsx_map_cigar: inconsistent length")
    d = dict(zip(("qs", "qe", "ts", "te", "n_eq", "n_x", "n_ins", "n_del"), (int(x) for x in aln)))
    d["cigar"] = buf.value.decode()
    return d


POLISH_BAD_MAP = 1


def _polish_item(ccs: bytes, segs, maps):
    """(seqs, seg_off, seg_len, map) arrays of one ZMW for ccsx_polish_in."""
    lens = _u32([len(x) for x in segs])
    offs = _u32(np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(segs) else [])
    if len(maps) != len(segs) or any(len(m) != len(x) for m, x in zip(maps, segs)):
        raise ValueError("polish: one map word per pushed base, one map per segment")
    m = _u32(np.concatenate([np.asarray(x, dtype=np.uint32) for x in maps]) if len(maps) else [])
    return b"".join(segs), offs, lens, m


def _split_map(m: np.ndarray, segs) -> list:
    out, o = [], 0
    for x in segs:
        a = m[o:o + len(x)].copy()
        a.setflags(write=False)
        out.append(a)
        o += len(x)
    return out


def polish_host(ccs: bytes, segs, maps):
    """ccsx_polish_host (SPEC.md §15): the draft ccs, its segments as pushed and
    their §11 maps -> (seq, qual, (nsub, nins, ndel), [realigned map per
    segment], status); status POLISH_BAD_MAP gives empty results."""
    seqs, offs, lens, m = _polish_item(ccs, segs, maps)
    cap = 2 * len(ccs) + 1
    oseq = C.create_string_buffer(cap)
    oqual = (C.c_uint8 * cap)()
    omap = np.zeros(max(len(m), 1), dtype=np.uint32)
    counts = (C.c_uint32 * 4)()
    st = lib().ccsx_polish_host(ccs, len(ccs), seqs, _p32(offs), _p32(lens), len(segs), _p32(m), oseq, oqual, _p32(omap),
                                counts)
    if st != 0:
        return b"", b"", (0, 0, 0), [], int(st)
    n = counts[0]
    return oseq.raw[:n], bytes(oqual[:n]), (int(counts[1]), int(counts[2]), int(counts[3])), _split_map(omap, segs), 0


def kin_frames(code: int) -> int:
    """ccsx_kin_frames: the frames an 8-bit kinetics code stands for (SPEC.md §13)."""
    return int(lib().ccsx_kin_frames(code))


def kin_code(frames: int) -> int:
    """ccsx_kin_code: the code nearest to min(frames, 952), the lower on a tie."""
    return int(lib().ccsx_kin_code(frames))


def kinetics_tags(recs) -> str:
    """ccsx_kinetics_tags: the fi / fp / ri / rp SAM array tags (tab-separated)
    of a ZMW's kinetics records (Engine.kinetics, uint8 [len, 8])."""
    r = np.ascontiguousarray(np.asarray(recs, dtype=np.uint8).reshape(-1, 8))
    L = lib()
    need = L.ccsx_kinetics_tags(r.ctypes.data, len(r), None, 0)
    buf = C.create_string_buffer(need + 1)
    if L.ccsx_kinetics_tags(r.ctypes.data, len(r), buf, need + 1) != need:
        raise RuntimeError("ccsx_kinetics_tags: inconsistent length")
    return buf.value.decode()


def pileup_call(rec, strand: int) -> int:
    """ccsx_pileup_call: the call of strand 0 (forward) / 1 (reverse) / 2 (both)
    from one 12-byte pileup record (Engine.pileup; SPEC.md §12): 0..3 a base, 4
    gap, -1 no evidence."""
    r = np.ascontiguousarray(np.asarray(rec, dtype=np.uint8).reshape(12))
    return int(lib().ccsx_pileup_call(r.ctypes.data, strand))


def read_calls(path: str, is_bam: bool = False, kinetics: bool = False):
    """Yield every ccsx_reader_next result the way main.c step 0 drives
    kseq_zmw_read (main.c:658-697): (n, movie, hole, [subreads]) for a ZMW,
    (-1, None, None, None) for each -1; after a -1 the next chunk reads on,
    and the input ends at the first chunk that yields no ZMW.  kinetics: read
    with ccsx_reader_next_kin and yield two more fields per ZMW, the ipd and pw
    codes per subread (lists of bytes), or None, None where the ZMW has none."""
    L = lib()
    r = L.ccsx_reader_open(path.encode(), 1 if is_bam else 0)
    if not r:
        raise OSError(f"cannot open {path}")
    try:
        mv, hl = C.c_char_p(), C.c_char_p()
        sq = C.c_void_p()
        ln = C.POINTER(C.c_uint32)()
        while True:
            got = 0
            while True:
                ki, kp = C.c_void_p(), C.c_void_p()
                if kinetics:
                    n = L.ccsx_reader_next_kin(r, C.byref(mv), C.byref(hl), C.byref(sq), C.byref(ln), C.byref(ki), C.byref(kp))
                else:
                    n = L.ccsx_reader_next(r, C.byref(mv), C.byref(hl), C.byref(sq), C.byref(ln))
                if n < 0:
                    yield (n, None, None, None, None, None) if kinetics else (n, None, None, None)
                    break
                got += 1
                lens = [ln[i] for i in range(n)]
                raw = C.string_at(sq, sum(lens))
                subs, o = [], 0
                for x in lens:
                    subs.append(raw[o:o + x])
                    o += x
                if kinetics:
                    planes = []
                    for p in (ki, kp):
                        if p.value:
                            rawk, o, per = C.string_at(p, sum(lens)), 0, []
                            for x in lens:
                                per.append(rawk[o:o + x])
                                o += x
                            planes.append(per)
                        else:
                            planes.append(None)
                    yield n, mv.value.decode(), hl.value.decode(), subs, planes[0], planes[1]
                    continue
                yield n, mv.value.decode(), hl.value.decode(), subs
            if not got:
                break
    finally:
        L.ccsx_reader_close(r)


def read_zmws(path: str, is_bam: bool = False, kinetics: bool = False):
    """Yield (movie, hole, [subreads]) per ZMW, as the CLI's step 0 sees them;
    with kinetics also the ipd and pw codes per subread (None, None where any
    subread of the ZMW lacks them): (movie, hole, [subreads], ipd, pw)."""
    for rec in read_calls(path, is_bam, kinetics):
        if rec[0] >= 0:
            yield rec[1:]


class SynthBatch:
    """ccsx_synth_batch_make: n synthetic ZMWs made and prepared on C threads."""

    def __init__(self, seed: int, holes, Ls, passes, nthreads: int = 16):
        n = len(holes)
        h = np.ascontiguousarray(holes, dtype=np.uint64)
        lv, pv = _u32(Ls), _u32(passes)
        self._L = lib()
        self.n = n
        self._b = self._L.ccsx_synth_batch_make(seed, h.ctypes.data_as(C.POINTER(C.c_uint64)), _p32(lv), _p32(pv), n,
                                                nthreads)
        self.zmws = self._L.ccsx_synth_batch_zmws(self._b)
        self.bases = sum(int(self.zmws[i].seg_len[k]) for i in range(n) for k in range(self.zmws[i].nseg))

    def __del__(self):
        try:
            self._L.ccsx_synth_batch_free(self._b)
        except Exception:
            pass


# ---------------------------------------------------------------- GPU engine
def device_count() -> int:
    """Visible HIP devices (0 without a GPU)."""
    return int(lib().ccsx_gpu_device_count())


class GpuError(RuntimeError):
    pass


class Aligner:
    """A band aligner context on one HIP device (ccsx_gpu_aln_*): SPEC.md §8's
    banded alignment of many pairs per launch; max_bytes = the most device
    memory its arena takes (0: the library's default)."""

    def __init__(self, device: int = 0, max_bytes: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_aln_open(device, max_bytes, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open an aligner on HIP device {device}")
        self.kernel_ms = 0.0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_aln_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_aln_error(self._ctx).decode()}")

    def band_align(self, jobs) -> list:
        """ccsx_gpu_band_align on jobs = [(q, t, d0)] (2-bit code bytes): one
        dict per job, as pairwise_band returns; kernel_ms = the kernels' time."""
        n = len(jobs)
        arr = (BandJob * max(n, 1))()
        for i, (q, t, d0) in enumerate(jobs):
            arr[i].q, arr[i].t, arr[i].qlen, arr[i].tlen, arr[i].d0 = q, t, len(q), len(t), d0
        out = (PairAln * max(n, 1))()
        ms = C.c_float(0)
        if self._L.ccsx_gpu_band_align(self._ctx, arr, n, out, C.byref(ms)) != 0:
            self._err("ccsx_gpu_band_align")
        self.kernel_ms = float(ms.value)
        return [_aln_dict(out[i]) for i in range(n)]

    def pairwise(self, pairs) -> list:
        """ccsx_pairwise of pairs = [(q, t)] with the seed on the host and the
        band on the device (a pair without a seed: the all-zero result)."""
        d0 = [pairwise_seed(q, t) for q, t in pairs]
        got = iter(self.band_align([(q, t, d) for (q, t), d in zip(pairs, d0) if d is not None]))
        zero = {n if n != "del_" else "del": 0 for n, _ in PairAln._fields_}
        return [next(got) if d is not None else dict(zero) for d in d0]

    def prepare_segments(self, zmws, nthreads: int = 4) -> list:
        """ccsx_prepare_batch: per ZMW (a list of subread bytes) its push list
        (offs, lens, reverse flags), equal to prepare_segments'; info = the
        call's rounds, jobs and times."""
        nz = len(zmws)
        seqs = [b"".join(z) for z in zmws]
        lens = [_u32([len(s) for s in z]) for z in zmws]
        cap = [max(len(z), 1) for z in zmws]
        so = [np.zeros(c, dtype=np.uint32) for c in cap]
        sl = [np.zeros(c, dtype=np.uint32) for c in cap]
        rv = [np.zeros(c, dtype=np.uint8) for c in cap]
        m = max(nz, 1)
        a_seq = (C.c_char_p * m)(*seqs)
        a_len = (C.POINTER(C.c_uint32) * m)(*[_p32(x) for x in lens])
        a_n = _u32([len(z) for z in zmws])
        a_so = (C.POINTER(C.c_uint32) * m)(*[_p32(x) for x in so])
        a_sl = (C.POINTER(C.c_uint32) * m)(*[_p32(x) for x in sl])
        a_rv = (C.POINTER(C.c_uint8) * m)(*[x.ctypes.data_as(C.POINTER(C.c_uint8)) for x in rv])
        nseg = np.zeros(m, dtype=np.uint32)
        info = BatchInfo()
        if self._L.ccsx_prepare_batch(self._ctx, a_seq, a_len, _p32(a_n), nz, nthreads, a_so, a_sl, a_rv, _p32(nseg),
                                      C.byref(info)) != 0:
            self._err("ccsx_prepare_batch")
        self.info = {n: getattr(info, n) for n, _ in BatchInfo._fields_}
        return [(so[i][:nseg[i]].copy(), sl[i][:nseg[i]].copy(), rv[i][:nseg[i]].copy()) for i in range(nz)]

    def stats(self) -> dict:
        """ccsx_gpu_aln_stats: jobs, slices launched, jobs run on the host,
        rounds and second pairs not consulted (the last two by prepare_segments)."""
        st = (C.c_uint64 * 5)()
        if self._L.ccsx_gpu_aln_stats(self._ctx, st, 5) != 0:
            self._err("ccsx_gpu_aln_stats")
        return dict(zip(("jobs", "slices", "host_jobs", "rounds", "discarded"), (int(x) for x in st)))


BC_NONE = -(1 << 31)  # CCSX_BC_NONE: `second` of a set of one barcode
BC_REASONS = ("ok", "end0", "end1", "ends", "insert")  # ccsx_bc_call's reason (CCSX_BC_OK ...), as the -D file names it


def _barcode_set(barcodes):
    """(seqs, off, len) arrays of a barcode list for the C-ABI."""
    bs = [bytes(b) for b in barcodes]
    lens = _u32([len(b) for b in bs])
    offs = _u32(np.concatenate([[0], np.cumsum(lens)[:-1]])) if len(bs) else _u32([])
    return b"".join(bs), offs, lens


def _bc_ends(o: BcOut):
    v = [int(x) for x in o.v]
    return tuple(v[:5]), tuple(v[5:])


def barcode_host(barcodes, ccs: bytes, window: int = 96):
    """ccsx_barcode_host (SPEC.md §16): per end (pattern, score, end, second,
    second_pattern) of one CCS read; ValueError for a bad set or window."""
    seqs, offs, lens = _barcode_set(barcodes)
    out = BcOut()
    if lib().ccsx_barcode_host(seqs, _p32(offs), _p32(lens), len(lens), window, ccs, len(ccs), C.byref(out)) != 0:
        raise ValueError("not a barcode set (1..2048 sequences of 1..64 ACGT letters) or window outside 1..256")
    return _bc_ends(out)


def barcode_call(result, lens, n: int, T: int = 60, D: int = 3):
    """ccsx_barcode_call: from a read's result (the two ends' five values), the
    barcodes' lengths and the read's length: (cl, cr, (called0, called1),
    assigned, reason); reason indexes BC_REASONS."""
    o = BcOut()
    for k, x in enumerate(tuple(result[0]) + tuple(result[1])):
        o.v[k] = x
    ln = _u32(lens)
    call = BcCall()
    lib().ccsx_barcode_call(C.byref(o), _p32(ln), len(ln), n, T, D, C.byref(call))
    return int(call.cl), int(call.cr), (bool(call.called[0]), bool(call.called[1])), bool(call.assigned), int(call.reason)


def read_barcodes(path: str) -> list:
    """ccsx_barcode_read: [(name, sequence)] of a barcode FASTA, unchecked;
    OSError if it cannot be opened or holds no record."""
    L = lib()
    s = L.ccsx_barcode_read(os.fsencode(path))
    if not s:
        raise OSError(f"{path}: cannot open, or no record")
    try:
        names, seqs = C.POINTER(C.c_char_p)(), C.POINTER(C.c_char_p)()
        n = L.ccsx_barcode_set_get(s, C.byref(names), C.byref(seqs))
        return [(names[i].decode(), bytes(seqs[i])) for i in range(n)]
    finally:
        L.ccsx_barcode_set_free(s)


class Demux:
    """A demultiplexer context on one HIP device (ccsx_gpu_bc_*): SPEC.md §16's
    scores of every barcode pattern against both end windows of many CCS reads
    per launch; max_bytes = the most device memory its arena takes (0: the
    library's default)."""

    def __init__(self, device: int = 0, max_bytes: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_bc_open(device, max_bytes, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open a demultiplexer on HIP device {device}")
        self.kernel_ms = 0.0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_bc_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_bc_error(self._ctx).decode()}")

    def set(self, barcodes, window: int = 96) -> None:
        """ccsx_gpu_bc_set: the set and window of the calls that follow;
        ValueError for a bad one (the earlier set stays)."""
        seqs, offs, lens = _barcode_set(barcodes)
        if not 0 <= window < 1 << 32:
            raise ValueError("window outside 1..256")
        if self._L.ccsx_gpu_bc_set(self._ctx, seqs, _p32(offs), _p32(lens), len(lens), window) != 0:
            if self._L.ccsx_barcode_check(seqs, _p32(offs), _p32(lens), len(lens)) != 0 or not 1 <= window <= 256:
                raise ValueError("not a barcode set (1..2048 sequences of 1..64 ACGT letters) or window outside 1..256")
            self._err("ccsx_gpu_bc_set")

    def score(self, reads) -> list:
        """ccsx_gpu_bc_score on a list of CCS reads: per read the two ends'
        (pattern, score, end, second, second_pattern), as barcode_host
        returns; kernel_ms = the kernel's time."""
        n = len(reads)
        arr = (BcIn * max(n, 1))()
        keep = [bytes(r) for r in reads]
        for i, r in enumerate(keep):
            arr[i].ccs, arr[i].len = r, len(r)
        out = (BcOut * max(n, 1))()
        ms = C.c_float(0)
        if self._L.ccsx_gpu_bc_score(self._ctx, arr, n, out, C.byref(ms)) != 0:
            self._err("ccsx_gpu_bc_score")
        self.kernel_ms = float(ms.value)
        return [_bc_ends(out[i]) for i in range(n)]

    def stats(self) -> dict:
        """ccsx_gpu_bc_stats: reads scored, slices launched, sets."""
        st = (C.c_uint64 * 3)()
        if self._L.ccsx_gpu_bc_stats(self._ctx, st, 3) != 0:
            self._err("ccsx_gpu_bc_stats")
        return dict(zip(("zmws", "slices", "sets"), (int(x) for x in st)))


_SCAN_SET_ERR = "not an adapter set (1..64 sequences of 1..64 ACGT letters) or threshold outside 1..100"


def _scan_hit(h: ScanHit) -> tuple:
    return int(h.adapter), int(h.orient), int(h.start), int(h.end), int(h.score)


def scan_host(adapters, ccs: bytes, T: int = 75) -> list:
    """ccsx_scan_host (SPEC.md §17): the hits of one CCS read as (adapter,
    orient, start, end, score) by (end, adapter); ValueError for a bad set or T."""
    seqs, offs, lens = _barcode_set(adapters)
    if not 0 <= T < 1 << 32:
        raise ValueError(_SCAN_SET_ERR)
    L = lib()
    n = L.ccsx_scan_host(seqs, _p32(offs), _p32(lens), len(lens), T, ccs, len(ccs), None, 0)
    if n < 0:
        raise ValueError(_SCAN_SET_ERR)
    hits = (ScanHit * max(n, 1))()
    if L.ccsx_scan_host(seqs, _p32(offs), _p32(lens), len(lens), T, ccs, len(ccs), hits, n) != n:
        raise RuntimeError("ccsx_scan_host: the second pass disagrees with the first")
    return [_scan_hit(hits[i]) for i in range(n)]


def scan_start(adapter: bytes, orient: int, ccs: bytes, end: int) -> tuple:
    """ccsx_scan_start: (start, the anchored maximum) of a hit that ends at
    column `end`."""
    sc = C.c_int32(0)
    s = lib().ccsx_scan_start(bytes(adapter), len(adapter), orient, ccs, len(ccs), end, C.byref(sc))
    if s < 0:
        raise ValueError("adapter length outside 1..64 or end past the read")
    return int(s), int(sc.value)


def scan_cut(hits, n: int, lmin: int = 50) -> list:
    """ccsx_scan_cut: the pieces (b, e, left, right) of a read of n bases from
    its hits (as scan_host lists them); left / right index the flanking hit,
    -1 at the read's end."""
    arr = (ScanHit * max(len(hits), 1))()
    for k, (a, o, s, e, sc) in enumerate(hits):
        arr[k].adapter, arr[k].orient, arr[k].start, arr[k].end, arr[k].score = a, o, s, e, sc
    L = lib()
    m = L.ccsx_scan_cut(arr, len(hits), n, lmin, None, 0)
    out = (ScanPiece * max(m, 1))()
    L.ccsx_scan_cut(arr, len(hits), n, lmin, out, m)
    return [(int(p.b), int(p.e), int(p.left), int(p.right)) for p in out[:m]]


class Scanner:
    """An adapter scanner context on one HIP device (ccsx_gpu_scan_*): SPEC.md
    §17's hits of every adapter, in both orientations, along whole CCS reads,
    many reads per launch; max_bytes = the most device memory its arena takes
    (0: the library's default)."""

    def __init__(self, device: int = 0, max_bytes: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_scan_open(device, max_bytes, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open a scanner on HIP device {device}")
        self.kernel_ms = 0.0
        self._npat = 0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_scan_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_scan_error(self._ctx).decode()}")

    @staticmethod
    def tile(rows: int) -> tuple:
        """ccsx_gpu_scan_tile: (TC, WU) of the kernel for `rows` rows."""
        tc, wu = C.c_uint32(0), C.c_uint32(0)
        if lib().ccsx_gpu_scan_tile(rows, C.byref(tc), C.byref(wu)) != 0:
            raise ValueError("rows is one of 16, 32, 48, 64")
        return int(tc.value), int(wu.value)

    def set(self, adapters, T: int = 75) -> None:
        """ccsx_gpu_scan_set: the set and threshold of the calls that follow;
        ValueError for a bad one (the earlier set stays)."""
        seqs, offs, lens = _barcode_set(adapters)
        if not 0 <= T < 1 << 32:
            raise ValueError(_SCAN_SET_ERR)
        if self._L.ccsx_gpu_scan_set(self._ctx, seqs, _p32(offs), _p32(lens), len(lens), T) != 0:
            if self._L.ccsx_scan_check(seqs, _p32(offs), _p32(lens), len(lens), T) != 0:
                raise ValueError(_SCAN_SET_ERR)
            self._err("ccsx_gpu_scan_set")
        self._npat = 2 * len(lens)

    def _reads(self, reads):
        keep = [bytes(r) for r in reads]
        arr = (BcIn * max(len(keep), 1))()
        for i, r in enumerate(keep):
            arr[i].ccs, arr[i].len = r, len(r)
        return keep, arr

    def scan(self, reads) -> list:
        """ccsx_gpu_scan on a list of CCS reads: per read its hits as
        scan_host returns them; kernel_ms = the kernels' time."""
        keep, arr = self._reads(reads)
        hits, n, ms = C.POINTER(ScanHit)(), C.c_uint64(0), C.c_float(0)
        if self._L.ccsx_gpu_scan(self._ctx, arr, len(keep), C.byref(hits), C.byref(n), C.byref(ms)) != 0:
            self._err("ccsx_gpu_scan")
        self.kernel_ms = float(ms.value)
        out = [[] for _ in keep]
        for k in range(n.value):
            out[hits[k].read].append(_scan_hit(hits[k]))
        return out

    def tracks(self, reads) -> list:
        """ccsx_gpu_scan_tracks: per read the bottom rows S_p(j) of the set's
        patterns as an int8 array of shape (2 A, len + 1)."""
        keep, arr = self._reads(reads)
        total = sum(self._npat * (len(r) + 1) for r in keep)
        buf = np.zeros(max(total, 1), np.int8)
        if self._L.ccsx_gpu_scan_tracks(self._ctx, arr, len(keep), buf.ctypes.data, total) != 0:
            self._err("ccsx_gpu_scan_tracks")
        out, at = [], 0
        for r in keep:
            sz = self._npat * (len(r) + 1)
            out.append(buf[at:at + sz].reshape(self._npat, len(r) + 1))
            at += sz
        return out

    def stats(self) -> dict:
        """ccsx_gpu_scan_stats: reads scanned, slices launched, sets,
        candidates, re-runs with the counted capacity, reads scanned on the host."""
        st = (C.c_uint64 * 6)()
        if self._L.ccsx_gpu_scan_stats(self._ctx, st, 6) != 0:
            self._err("ccsx_gpu_scan_stats")
        return dict(zip(("reads", "slices", "sets", "candidates", "reruns", "host_reads"), (int(x) for x in st)))


REF_FIELDS = ("g", "o", "d0", "votes", "votes2", "qb", "qe", "tb", "te", "mat", "mis", "ins", "del", "aln", "score")
_REF_SET_ERR = "not a reference set (1..64 sequences of at least 13 letters, at most 1,048,576 letters in all)"


def read_refs(path: str) -> list:
    """[(name, sequence)] of a reference FASTA (ccsx_barcode_read), unchecked;
    OSError if it cannot be opened or holds no record."""
    return read_barcodes(path)


class RefSet:
    """A ccsx_ref_set (ccsx_ref_set_make); ValueError for a bad one."""

    def __init__(self, refs):
        seqs, offs, lens = _barcode_set(refs)
        self._L = lib()
        self.p = self._L.ccsx_ref_set_make(seqs, _p32(offs), _p32(lens), len(lens))
        if not self.p:
            raise ValueError(_REF_SET_ERR)

    def __del__(self):
        if getattr(self, "p", None):
            self._L.ccsx_ref_set_free(self.p)
            self.p = None


def _ref_rec(r: RefRec) -> tuple:
    return tuple(int(x) for x in r.v)


def ref_host(refs, ccs: bytes, words: bool = True):
    """ccsx_ref_host (SPEC.md §18) of one CCS read against the reference
    sequences `refs` (or a RefSet made from them once): (record,
    words); the record as a tuple in REF_FIELDS' order, the words as a uint32
    array of the read's length (of the read in orientation o), or None."""
    rs = refs if isinstance(refs, RefSet) else RefSet(refs)
    ccs = bytes(ccs)
    rec = RefRec()
    w = np.zeros(max(len(ccs), 1), np.uint32) if words else None
    if lib().ccsx_ref_host(rs.p, ccs, len(ccs), C.byref(rec), w.ctypes.data if words else None) != 0:
        raise RuntimeError("ccsx_ref_host failed")
    return _ref_rec(rec), (w[:len(ccs)] if words else None)


def ref_pass(rec, y: int = 50, Y: int = 75) -> bool:
    """ccsx_ref_pass: a mapped read is reported iff aln >= y and 100 mat >= Y aln."""
    r = RefRec()
    for k, x in enumerate(rec):
        r.v[k] = x
    return bool(lib().ccsx_ref_pass(C.byref(r), y, Y))


class RefMapper:
    """A reference mapper context on one HIP device (ccsx_gpu_ref_*): SPEC.md
    §18's seed, band and path of many CCS reads per call against a reference
    set; max_bytes = the most device memory its arena takes (0: the library's
    default, 4 GiB)."""

    def __init__(self, device: int = 0, max_bytes: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_ref_open(device, max_bytes, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open a reference mapper on HIP device {device}")
        self.vote_ms = self.band_ms = 0.0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_ref_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_ref_error(self._ctx).decode()}")

    def set(self, refs) -> None:
        """ccsx_gpu_ref_set: the reference sequences of the calls that follow;
        ValueError for a bad set (the earlier one stays)."""
        rs = RefSet(refs)
        if self._L.ccsx_gpu_ref_set(self._ctx, rs.p) != 0:
            self._err("ccsx_gpu_ref_set")

    def vote_cap(self, slots: int) -> None:
        """ccsx_gpu_ref_vote_cap: the slots of the vote kernel's table (a power
        of two in 64 .. 4096); a read with more distinct (target, orientation,
        bin) keys is mapped on the host."""
        if not 0 <= slots < 1 << 32 or self._L.ccsx_gpu_ref_vote_cap(self._ctx, slots) != 0:
            raise ValueError("a power of two in 64 .. 4096")

    def map(self, reads, words: bool = True) -> list:
        """ccsx_gpu_ref_map on a list of CCS reads: per read (record, words) as
        ref_host returns them; vote_ms / band_ms = the kernels' times."""
        keep = [bytes(r) for r in reads]
        n = len(keep)
        arr = (BcIn * max(n, 1))()
        for i, r in enumerate(keep):
            arr[i].ccs, arr[i].len = r, len(r)
        recs = (RefRec * max(n, 1))()
        total = sum(len(r) for r in keep)
        w = np.zeros(max(total, 1), np.uint32) if words else None
        ms = (C.c_float * 2)()
        if self._L.ccsx_gpu_ref_map(self._ctx, arr, n, recs, w.ctypes.data if words else None, ms) != 0:
            self._err("ccsx_gpu_ref_map")
        self.vote_ms, self.band_ms = float(ms[0]), float(ms[1])
        out, at = [], 0
        for i, r in enumerate(keep):
            out.append((_ref_rec(recs[i]), w[at:at + len(r)].copy() if words else None))
            at += len(r)
        return out

    def stats(self) -> dict:
        """ccsx_gpu_ref_stats: reads, slices launched, sets, reads mapped,
        reads whose votes overflowed, reads mapped on the host."""
        st = (C.c_uint64 * 6)()
        if self._L.ccsx_gpu_ref_stats(self._ctx, st, 6) != 0:
            self._err("ccsx_gpu_ref_stats")
        return dict(zip(("reads", "slices", "sets", "mapped", "overflows", "host_reads"), (int(x) for x in st)))


class Polisher:
    """A polisher context on one HIP device (ccsx_gpu_polish_*): SPEC.md §15's
    realignment of every pushed segment to the draft CCS, the vote and the
    polished read, for many ZMWs per launch; max_bytes = the most device memory
    its arena takes (0: the library's default)."""

    def __init__(self, device: int = 0, max_bytes: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_polish_open(device, max_bytes, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open a polisher on HIP device {device}")
        self.kernel_ms = 0.0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_polish_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_polish_error(self._ctx).decode()}")

    def polish(self, items) -> list:
        """ccsx_gpu_polish on items = [(ccs, segs, maps)]: the draft, its
        segments as pushed and their §11 maps (Engine.base_map).  Per ZMW
        (seq, qual, (nsub, nins, ndel), [realigned map per segment], status), as
        polish_host returns; kernel_ms = the kernels' time."""
        n = len(items)
        arr = (PolishIn * max(n, 1))()
        keep = []
        for i, (ccs, segs, maps) in enumerate(items):
            seqs, offs, lens, m = _polish_item(ccs, segs, maps)
            keep.append((ccs, seqs, offs, lens, m))
            arr[i].ccs, arr[i].len, arr[i].seqs, arr[i].nseg = ccs, len(ccs), seqs, len(segs)
            arr[i].seg_off, arr[i].seg_len, arr[i].map = _p32(offs), _p32(lens), _p32(m)
        out = (PolishOut * max(n, 1))()
        ms = C.c_float(0)
        if self._L.ccsx_gpu_polish(self._ctx, arr, n, out, C.byref(ms)) != 0:
            self._err("ccsx_gpu_polish")
        self.kernel_ms = float(ms.value)
        res = []
        for i, (ccs, segs, maps) in enumerate(items):
            o = out[i]
            if o.status != 0:
                res.append((b"", b"", (0, 0, 0), [], int(o.status)))
                continue
            rows = sum(len(x) for x in segs)
            m = np.ctypeslib.as_array(o.map, (rows,)).copy() if rows else np.zeros(0, np.uint32)
            res.append((C.string_at(o.seq, o.len), C.string_at(o.qual, o.len), (int(o.nsub), int(o.nins), int(o.ndel)),
                        _split_map(m, segs), 0))
        return res

    def stats(self) -> dict:
        """ccsx_gpu_polish_stats: ZMWs, segments, slices launched, ZMWs run on
        the host, ZMWs with a bad map."""
        st = (C.c_uint64 * 5)()
        if self._L.ccsx_gpu_polish_stats(self._ctx, st, 5) != 0:
            self._err("ccsx_gpu_polish_stats")
        return dict(zip(("zmws", "segments", "slices", "host_zmws", "bad_maps"), (int(x) for x in st)))


class Engine:
    """A context on one HIP device: the batched C-ABI of include/ccsx_gpu.h."""

    def __init__(self, device: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        if self._L.ccsx_gpu_open(device, C.byref(self._ctx)) != 0:
            raise GpuError(f"cannot open HIP device {device}")
        self._keep = None
        self._nz = 0

    def close(self):
        if self._ctx:
            self._L.ccsx_gpu_close(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what: str):
        raise GpuError(f"{what}: {self._L.ccsx_gpu_error(self._ctx).decode()}")

    @staticmethod
    def _build_in(zmws: list[Prepared]):
        arr = (ZmwIn * max(len(zmws), 1))()
        keep = []
        for i, z in enumerate(zmws):
            offs, lens = _u32(z.offs), _u32(z.lens)
            keep += [z.seqs, offs, lens]
            arr[i].seqs = z.seqs
            arr[i].seg_off = _p32(offs)
            arr[i].seg_len = _p32(lens)
            arr[i].nseg = len(lens)
            rev = getattr(z, "rev", None)
            if rev is not None:
                rev = np.ascontiguousarray(np.asarray(rev, dtype=np.uint8))
                if len(rev) != len(lens):
                    raise ValueError("Prepared.rev needs one flag per segment")
                keep.append(rev)
                arr[i].seg_rev = rev.ctypes.data_as(C.POINTER(C.c_uint8))
            ipd, pw = getattr(z, "ipd", None), getattr(z, "pw", None)
            if ipd is not None and pw is not None:
                if len(ipd) != len(z.seqs) or len(pw) != len(z.seqs):
                    raise ValueError("Prepared.ipd / .pw need one code per byte of seqs")
                bi, bp = np.frombuffer(bytes(ipd), np.uint8), np.frombuffer(bytes(pw), np.uint8)
                keep += [bi, bp]
                arr[i].ipd = bi.ctypes.data_as(C.POINTER(C.c_uint8))
                arr[i].pw = bp.ctypes.data_as(C.POINTER(C.c_uint8))
        return arr, keep

    def stage(self, zmws: list[Prepared], mode: int | None = None) -> None:
        """Stage a slice (tight capacities); with `mode`, the capacities
        ccsx_gpu_run uses for that mode (ccsx_gpu_stage_for)."""
        arr, keep = self._build_in(zmws)
        rc = (self._L.ccsx_gpu_stage(self._ctx, arr, len(zmws)) if mode is None
              else self._L.ccsx_gpu_stage_for(self._ctx, mode, arr, len(zmws)))
        if rc != 0:
            self._err("ccsx_gpu_stage")
        self._keep = (arr, keep)
        self._nz = len(zmws)

    def launch(self, mode: int = MODE_SHRED) -> float:
        ms = C.c_float(0)
        if self._L.ccsx_gpu_launch(self._ctx, mode, C.byref(ms)) != 0:
            self._err("ccsx_gpu_launch")
        return ms.value

    def fetch(self):
        out = (ZmwOut * max(self._nz, 1))()
        rc = self._L.ccsx_gpu_fetch(self._ctx, out)
        if rc != 0:
            self._err("ccsx_gpu_fetch")
        res = []
        for i in range(self._nz):
            o = out[i]
            res.append((C.string_at(o.ccs, o.len) if o.len else b"", o.status, o.cells))
        return res

    def run(self, zmws: list[Prepared], mode: int = MODE_SHRED):
        """ccsx_gpu_run (memory-sized slices, full-capacity re-run of ZMWs that
        outgrow the tight workspace): returns [(ccs bytes, status, cells)]."""
        arr, keep = self._build_in(zmws)
        out = (ZmwOut * max(len(zmws), 1))()
        if self._L.ccsx_gpu_run(self._ctx, mode, arr, len(zmws), out) != 0:
            self._err("ccsx_gpu_run")
        return [(C.string_at(out[i].ccs, out[i].len) if out[i].len else b"", out[i].status, out[i].cells)
                for i in range(len(zmws))]

    def single_poa(self, reads: list[bytes]):
        """One POA of `reads` on this context (ccsx_gpu_single_poa, the path
        of the bspoa-compatible API; a forced kernel object applies): returns
        (consensus codes uint8 [ncns], tidy MSA uint8 [ncols, nseq + 4])."""
        fn = self._L.ccsx_gpu_single_poa
        fn.argtypes = [C.c_void_p, C.POINTER(ZmwIn), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        offs, o = [], 0
        for r in reads:
            offs.append(o)
            o += len(r)
        arr, keep = self._build_in([Prepared(b"".join(reads), _u32(offs), _u32([len(r) for r in reads]))])
        cns, msa = C.c_void_p(), C.c_void_p()
        ncns, ncols = C.c_uint32(0), C.c_uint32(0)
        if fn(self._ctx, arr, C.byref(cns), C.byref(ncns), C.byref(msa), C.byref(ncols)) != 0:
            self._err("ccsx_gpu_single_poa")
        self._nz = 1
        mrow = len(reads) + 4
        # (the engine returns the consensus as letters; bspoa's g->cns holds codes)
        letters = C.string_at(cns, ncns.value) if ncns.value else b""
        c = np.frombuffer(letters.translate(bytes.maketrans(b"ACGT", bytes(range(4)))), dtype=np.uint8).copy()
        m = (np.frombuffer(C.string_at(msa, ncols.value * mrow), dtype=np.uint8).reshape(ncols.value, mrow).copy()
             if ncols.value else np.zeros((0, mrow), np.uint8))
        return c, m

    def run_batch(self, batch: "SynthBatch", mode: int = MODE_SHRED, keep=()):
        """ccsx_gpu_run on a synthetic batch; returns [(status, cells, len)]
        and, when `keep` lists batch indices, also {index: CCS bytes}."""
        out = (ZmwOut * max(batch.n, 1))()
        rc = self._L.ccsx_gpu_run(self._ctx, mode, batch.zmws, batch.n, out)
        if rc != 0:
            self._err("ccsx_gpu_run")
        res = [(out[i].status, out[i].cells, out[i].len) for i in range(batch.n)]
        if keep:
            return res, {i: C.string_at(out[i].ccs, out[i].len) if out[i].len else b"" for i in keep}
        return res

    def stage_batch(self, batch: "SynthBatch", mode: int = MODE_SHRED) -> None:
        """ccsx_gpu_stage_for on a synthetic batch (inputs resident for launch())."""
        if self._L.ccsx_gpu_stage_for(self._ctx, mode, batch.zmws, batch.n) != 0:
            self._err("ccsx_gpu_stage_for")
        self._keep = batch
        self._nz = batch.n

    def set_mem_share(self, share: int) -> None:
        """This context uses at most 1/share of the device's memory (several
        contexts, or processes, on one device)."""
        if self._L.ccsx_gpu_set_mem_share(self._ctx, share) != 0:
            self._err("ccsx_gpu_set_mem_share")

    def set_kernel_cfg(self, cfg: int) -> None:
        """-1 = by slice size, 0 = latency (8-row blocks), 1 = occupancy (4-row blocks)."""
        if self._L.ccsx_gpu_set_kernel_cfg(self._ctx, cfg) != 0:
            self._err("ccsx_gpu_set_kernel_cfg")

    def kernel_cfg(self) -> int:
        return int(self._L.ccsx_gpu_kernel_cfg(self._ctx))

    def rerun_count(self) -> int:
        """ZMWs run() has re-run with full caps so far."""
        return int(self._L.ccsx_gpu_rerun_count(self._ctx))

    def hbm_launches(self) -> int:
        """Slices launched on the HBM-read kernel instance so far."""
        return int(self._L.ccsx_gpu_hbm_launches(self._ctx))

    def run_stats(self) -> dict:
        """ccsx_gpu_run counters so far: reruns, slices, dealt lists, their
        parts, slices that waited for device memory, slices cut below the plan."""
        st = (C.c_uint64 * 6)()
        if self._L.ccsx_gpu_run_stats(self._ctx, st, 6) != 0:
            self._err("ccsx_gpu_run_stats")
        return dict(zip(("reruns", "slices", "dealt", "parts", "mem_waits", "mem_replans"), (int(x) for x in st)))

    def set_mem_wait(self, ms: int) -> None:
        """How long a slice waits for device memory a neighbour still holds."""
        if self._L.ccsx_gpu_set_mem_wait(self._ctx, ms) != 0:
            self._err("ccsx_gpu_set_mem_wait")

    def zmw_bytes(self, z: Prepared, mode: int = MODE_SHRED) -> int:
        """Device bytes one ZMW occupies in a ccsx_gpu_run slice of `mode`."""
        arr, keep = self._build_in([z])
        return int(self._L.ccsx_gpu_zmw_bytes(self._ctx, mode, arr))

    def slot_bytes(self) -> int:
        """ccsx_gpu_slot_bytes: the bytes one submitted batch may take."""
        v = C.c_uint64(0)
        if self._L.ccsx_gpu_slot_bytes(self._ctx, C.byref(v)) != 0:
            self._err("ccsx_gpu_slot_bytes")
        return int(v.value)

    def submit(self, zmws: list, mode: int = MODE_SHRED) -> int:
        """ccsx_gpu_submit: stage + launch one batch on a free slot (returns
        the slot to collect; raises on -3 / -4 with the code in the message)."""
        arr, keep = self._build_in(zmws)
        slot = C.c_int(-1)
        rc = self._L.ccsx_gpu_submit(self._ctx, mode, arr, len(zmws), C.byref(slot))
        if rc != 0:
            self._err(f"ccsx_gpu_submit ({rc})")
        self._tickets = getattr(self, "_tickets", {})
        self._tickets[slot.value] = (arr, keep, len(zmws))
        return slot.value

    def collect(self, slot: int):
        """ccsx_gpu_collect: [(ccs bytes, status, cells)] of a submitted batch."""
        arr, keep, n = self._tickets.pop(slot)
        out = (ZmwOut * max(n, 1))()
        rc = self._L.ccsx_gpu_collect(self._ctx, slot, out)
        if rc not in (0, -2):
            self._err("ccsx_gpu_collect")
        return [(C.string_at(out[i].ccs, out[i].len) if out[i].len else b"", out[i].status, out[i].cells)
                for i in range(n)]

    def set_quality(self, on: bool = True) -> None:
        """Per-base qualities for the following stage / run / submit calls
        (ccsx_gpu_set_quality): a second output plane, read with quality()."""
        if self._L.ccsx_gpu_set_quality(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_quality")

    def quality(self, i: int, slot: int = -1) -> bytes:
        """Raw quality bytes (0..93) of ZMW i: of the last run() / fetch()
        (slot -1) or of the batch collected from `slot`; raises if that batch
        ran with quality off."""
        p = C.c_void_p()
        n = C.c_uint32(0)
        if self._L.ccsx_gpu_quality(self._ctx, slot, i, C.byref(p), C.byref(n)) != 0:
            self._err("ccsx_gpu_quality")
        return C.string_at(p, n.value) if n.value else b""

    def set_pass_stats(self, on: bool = True) -> None:
        """Per-pass alignment statistics for the following stage / run / submit
        calls (ccsx_gpu_set_pass_stats): one record per segment, read with
        pass_stats()."""
        if self._L.ccsx_gpu_set_pass_stats(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_pass_stats")

    def pass_stats(self, i: int, slot: int = -1) -> np.ndarray:
        """The pass records of ZMW i, uint32 [nseg, 6] = match, mismatch, ins,
        del, cbeg, cend per segment in push order: of the last run() / fetch()
        (slot -1) or of the batch collected from `slot`; raises if that batch
        ran with pass statistics off or the ZMW failed."""
        p = C.c_void_p()
        n = C.c_uint32(0)
        if self._L.ccsx_gpu_pass_stats(self._ctx, slot, i, C.byref(p), C.byref(n)) != 0:
            self._err("ccsx_gpu_pass_stats")
        if not n.value:
            return np.zeros((0, 6), np.uint32)
        return np.frombuffer(C.string_at(p, n.value * 24), dtype=np.uint32).reshape(n.value, 6).copy()

    def set_base_map(self, on: bool = True) -> None:
        """The subread-to-CCS coordinate map for the following stage / run /
        submit calls (ccsx_gpu_set_base_map): one uint32 per pushed base (SPEC.md
        §11), read with base_map()."""
        if self._L.ccsx_gpu_set_base_map(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_base_map")

    def base_map(self, i: int, slot: int = -1) -> list:
        """The map of ZMW i: one read-only uint32 array per segment in push
        order, seg_len[k] words in base order (bits 0..29 the CCS offset, bit 30
        mismatch, bit 31 insertion): of the last run() / fetch() (slot -1) or of
        the batch collected from `slot`; raises if that batch ran with the map
        off or the ZMW failed."""
        segs = []
        while True:
            p = C.POINTER(C.c_uint32)()
            n = C.c_uint32(0)
            if self._L.ccsx_gpu_base_map(self._ctx, slot, i, len(segs), C.byref(p), C.byref(n)) != 0:
                # (every refusal but "segment beyond the ZMW's" also refuses segment 0)
                if not segs:
                    self._err("ccsx_gpu_base_map")
                return segs
            a = np.ctypeslib.as_array(p, (n.value,)).copy() if n.value else np.zeros(0, np.uint32)
            a.setflags(write=False)
            segs.append(a)

    def set_pileup(self, on: bool = True) -> None:
        """The per-base strand pileup for the following stage / run / submit
        calls (ccsx_gpu_set_pileup): twelve bytes per CCS base (SPEC.md §12),
        read with pileup()."""
        if self._L.ccsx_gpu_set_pileup(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_pileup")

    def pileup(self, i: int, slot: int = -1) -> np.ndarray:
        """The pileup of ZMW i, uint8 [len, 12]: per CCS base the forward reads'
        A, C, G, T, gap, ins counts, then the reverse reads', each saturating at
        255: of the last run() / fetch() (slot -1) or of the batch collected
        from `slot`; raises if that batch ran with the pileup off or the ZMW
        failed."""
        p = C.c_void_p()
        n = C.c_uint32(0)
        if self._L.ccsx_gpu_pileup(self._ctx, slot, i, C.byref(p), C.byref(n)) != 0:
            self._err("ccsx_gpu_pileup")
        if not n.value:
            return np.zeros((0, 12), np.uint8)
        return np.frombuffer(C.string_at(p, n.value * 12), dtype=np.uint8).reshape(n.value, 12).copy()

    def set_kinetics(self, on: bool = True) -> None:
        """The per-base consensus kinetics for the following stage / run /
        submit calls (ccsx_gpu_set_kinetics): eight bytes per CCS base (SPEC.md
        §13) from Prepared.ipd / .pw, read with kinetics()."""
        if self._L.ccsx_gpu_set_kinetics(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_kinetics")

    def kinetics(self, i: int, slot: int = -1) -> np.ndarray:
        """The kinetics of ZMW i, uint8 [len, 8]: per CCS base the forward
        reads' code of the mean ipd, code of the mean pw and min(reads, 255),
        then the reverse reads', then two zero bytes: of the last run() /
        fetch() (slot -1) or of the batch collected from `slot`; raises if that
        batch ran with kinetics off or the ZMW failed."""
        p = C.c_void_p()
        n = C.c_uint32(0)
        if self._L.ccsx_gpu_kinetics(self._ctx, slot, i, C.byref(p), C.byref(n)) != 0:
            self._err("ccsx_gpu_kinetics")
        if not n.value:
            return np.zeros((0, 8), np.uint8)
        return np.frombuffer(C.string_at(p, n.value * 8), dtype=np.uint8).reshape(n.value, 8).copy()

    def set_by_strand(self, on: bool = True) -> None:
        """The per-strand consensus for the following stage / run / submit calls
        (ccsx_gpu_set_by_strand): the sequence each strand's reads support in
        the MSA the CCS was called from (SPEC.md §14), read with by_strand()."""
        if self._L.ccsx_gpu_set_by_strand(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_by_strand")

    def by_strand(self, i: int, slot: int = -1):
        """The strand consensuses of ZMW i: (forward bases, forward qualities
        uint8 [len_fwd], reverse bases, reverse qualities uint8 [len_rev]), both
        in the CCS's orientation, a strand without a pushed segment empty: of
        the last run() / fetch() (slot -1) or of the batch collected from
        `slot`; raises if that batch ran with the output off or the ZMW failed."""
        out = []
        for strand in (0, 1):
            p, q = C.c_void_p(), C.c_void_p()
            n = C.c_uint32(0)
            if self._L.ccsx_gpu_by_strand(self._ctx, slot, i, strand, C.byref(p), C.byref(q), C.byref(n)) != 0:
                self._err("ccsx_gpu_by_strand")
            out.append(C.string_at(p, n.value) if n.value else b"")
            out.append(np.frombuffer(C.string_at(q, n.value), dtype=np.uint8).copy() if n.value else np.zeros(0, np.uint8))
        return tuple(out)

    def set_fault(self, i: int) -> None:
        """Test hook (ccsx_gpu_set_fault): the next run() / submit() reports ZMW
        i of its batch as failed after computing it; -1 = off."""
        if self._L.ccsx_gpu_set_fault(self._ctx, i) != 0:
            self._err("ccsx_gpu_set_fault")

    def set_bp_log(self, on: bool = True) -> None:
        """Record the -v >= 3 breakpoint log (main.c:619-620) in ccsx_gpu_run."""
        if self._L.ccsx_gpu_set_bp_log(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_bp_log")

    def bp_log(self, i: int) -> list:
        """(breakpoint, MSA columns) per shredding round of ZMW i of the last run()."""
        pr = C.POINTER(C.c_uint32)()
        n = C.c_uint32(0)
        if self._L.ccsx_gpu_bp_log(self._ctx, i, C.byref(pr), C.byref(n)) != 0:
            self._err("ccsx_gpu_bp_log")
        return [(int(pr[2 * r]), int(pr[2 * r + 1])) for r in range(n.value)]

    def set_slot_budget(self, nbytes: int) -> None:
        """Test hook: bytes per ccsx_gpu_run slot (0 = by device memory)."""
        if self._L.ccsx_gpu_set_slot_budget(self._ctx, nbytes) != 0:
            self._err("ccsx_gpu_set_slot_budget")

    def set_wg_cap(self, wg_per_cu: int) -> None:
        """Measurement hook: at most wg_per_cu resident workgroups per CU (0 = off)."""
        if self._L.ccsx_gpu_set_wg_cap(self._ctx, wg_per_cu) != 0:
            self._err("ccsx_gpu_set_wg_cap")

    def set_shred_read_cap(self, bases: int) -> None:
        """The LDS read buffer of tight-cap shredded slices, in bases."""
        if self._L.ccsx_gpu_set_shred_read_cap(self._ctx, bases) != 0:
            self._err("ccsx_gpu_set_shred_read_cap")

    def set_tight_rows(self, rows: int) -> None:
        """Test hook: override the tight row capacity (0 = default)."""
        self._L.ccsx_gpu_set_tight_rows(self._ctx, rows)

    def set_tight_far(self, rows: int) -> None:
        """Test hook: override the tight far slot record rows (0 = default)."""
        self._L.ccsx_gpu_set_tight_far(self._ctx, rows)

    def set_prealloc(self, on: bool) -> None:
        """Pinned staging floors and one-off slice budget, as the CLI's contexts."""
        self._L.ccsx_gpu_set_prealloc(self._ctx, 1 if on else 0)

    def set_stage_piece(self, nbytes: int) -> None:
        """Test hook: half size of the piecewise subread staging (0 = default)."""
        self._L.ccsx_gpu_set_stage_piece(self._ctx, nbytes)

    def set_tight_out(self, nbytes: int) -> None:
        """Test hook: override the tight output slab in bytes (0 = default)."""
        self._L.ccsx_gpu_set_tight_out(self._ctx, nbytes)

    PROF_SLOTS = ("total", "load_read", "dp", "traceback", "merge", "columns", "shred", "dp_rows",
                  "row_A_fast", "row_B_general", "row_C_unused", "row_D_nfast", "row_E_store_loop", "flush", "spare0", "spare1",
                  "a_busy", "a_wait", "b_busy", "b_wait", "tw_rows", "sw_rows", "spare2", "spare3",
                  "tb_probe", "tb_step", "tb_di", "tb_switch", "tb_nsw", "hw0", "hw1", "hw2", "start_rt", "end_rt", "a_head", "a_body", "a_tail", "a_fast",
                  "cold_far", "cold_chain", "cold_np1", "cold_np2", "cold_gen", "cold_spill", "cold_near",
                  "n_far", "n_chain", "n_np1", "n_np2", "n_gen", "n_spill", "n_near",
                  "tb_isteps", "tb_iruns", "tb_dsteps", "tb_druns")

    def set_profiling(self, on: bool = True) -> None:
        """Per-phase counters on / off; raises with the product library (its
        objects carry none: CCSX_LIB=libccsx_amd_diag.so)."""
        if self._L.ccsx_gpu_set_profiling(self._ctx, 1 if on else 0) != 0:
            self._err("ccsx_gpu_set_profiling")

    def profile(self) -> dict:
        """Per-phase shader-clock cycles summed over the last launch's ZMWs."""
        buf = (C.c_uint64 * len(self.PROF_SLOTS))()
        if self._L.ccsx_gpu_profile(self._ctx, buf, len(self.PROF_SLOTS)) != 0:
            self._err("ccsx_gpu_profile")
        return {k: int(buf[i]) for i, k in enumerate(self.PROF_SLOTS)}

    def profile_zmw(self, nzmw: int) -> list:
        """The same counters per ZMW of the last launch (staging order)."""
        ns = len(self.PROF_SLOTS)
        buf = (C.c_uint64 * (nzmw * ns))()
        if self._L.ccsx_gpu_profile_zmw(self._ctx, buf, nzmw, ns) != 0:
            self._err("ccsx_gpu_profile_zmw")
        return [{k: int(buf[z * ns + i]) for i, k in enumerate(self.PROF_SLOTS)} for z in range(nzmw)]

    def staged_bytes(self) -> int:
        return int(self._L.ccsx_gpu_staged_bytes(self._ctx))
