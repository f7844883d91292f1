"""ccsx_amd -- MI355X-native engine for ccsx's per-ZMW circular-consensus hot path.

See DESIGN.md.  The product is the in-tree ``libccsx_amd.so`` (HIP kernels for
gfx950 + C-ABI, include/*.h); this package holds its build script and ctypes
bindings.
"""
from .native import (BC_NONE, BC_REASONS, MODE_PRIMITIVE, MODE_SHRED, POLISH_BAD_MAP, Aligner, Demux, Engine, GpuError, Prepared, kin_code, kin_frames, kinetics_tags, lib, map_cigar, pairwise, pairwise_band, pairwise_seed, partition, pileup_call,  # noqa: F401
                     barcode_call, barcode_host, pass_identity, Polisher, polish_host, read_barcodes, Prep, prepare, prepare_segments, qual_phred, qual_rq, read_calls, read_zmws, revcomp, scan_cut, scan_host, scan_start, Scanner, read_refs, ref_host, ref_pass, RefMapper, RefSet, REF_FIELDS, synth_zmw, zmw_cost)

__version__ = "0.1.0"
