"""Inputs of the strand pileup tests (SPEC.md §12), shared by the CPU and GPU
tests: tests/zmw_cases.py's edge cases with strand flags alternating 0, 1, 0, ...
in push order, and constructed exact cases whose records are known by
construction (tests/test_pileup_host.py states what each must show)."""
from __future__ import annotations

import random

import numpy as np

import ccsx_amd as cx

from .zmw_cases import _copies, _dirty_from, _other, _rb, edge_cases, raw, tie_cases

CARRY_G = (1, 3)
# the oracle's first round of the carry cases: (i, ncols) per g
CARRY_FIRST_ROUND = {1: (1947, 2001), 3: (1949, 2003)}


def with_rev(z: cx.Prepared, rev) -> cx.Prepared:
    return cx.Prepared(z.seqs, z.offs, z.lens, None if rev is None else np.asarray(rev, np.uint8))


def alternating(n: int) -> np.ndarray:
    return (np.arange(n) % 2).astype(np.uint8)


def edge() -> dict[str, cx.Prepared]:
    return {k: with_rev(z, alternating(len(z.lens))) for k, z in edge_cases().items()}


def carry_reads(g: int, both: bool) -> list[bytes]:
    """shred_cases()' dirty-column copies with g bases inserted ten columns under
    the first dirty column, in read 1 (both: in reads 1 and 3): the first round's
    last g emitted columns are gap-consensus columns."""
    rng = random.Random(7000)
    T = _rb(rng, 14000)
    reads = _copies(T, 5, 4200, dirty=_dirty_from(1956))
    ins = bytes(_other(T[1946], 1 + x % 2) for x in range(g))
    for k in (1, 3) if both else (1,):
        reads[k] = reads[k][:1946] + ins + reads[k][1946:]
    return reads


def saturation_reads() -> list[bytes]:
    """300 copies of a 60-base string, one substitution each (nw = 5)."""
    rng = random.Random(12000)
    S = _rb(rng, 60)
    return [S[:c] + bytes([_other(S[c], 1 + k % 3)]) + S[c + 1:] for k in range(300) for c in [5 + k % 50]]


def constructed() -> dict[str, cx.Prepared]:
    tie = tie_cases()
    cases = {}
    cases["heteroduplex"] = with_rev(raw(tie["split_2_2"]), [0, 1, 0, 1])
    cases["heteroduplex_same_strand"] = with_rev(raw(tie["split_2_2"]), [0, 0, 1, 1])
    cases["strand_deletion"] = with_rev(raw(tie["gap_equals_best_del"]), [0, 1, 1, 0])
    for g in CARRY_G:
        cases[f"carry_g{g}"] = with_rev(raw(carry_reads(g, False)), alternating(5))
        cases[f"carry_g{g}_two_reads"] = with_rev(raw(carry_reads(g, True)), alternating(5))
    cases["no_flags"] = with_rev(raw(tie["split_2_2"]), None)
    cases["reverse_only"] = with_rev(raw(tie["gap_equals_best_ins"]), [1, 1, 1, 1])
    sat = raw(saturation_reads())
    cases["saturation_alternating"] = with_rev(sat, alternating(300))
    cases["saturation_forward"] = with_rev(sat, np.zeros(300, np.uint8))
    return cases


CARRY_CASES = tuple(f"carry_g{g}{t}" for g in CARRY_G for t in ("", "_two_reads"))


def all_cases() -> dict[str, cx.Prepared]:
    return {**edge(), **constructed()}
