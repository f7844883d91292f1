"""Inputs of the per-strand consensus tests (SPEC.md §14) beside
tests/pileup_cases.all_cases(), shared by the CPU and GPU tests: constructed
exact cases whose strand consensuses are known by construction
(tests/test_strand_host.py states what each must show)."""
from __future__ import annotations

import random

import numpy as np

import ccsx_amd as cx

from .pileup_cases import all_cases as pileup_all_cases
from .pileup_cases import alternating, with_rev
from .zmw_cases import _rb, raw

PRIVATE_INS = 20  # the bases only the reverse reads of "private_insertion" carry
PRIVATE_AT = 200


def private_insertion_reads() -> list[bytes]:
    """Five exact copies of a 400-base string; reads 1 and 3 carry the same 20
    extra bases after base 200 (two reads of five: a gap-consensus stretch)."""
    rng = random.Random(14000)
    T = _rb(rng, 400)
    ins = _rb(rng, PRIVATE_INS)
    return [T[:PRIVATE_AT] + ins + T[PRIVATE_AT:] if k in (1, 3) else T for k in range(5)]


def constructed() -> dict[str, cx.Prepared]:
    rng = random.Random(14001)
    T = _rb(rng, 350)
    cases = {}
    # exact copies on both strands: fwd = rev = CCS
    cases["exact_both_strands"] = with_rev(raw([T] * 6), [0, 1, 1, 0, 1, 0])
    # flags given but all zero / all one: one strand is the CCS, the other empty
    cases["all_zero_flags"] = with_rev(raw([T, T[:300], T[20:], T]), np.zeros(4, np.uint8))
    cases["all_one_flags"] = with_rev(raw([T, T[:300], T[20:], T]), np.ones(4, np.uint8))
    # an insertion only the reverse reads carry: in the reverse consensus, not in the CCS
    cases["private_insertion"] = with_rev(raw(private_insertion_reads()), alternating(5))
    return cases


def all_cases() -> dict[str, cx.Prepared]:
    return {**pileup_all_cases(), **constructed()}
