"""The many-batch configuration of the host program's CLI tests and the check
that a run really spread.

The host program cuts a chunk into micro-batches of at least CCSX_MIN_BATCH
ZMWs (default 256; host/dispatch.cpp: nb = max(1, min(nparts, n / floor))), so
a test input of a few hundred ZMWs runs as one batch on one context in one
slot whatever CCSX_NGPU and CCSX_CTX_BATCHES say.  SPREAD lowers the floor and
the first chunk: chunks of 16, 64, 256, ... ZMWs (the first has CCSX_CHUNK0,
each next one four times the last), 2 x 2 contexts, 4 x 3 = 12 parts asked per
chunk and a floor of 4, so a chunk of n ZMWs is cut into min(12, n / 4)
batches: 4, 12, 12, ...  CCSX_TIMING makes the program say on stderr which
context ran which batch; assert_spread() reads that.
"""
from __future__ import annotations

import re

SPREAD = dict(CCSX_NGPU="2", CCSX_SLOTS="2", CCSX_CTX_BATCHES="3", CCSX_MIN_BATCH="4", CCSX_CHUNK0="16",
              CCSX_TIMING="1", CCSX_DEV_SHARE="8")
# one context and one worker (its chunks are cut into 1 x 3 batches): a
# difference from SPREAD's files is then one of concurrency, not of indexing
SINGLE = dict(SPREAD, CCSX_NGPU="1", CCSX_SLOTS="1")

_BATCH = re.compile(r"^\[ccsx\] chunk (\d+) batch of (\d+) ZMWs on context (\d+):", re.M)


def batch_lines(stderr) -> list:
    """[(chunk, ZMWs, context)] of a CCSX_TIMING run's per-batch lines."""
    if isinstance(stderr, bytes):
        stderr = stderr.decode(errors="replace")
    return [(int(c), int(n), int(w)) for c, n, w in _BATCH.findall(stderr)]


def spread(stderr) -> dict:
    """What assert_spread counts: chunks, the most batches of one chunk,
    contexts, the most batches of one context."""
    rows = batch_lines(stderr)
    per_chunk: dict = {}
    per_ctx: dict = {}
    for c, _, w in rows:
        per_chunk[c] = per_chunk.get(c, 0) + 1
        per_ctx[w] = per_ctx.get(w, 0) + 1
    return dict(chunks=len(per_chunk), chunk_batches=max(per_chunk.values(), default=0), contexts=len(per_ctx),
                ctx_batches=max(per_ctx.values(), default=0))


def assert_spread(stderr, single=False) -> None:
    """The run had at least 3 chunks, a chunk of at least 4 batches, at least 2
    contexts at work and a context that ran at least 3 batches (a pipelined
    worker keeps two in flight, so its third reuses a slot).  The first, second
    and last follow from the partition arithmetic above; which worker pops a
    batch is not fixed, but 20 or more batches over four workers cannot all go
    to one.  single: SINGLE's run instead, whose one context ran everything,
    three batches per chunk."""
    s = spread(stderr)
    assert s["chunks"] >= 3 and s["chunk_batches"] >= (3 if single else 4) and s["ctx_batches"] >= 3, s
    assert s["contexts"] == 1 if single else s["contexts"] >= 2, s
