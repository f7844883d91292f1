"""The reference mapper's cost next to the consensus launch it follows (DESIGN.md
§22): N config-E ZMWs (bench.py's shapes and holes) staged and launched once
(ccsx_gpu_launch's own time, HIP events).  The panel is cut from their CCS
reads: target g is the first `tlen` bases of read g N / G.  A reference set
holds at most 2^20 letters, about 70 whole config-E reads, so every read is
given `stretch` bases of a random target at a random place in a random
orientation: every read then maps, and its band runs over all its bases, as a
read of an amplicon panel's would.  The reads are mapped by ccsx_gpu_ref_map
`reps` times (vote_ms / band_ms: the two kernels of every slice, HIP events;
call_ms: the whole call with its coding, copies and slices), and by
ccsx_ref_host on `threads` threads over the first `host-reads` reads.  Prints
one JSON line; run it in fresh processes and take the median.
Usage: refmap_bench.py [--zmws 16384] [--targets 64] [--tlen 4096] [--stretch 1000] [--reps 3] [--host-reads 64] [--threads 16]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ccsx_amd as cx  # noqa: E402
import ccsx_amd.native as nat  # noqa: E402
from bench import CONFIGS, E_LAUNCH_HOLE0, SEED, zmw_shape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--tlen", type=int, default=4096)
    ap.add_argument("--stretch", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reads", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    holes = list(range(E_LAUNCH_HOLE0, E_LAUNCH_HOLE0 + a.zmws))
    shapes = [zmw_shape(CONFIGS["E"], h) for h in holes]
    batch = nat.SynthBatch(SEED, holes, [s[0] for s in shapes], [s[1] for s in shapes], a.threads)
    eng = cx.Engine(0)
    eng.stage_batch(batch, cx.MODE_SHRED)
    launch_ms = eng.launch(cx.MODE_SHRED)
    ccs = [c for c, status, _ in eng.fetch() if status == 0 and c]
    rng = random.Random(SEED)
    G = min(a.targets, len(ccs))
    panel = [ccs[g * len(ccs) // G][:a.tlen] for g in range(G)]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for c in ccs:
        t = panel[rng.randrange(G)]
        b = rng.randrange(max(len(t) - a.stretch, 1))
        s = t[b:b + a.stretch]
        if rng.random() < .5:
            s = s[::-1].translate(rc)
        r = bytearray(c)
        at = rng.randrange(max(len(r) - len(s), 1))
        r[at:at + len(s)] = s
        reads.append(bytes(r[:len(c)]))
    n = len(reads)
    m = cx.RefMapper(0)
    m.set(panel)
    m.map(reads[:16], words=False)  # warm-up: the code objects, the stream
    # the C call itself, into buffers made once (the binding's per-read arrays are not the mapper's cost)
    L = cx.lib()
    arr = (nat.BcIn * max(n, 1))()
    for i, r in enumerate(reads):
        arr[i].ccs, arr[i].len = r, len(r)
    recs = (nat.RefRec * max(n, 1))()
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    words = np.zeros(max(int(offs[-1]), 1), np.uint32)
    ms = (C.c_float * 2)()
    vote, band, wall = [], [], []
    for _ in range(a.reps):
        before = m.stats()
        t0 = time.perf_counter()
        if L.ccsx_gpu_ref_map(m._ctx, arr, n, recs, words.ctypes.data, ms) != 0:
            raise SystemExit(L.ccsx_gpu_ref_error(m._ctx).decode())
        wall.append((time.perf_counter() - t0) * 1e3)
        vote.append(float(ms[0])), band.append(float(ms[1]))
    after = m.stats()
    got = [(tuple(int(x) for x in recs[i].v), words[offs[i]:offs[i + 1]]) for i in range(min(n, a.host_reads))]
    nh = min(n, a.host_reads)
    rs = cx.RefSet(panel)

    def one(i):
        return cx.ref_host(rs, reads[i])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        host = list(ex.map(one, range(nh)))
    host_ms = (time.perf_counter() - t0) * 1e3
    same = all(h[0] == g[0] and np.array_equal(h[1], g[1]) for h, g in zip(host, got))
    bases = sum(len(r) for r in reads)
    v, bnd, w = float(np.median(vote)), float(np.median(band)), float(np.median(wall))
    print(json.dumps(dict(
        zmws=n, targets=G, panel_letters=sum(len(t) for t in panel), stretch=a.stretch, mean_read=round(bases / max(n, 1)),
        launch_ms=round(launch_ms, 1), vote_kernel_ms=[round(x, 2) for x in vote], band_kernel_ms=[round(x, 2) for x in band],
        map_call_ms=[round(x, 1) for x in wall],
        vote_ratio=round(v / launch_ms, 5), band_ratio=round(bnd / launch_ms, 5), call_ratio=round(w / launch_ms, 5),
        band_gcups=round(bases * 513 / (bnd / 1e3) / 1e9, 1), band_alignments_per_s=round(n / (bnd / 1e3)),
        vote_mbases_per_s=round(bases / (v / 1e3) / 1e6, 1),
        slices_per_call=after["slices"] - before["slices"], mapped_per_call=after["mapped"] - before["mapped"],
        overflows=after["overflows"], host_fallbacks=after["host_reads"],
        host_reads=nh, host_threads=a.threads, host_ms=round(host_ms, 1),
        host_ms_per_read_over_call_ms_per_read=round((host_ms / max(nh, 1)) / (w / max(n, 1)), 1),
        host_equals_device=same)), flush=True)
    m.close()
    eng.close()


if __name__ == "__main__":
    main()
