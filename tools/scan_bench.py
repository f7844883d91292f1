"""The adapter scanner's cost next to the consensus launch it follows (DESIGN.md
§21): N config-E ZMWs (bench.py's shapes and holes) staged and launched once
(ccsx_gpu_launch's own time, HIP events), their CCS reads given `copies`
adapters each at random places and in random orientations, then scanned by
ccsx_gpu_scan `reps` times against a set of A random adapters of L bases
(kernel_ms: the kernel of every slice, HIP events; call_ms: the whole call with
its coding, copies and the host's finish), and by ccsx_scan_host on `threads`
threads over the first `host-reads` reads.  Cells = columns x 2 A patterns x L,
as §20 counts them; the warm-up columns of the tiles (WU before every tile but
a read's first) are counted apart, and the VALU fraction counts 4 integer
operations per cell of both, over the kernel's LR rows, against 256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz.  Prints one JSON line; run it in fresh processes
and take the median.
Usage: scan_bench.py [--zmws 16384] [--adapters 16] [--length 25] [--copies 8] [--reps 3] [--host-reads 256] [--threads 16]"""
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

PEAK_INT32 = 256 * 4 * 32 * 2.4e9
OPS_PER_CELL = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=16384)
    ap.add_argument("--adapters", type=int, default=16)
    ap.add_argument("--length", type=int, default=25)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reads", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    holes = list(range(E_LAUNCH_HOLE0, E_LAUNCH_HOLE0 + a.zmws))
    shapes = [zmw_shape(CONFIGS["E"], h) for h in holes]
    batch = nat.SynthBatch(SEED, holes, [s[0] for s in shapes], [s[1] for s in shapes], a.threads)
    L = cx.lib()
    eng = cx.Engine(0)
    eng.stage_batch(batch, cx.MODE_SHRED)
    launch_ms = eng.launch(cx.MODE_SHRED)
    res = eng.fetch()
    rng = random.Random(SEED)
    adapters = [bytes(rng.choice(b"ACGT") for _ in range(a.length)) for _ in range(a.adapters)]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for ccs, status, _ in res:
        if status or not ccs:
            continue
        r = bytearray(ccs)
        for _ in range(a.copies):
            ad = adapters[rng.randrange(a.adapters)]
            if rng.random() < .5:
                ad = ad[::-1].translate(rc)
            at = rng.randrange(0, max(len(r) - a.length, 1))
            r[at:at + a.length] = ad
        reads.append(bytes(r))
    n = len(reads)
    arr = (nat.BcIn * max(n, 1))()
    for i, r in enumerate(reads):
        arr[i].ccs, arr[i].len = r, len(r)
    hits, nhits, ms = C.POINTER(nat.ScanHit)(), C.c_uint64(0), C.c_float(0)
    sc = cx.Scanner(0)
    sc.set(adapters)

    def scan(m):
        if L.ccsx_gpu_scan(sc._ctx, arr, m, C.byref(hits), C.byref(nhits), C.byref(ms)) != 0:
            raise SystemExit(L.ccsx_gpu_scan_error(sc._ctx).decode())

    scan(min(n, 16))  # warm-up: the code object, the stream
    kms, wall = [], []
    for _ in range(a.reps):
        before = sc.stats()
        t0 = time.perf_counter()
        scan(n)
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(float(ms.value))
    after = sc.stats()
    dev = [(int(hits[k].read), int(hits[k].adapter), int(hits[k].orient), int(hits[k].start), int(hits[k].end), int(hits[k].score))
           for k in range(nhits.value)]
    # the host restatement on the first host-reads reads, one read per task
    nh = min(n, a.host_reads)

    def one(i):
        return [(i,) + h for h in cx.scan_host(adapters, reads[i])]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        host = [h for hs in ex.map(one, range(nh), chunksize=4) for h in hs]
    host_ms = (time.perf_counter() - t0) * 1e3
    same = host == [h for h in dev if h[0] < nh]
    rows = (a.length + 15) // 16 * 16
    tc, wu = cx.Scanner.tile(rows)
    cols = sum(len(r) for r in reads)
    warm = sum(sum(min(t0, wu) for t0 in range(tc, len(r) + 1, tc)) for r in reads)
    cells = cols * 2 * a.adapters * a.length
    k = float(np.median(kms))
    w = float(np.median(wall))
    print(json.dumps(dict(
        zmws=n, adapters=a.adapters, length=a.length, rows=rows, tc=tc, wu=wu, mean_read=round(cols / max(n, 1)),
        launch_ms=round(launch_ms, 1), scan_kernel_ms=[round(x, 2) for x in kms], scan_call_ms=[round(x, 1) for x in wall],
        kernel_ratio=round(k / launch_ms, 5), call_ratio=round(w / launch_ms, 5),
        gcells=round(cells / 1e9, 2), warmup_col_fraction=round(warm / max(cols, 1), 4),
        gcells_per_s=round(cells / (k / 1e3) / 1e9, 1),
        valu_fraction=round((cols + warm) * 2 * a.adapters * rows * OPS_PER_CELL / (k / 1e3) / PEAK_INT32, 4),
        slices_per_call=after["slices"] - before["slices"], reruns=after["reruns"], host_fallbacks=after["host_reads"],
        candidates_per_call=after["candidates"] - before["candidates"], hits=len(dev),
        host_reads=nh, host_threads=a.threads, host_ms=round(host_ms, 1),
        host_gcells_per_s=round(cells / max(n, 1) * nh / host_ms / 1e6, 2),
        host_ms_per_read_over_call_ms_per_read=round((host_ms / max(nh, 1)) / (w / max(n, 1)), 1),
        host_equals_device=same)), flush=True)
    sc.close()
    eng.close()


if __name__ == "__main__":
    main()
