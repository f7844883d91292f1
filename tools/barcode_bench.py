"""The demultiplexer's cost next to the consensus launch it follows (DESIGN.md
§20): N config-E ZMWs (bench.py's shapes and holes) staged and launched once
(ccsx_gpu_launch's own time, HIP events), their CCS reads given a barcode at
either end, then scored by ccsx_gpu_bc_score `reps` times against a set of B
random 16-base barcodes (kernel_ms: the kernel of every slice, HIP events;
call_ms: the whole call with its window coding and copies), and by
ccsx_barcode_host on `threads` threads over the first `host-reads` reads.
Cells = reads x 2 ends x 2 B patterns x 16 x window; the VALU fraction counts 4
integer operations per cell (bit extract, multiply-add, max3, subtract) against
256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz.  Prints one JSON line; run it in fresh
processes and take the median.
Usage: barcode_bench.py [--zmws 16384] [--barcodes 96] [--window 96] [--reps 3] [--host-reads 2048] [--threads 16]"""
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
    ap.add_argument("--barcodes", type=int, default=96)
    ap.add_argument("--window", type=int, default=96)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reads", type=int, default=2048)
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
    barcodes = [bytes(rng.choice(b"ACGT") for _ in range(16)) for _ in range(a.barcodes)]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    reads = [barcodes[rng.randrange(a.barcodes)] + ccs + barcodes[rng.randrange(a.barcodes)][::-1].translate(rc)
             for ccs, status, _ in res if status == 0 and ccs]
    n = len(reads)
    arr = (nat.BcIn * max(n, 1))()
    for i, r in enumerate(reads):
        arr[i].ccs, arr[i].len = r, len(r)
    out = (nat.BcOut * max(n, 1))()
    ms = C.c_float(0)
    dm = cx.Demux(0)
    dm.set(barcodes, a.window)
    if L.ccsx_gpu_bc_score(dm._ctx, arr, min(n, 16), out, C.byref(ms)) != 0:  # warm-up: the code object, the stream
        raise SystemExit(L.ccsx_gpu_bc_error(dm._ctx).decode())
    kms, wall = [], []
    for _ in range(a.reps):
        before = dm.stats()
        t0 = time.perf_counter()
        if L.ccsx_gpu_bc_score(dm._ctx, arr, n, out, C.byref(ms)) != 0:
            raise SystemExit(L.ccsx_gpu_bc_error(dm._ctx).decode())
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(float(ms.value))
    slices = dm.stats()["slices"] - before["slices"]
    lens = [16] * a.barcodes
    assigned = sum(cx.barcode_call(nat._bc_ends(out[i]), lens, len(reads[i]))[3] for i in range(n))
    # the host restatement on the same reads (the first host-reads of them), one read per task
    seqs, offs, blen = nat._barcode_set(barcodes)
    nh = min(n, a.host_reads)
    hout = (nat.BcOut * max(nh, 1))()

    def one(i):
        L.ccsx_barcode_host(seqs, nat._p32(offs), nat._p32(blen), len(blen), a.window, reads[i], len(reads[i]), C.byref(hout[i]))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        list(ex.map(one, range(nh), chunksize=16))
    host_ms = (time.perf_counter() - t0) * 1e3
    same = all(bytes(hout[i]) == bytes(out[i]) for i in range(nh))
    cells_per_read = 2 * 2 * a.barcodes * 16 * sum(min(len(r), a.window) for r in reads) / max(n, 1)
    k = float(np.median(kms))
    cps = cells_per_read * n / (k / 1e3)
    print(json.dumps(dict(
        zmws=n, barcodes=a.barcodes, window=a.window, launch_ms=round(launch_ms, 1),
        bc_kernel_ms=[round(x, 2) for x in kms], bc_call_ms=[round(x, 1) for x in wall],
        kernel_ratio=round(k / launch_ms, 5), call_ratio=round(float(np.median(wall)) / launch_ms, 5),
        cells_per_read=round(cells_per_read), gcells_per_s=round(cps / 1e9, 1),
        valu_fraction=round(cps * OPS_PER_CELL / PEAK_INT32, 4), slices_per_call=slices, assigned=assigned,
        host_reads=nh, host_threads=a.threads, host_ms=round(host_ms, 1),
        host_gcells_per_s=round(cells_per_read * nh / host_ms / 1e6, 2),
        host_ms_per_read_over_call_ms_per_read=round((host_ms / max(nh, 1)) / (float(np.median(wall)) / max(n, 1)), 1),
        host_equals_device=same)), flush=True)
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
