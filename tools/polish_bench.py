"""The polisher's cost next to the consensus launch it follows:
N config-E ZMWs (bench.py's shapes and holes) staged and launched once with
the base map on (ccsx_gpu_launch's own time, HIP events), then their drafts,
segments and maps through ccsx_gpu_polish `reps` times (kernel_ms: the three
kernels of every slice, HIP events; call_ms: the whole call with its copies
and, for ZMWs that do not fit, the host).  Prints one JSON line; run it in
fresh processes and take the median.
Usage: polish_bench.py [--zmws 2048] [--reps 3] [--max-bytes 0] [--threads 16]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ccsx_amd as cx  # noqa: E402
import ccsx_amd.native as nat  # noqa: E402
from bench import CONFIGS, E_LAUNCH_HOLE0, SEED, zmw_shape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    holes = list(range(E_LAUNCH_HOLE0, E_LAUNCH_HOLE0 + a.zmws))
    shapes = [zmw_shape(CONFIGS["E"], h) for h in holes]
    batch = nat.SynthBatch(SEED, holes, [s[0] for s in shapes], [s[1] for s in shapes], a.threads)
    L = cx.lib()
    eng = cx.Engine(0)
    eng.set_base_map(True)
    eng.stage_batch(batch, cx.MODE_SHRED)
    launch_ms = eng.launch(cx.MODE_SHRED)
    res = eng.fetch()
    # the polisher's input: the batch's own bases, the engine's drafts and maps
    keep, arr, n = [], (nat.PolishIn * a.zmws)(), 0
    t0 = time.perf_counter()
    for i, (ccs, status, _) in enumerate(res):
        if status != 0 or not ccs:
            continue
        z = batch.zmws[i]
        m = np.concatenate([np.asarray(x) for x in eng.base_map(i)])
        keep += [ccs, m]
        arr[n].ccs, arr[n].len = ccs, len(ccs)
        arr[n].seqs = C.c_char_p(C.cast(C.byref(z), C.POINTER(C.c_void_p))[0])
        arr[n].seg_off, arr[n].seg_len, arr[n].nseg = z.seg_off, z.seg_len, z.nseg
        arr[n].map = nat._p32(m)
        n += 1
    gather_s = time.perf_counter() - t0
    pol = cx.Polisher(0, a.max_bytes)
    out = (nat.PolishOut * max(n, 1))()
    ms = C.c_float(0)
    if L.ccsx_gpu_polish(pol._ctx, arr, min(n, 16), out, C.byref(ms)) != 0:  # warm-up: the code object, the streams
        raise SystemExit(L.ccsx_gpu_polish_error(pol._ctx).decode())
    kms, wall = [], []
    for _ in range(a.reps):
        before = pol.stats()
        t0 = time.perf_counter()
        if L.ccsx_gpu_polish(pol._ctx, arr, n, out, C.byref(ms)) != 0:
            raise SystemExit(L.ccsx_gpu_polish_error(pol._ctx).decode())
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(float(ms.value))
    st = pol.stats()
    bases = sum(len(m) for m in keep[1::2])
    draft = sum(len(c) for c in keep[0::2])
    k = float(np.median(kms))
    print(json.dumps(dict(
        zmws=n, pushed_bases=bases, draft_bases=draft, launch_ms=round(launch_ms, 1),
        polish_kernel_ms=[round(x, 1) for x in kms], polish_call_ms=[round(x, 1) for x in wall],
        kernel_ratio=round(k / launch_ms, 4), gcups=round(64 * bases / k / 1e6, 1),
        slices_per_call=st["slices"] - before["slices"], host_zmws_per_call=st["host_zmws"] - before["host_zmws"],
        changed=dict(nsub=sum(out[i].nsub for i in range(n)), nins=sum(out[i].nins for i in range(n)),
                     ndel=sum(out[i].ndel for i in range(n))),
        map_gather_s=round(gather_s, 2))), flush=True)
    pol.close()
    eng.close()


if __name__ == "__main__":
    main()
