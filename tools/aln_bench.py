"""The band aligner's rate: N band jobs of one length through
cx.Aligner.band_align, the kernels timed with HIP events (inputs resident in
the arena), against ccsx_pairwise_band over the same jobs on host threads.
Prints one JSON line per length.
Usage: aln_bench.py [--jobs 4096] [--lengths 15000,2000] [--host-jobs 512] [--threads 16] [--reps 3]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ccsx_amd as cx  # noqa: E402


def make_jobs(n, length, seed=20261020):
    """n pairs of two passes of one insert: 10 % error between them."""
    rng = np.random.default_rng(seed + length)
    jobs = []
    for _ in range(n):
        t = rng.integers(0, 4, length).astype(np.uint8)
        q = t.copy()
        m = rng.random(length)
        q[m < 0.02] = rng.integers(0, 4, int((m < 0.02).sum()))
        q = np.delete(q, np.where(rng.random(len(q)) < 0.03)[0])
        at = np.where(rng.random(len(q)) < 0.05)[0]
        q = np.insert(q, at, rng.integers(0, 4, len(at))).astype(np.uint8)
        qb, tb = q.tobytes(), t.tobytes()
        d0 = cx.pairwise_seed(qb, tb)
        jobs.append((qb, tb, d0 if d0 is not None else 0))
    return jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--lengths", default="15000,2000")
    ap.add_argument("--host-jobs", type=int, default=512, help="jobs of the host leg (the first ones)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=0)
    a = ap.parse_args()
    aln = cx.Aligner(0, a.max_bytes)
    for length in (int(x) for x in a.lengths.split(",")):
        jobs = make_jobs(a.jobs, length)
        cells = sum(513 * len(q) for q, _, _ in jobs)
        aln.band_align(jobs[:64])  # warm-up: the arena's first allocation, the code object
        kms, wall = [], []
        for _ in range(a.reps):
            before = aln.stats()
            t0 = time.perf_counter()
            got = aln.band_align(jobs)
            wall.append((time.perf_counter() - t0) * 1e3)
            kms.append(aln.kernel_ms)
        st = aln.stats()
        nh = min(a.host_jobs, len(jobs))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as ex:
            host = list(ex.map(lambda j: cx.pairwise_band(*j), jobs[:nh]))
        host_s = time.perf_counter() - t0
        k = float(np.median(kms))
        print(json.dumps(dict(
            length=length, jobs=len(jobs), slices_per_call=st["slices"] - before["slices"],
            kernel_ms=[round(x, 2) for x in kms], call_ms=[round(x, 1) for x in wall],
            aln_per_s_kernel=round(len(jobs) / k * 1e3), gcups_kernel=round(cells / k / 1e6, 2),
            aln_per_s_call=round(len(jobs) / float(np.median(wall)) * 1e3),
            host_threads=a.threads, host_jobs=nh, host_aln_per_s=round(nh / host_s, 1),
            host_gcups=round(sum(513 * len(q) for q, _, _ in jobs[:nh]) / host_s / 1e9, 3),
            equal_to_host=got[:nh] == host)), flush=True)
    aln.close()


if __name__ == "__main__":
    main()
