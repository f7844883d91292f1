"""The device's band aligner (ccsx_align.hip through cx.Aligner) against the
oracle's pairwise aligner (oracle/prep_oracle.c) and, for the batched
ccs_prepare and the CLI's CCSX_GPU_STRAND=1, against the oracle's push lists
and consensus.  Every comparison is exact.  Where a band is placed by hand
(d0 given) the oracle, which always seeds, cannot be asked: the reference is
band_ref below, SPEC.md §8's cell rules restated in numpy, itself held to the
oracle at the seed's diagonal."""
import os
import random
import subprocess

import numpy as np
import pytest

import ccsx_amd as cx
from oracle import oracle as orc
from oracle.oracle import batch
from tools.gen_synth import write_subreads

from .test_prepare_resume import ZERO, family_reference, same_lists

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccsx_amd", "bin", "ccsx")


@pytest.fixture(scope="module")
def aligner():
    a = cx.Aligner(0)
    yield a
    a.close()


def band_ref(q: bytes, t: bytes, d0: int) -> dict:
    """SPEC.md §8 steps 2-3, cell for cell: rows in numpy, the in-row left chain
    as a running maximum of H(k) + 2k."""
    qa, ta = np.frombuffer(q, np.uint8).astype(np.int64), np.frombuffer(t, np.uint8).astype(np.int64)
    BW, lo = 513, d0 - 256
    ks = np.arange(BW)
    prev = np.zeros(BW + 1, np.int64)  # P(i-1, k), one zero beyond the band
    dirs = np.zeros((len(qa), BW), np.uint8)
    best, bi, bk = 0, -1, -1
    for i in range(len(qa)):
        j = i + lo + ks
        inside = (j >= 0) & (j < len(ta))
        tj = np.where(inside, ta[np.clip(j, 0, max(len(ta) - 1, 0))] if len(ta) else 0, 9)
        s = np.where((qa[i] < 4) & (tj == qa[i]), 1, -2)
        diag, up = prev[:BW] + s, prev[1:] - 2
        e = np.maximum(0, np.maximum(diag, up))
        d = np.where(diag > 0, 1, 0)
        d = np.where(up > np.maximum(diag, 0), 2, d)
        e, d = np.where(inside, e, 0), np.where(inside, d, 0)
        # H(k) = max(E(k), H(k-1) - 2); left wins only when strictly larger
        h = np.maximum.accumulate(e + 2 * ks) - 2 * ks
        left = np.concatenate([[0], h[:-1]]) - 2
        d = np.where(inside & (left > e), 3, d)
        h = np.where(inside, h, 0)
        dirs[i] = d
        m = int(h.max())
        if m > best:
            best, bi, bk = m, i, int(np.argmax(h))
        prev[:BW] = h
    r = dict(ZERO)
    if bi < 0:
        return r
    i, k = bi, bk
    r["qe"], r["te"], r["score"] = bi + 1, bi + lo + bk + 1, best
    while True:
        d = dirs[i, k]
        if d == 0:
            break
        j = i + lo + k
        if d == 1:
            r["mat" if qa[i] < 4 and qa[i] == ta[j] else "mis"] += 1
            r["qb"], r["tb"] = i, j
            i -= 1
        elif d == 2:
            r["ins"] += 1
            r["qb"] = i
            i, k = i - 1, k + 1
        else:
            r["del"] += 1
            r["tb"] = j
            k -= 1
        if i < 0 or k < 0 or k >= BW:
            break
    r["aln"] = r["mat"] + r["mis"] + r["ins"] + r["del"]
    return r


def noisy(rng, t, sub=0.04, dele=0.03, ins=0.05):
    q = np.array(t, dtype=np.uint8)
    m = rng.random(len(q))
    q[m < sub] = rng.integers(0, 4, int((m < sub).sum()))
    q = np.delete(q, np.where(rng.random(len(q)) < dele)[0])
    at = np.where(rng.random(len(q)) < ins)[0]
    return np.insert(q, at, rng.integers(0, 4, len(at))).astype(np.uint8)


def rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def tiling_pairs():
    """Lengths around the band's tiling (9 cells per lane, 64-row blocks, 513
    cells): every qlen x tlen of the set, the query a noisy copy of the
    target's head (or the target of the query's)."""
    rng = np.random.default_rng(1)
    sizes = (13, 14, 63, 64, 65, 511, 512, 513, 514, 1000)
    out = []
    for ql in sizes:
        for tl in sizes:
            base = rand(rng, max(ql, tl) + 100)
            q = noisy(rng, base)[:ql]
            out.append((q.tobytes(), base[:tl].tobytes()))
            assert len(out[-1][0]) == ql and len(out[-1][1]) == tl
    return out


def geometry_pairs():
    rng = np.random.default_rng(2)
    t = rand(rng, 1500)
    out = {}
    out["d0_negative"] = (np.concatenate([rand(rng, 400), noisy(rng, t[:700])]).tobytes(), t.tobytes())
    out["d0_near_tlen"] = (noisy(rng, t[1200:]).tobytes(), t.tobytes())
    out["q_longer"] = (np.concatenate([rand(rng, 300), noisy(rng, t), rand(rng, 500)]).tobytes(), t[200:1100].tobytes())
    q = noisy(rng, t, 0.01, 0.01, 0.01)
    out["deletion_300"] = (np.concatenate([q[:700], q[1000:]]).tobytes(), t.tobytes())
    out["insertion_300"] = (np.concatenate([q[:700], rand(rng, 300), q[700:]]).tobytes(), t.tobytes())
    return out


def tie_pairs():
    rng = np.random.default_rng(3)
    out = {}
    for name, unit in (("homopolymer", [2]), ("dinucleotide", [0, 3])):
        for run in (50, 61, 70):
            rep = np.array((unit * run)[:run], dtype=np.uint8)
            a, b = rand(rng, 300), rand(rng, 300)
            t = np.concatenate([a, rep, b])
            # the query's run is shorter and longer than the target's: gaps that may go anywhere in it
            for dl in (-7, 5):
                rq = np.array((unit * (run + dl))[:run + dl], dtype=np.uint8)
                out[f"{name}_{run}_{dl}"] = (np.concatenate([noisy(rng, a, 0.02, 0.01, 0.01), rq, b]).tobytes(), t.tobytes())
    # (diagonals 50 and 237, 0 and 200: both copies inside one band)
    src = rand(rng, 200)
    out["two_copies"] = (src[:150].tobytes(),
                         np.concatenate([rand(rng, 50), src[:150], rand(rng, 37), src[:150], rand(rng, 60)]).tobytes())
    out["two_copies_adjacent"] = (src.tobytes(), np.concatenate([src, src]).tobytes())
    t = rand(rng, 600)
    q = t.copy()
    q[rng.random(600) < 0.03] = 4
    out["n_in_q"] = (q.tobytes(), t.tobytes())
    t4 = t.copy()
    t4[rng.random(600) < 0.03] = 4
    out["n_in_t"] = (t.tobytes(), t4.tobytes())
    both = t.copy()
    both[100:140:3] = 4
    both[300:310] = 5
    out["n_aligned_to_n"] = (both.tobytes(), both.tobytes())
    return out


_MIX = {}


def mixed():
    """Every seeded case above in one shuffled list, with the oracle's answers."""
    if not _MIX:
        pairs = tiling_pairs() + list(geometry_pairs().values()) + list(tie_pairs().values())
        pairs += [(bytes(12), bytes(300)), (bytes(300), bytes(5)), (b"", bytes(40))]
        random.Random(4).shuffle(pairs)
        _MIX["pairs"], _MIX["ref"] = pairs, [orc.pairwise(q, t) for q, t in pairs]
    return _MIX["pairs"], _MIX["ref"]


def test_lengths_around_the_tiling(aligner):
    pairs = tiling_pairs()
    got = aligner.pairwise(pairs)
    hit = 0
    for (q, t), g in zip(pairs, got):
        assert g == orc.pairwise(q, t), (len(q), len(t))
        hit += g["score"] > 0
    assert hit >= 50  # (a 13- or 14-base side seldom shares an exact 13-mer with a noisy copy)


def test_short_pairs_and_no_jobs(aligner):
    assert aligner.band_align([]) == []
    assert aligner.pairwise([(bytes(12), bytes(300)), (bytes(300), bytes(12))]) == [ZERO, ZERO]
    # the band itself has no length floor: a job below 13 bases is plain DP
    rng = np.random.default_rng(5)
    t = rand(rng, 40).tobytes()
    jobs = [(t[5:14], t, 5), (t[:12], t[:12], 0), (b"", t, 0), (t, b"", 0), (t[3:4], t, 3)]
    assert aligner.band_align(jobs) == [band_ref(*j) for j in jobs]
    assert aligner.band_align(jobs)[0]["score"] == 9


@pytest.mark.parametrize("n", [20000, 34000])
def test_long_job(aligner, n):
    """20,000 x 20,000: the traceback crosses hundreds of record blocks.  At
    +1 per match its score cannot reach 2^15; the 34,000 x 34,000 job's does
    (34,000 - 3 x 150 substitutions), beyond a 16-bit score."""
    rng = np.random.default_rng(6)
    t = rand(rng, n)
    q = t.copy()
    at = rng.choice(n, 150, replace=False)
    q[at] = (q[at] + 1) % 4
    got = aligner.pairwise([(q.tobytes(), t.tobytes())])[0]
    assert got == orc.pairwise(q.tobytes(), t.tobytes())
    assert got["aln"] >= n - 1000 and got["score"] >= n - 3 * 150 - 1000
    if n == 34000:
        assert got["score"] > 1 << 15


@pytest.mark.parametrize("name", sorted(geometry_pairs()))
def test_band_geometry(aligner, name):
    q, t = geometry_pairs()[name]
    d0 = cx.pairwise_seed(q, t)
    got = aligner.pairwise([(q, t)])[0]
    assert got == orc.pairwise(q, t) and got["score"] > 100
    if name == "d0_negative":
        assert d0 < -300
    if name == "d0_near_tlen":
        assert d0 > len(t) - 400
    if name.endswith("_300"):
        # the path leaves the seeded band: the alignment stops at a band edge
        assert got["aln"] < 1100


def test_band_placed_by_hand(aligner):
    """d0 at +-1, +-255, +-256, +-257 from the seed's value: the path meets the
    band's edges k = 0 and k = 512, or lies outside the band."""
    rng = np.random.default_rng(7)
    t = rand(rng, 900)
    t = t.tobytes()
    for q in (noisy(rng, np.frombuffer(t, np.uint8)[100:700]).tobytes(),
              noisy(rng, np.frombuffer(t, np.uint8)[100:700], 0.03, 0, 0).tobytes()):
        d0 = cx.pairwise_seed(q, t)
        assert band_ref(q, t, d0) == orc.pairwise(q, t)  # the reference held to the oracle
        jobs = [(q, t, d0 + s * m) for m in (1, 255, 256, 257) for s in (1, -1)]
        got = aligner.band_align(jobs)
        for j, g in zip(jobs, got):
            assert g == band_ref(*j), j[2] - d0
        assert got[0]["aln"] > 500 and got[1]["aln"] > 500
    # the second query has no indels: its path is the diagonal 100 alone, which is
    # cell k = 0 of the band at d0 = 356, k = 512 at d0 = -156, and outside beyond
    jobs = [(q, t, 100 + s * m) for m in (256, 257) for s in (1, -1)]
    got = aligner.band_align(jobs)
    for j, g in zip(jobs, got):
        assert g == band_ref(*j), j[2]
    assert got[0]["aln"] > 500 and got[1]["aln"] > 500 and got[2]["aln"] < 50 and got[3]["aln"] < 50


@pytest.mark.parametrize("name", sorted(tie_pairs()))
def test_ties(aligner, name):
    q, t = tie_pairs()[name]
    got = aligner.pairwise([(q, t)])[0]
    assert got == orc.pairwise(q, t)
    assert got["score"] > 0
    if name == "two_copies":
        assert (got["tb"], got["te"], got["score"]) == (50, 200, 150)  # the first copy wins
    if name == "two_copies_adjacent":
        assert (got["tb"], got["te"], got["score"]) == (0, 200, 200)
    if name == "n_aligned_to_n":
        assert got["mis"] >= 10


def test_many_jobs_in_one_call(aligner):
    """3,000 jobs of 200-400 bases: more jobs than the grid has waves."""
    rng = np.random.default_rng(8)
    pairs = []
    for _ in range(3000):
        t = rand(rng, int(rng.integers(200, 401)))
        a = int(rng.integers(0, 60))
        pairs.append((noisy(rng, t[a:])[:400].tobytes(), t.tobytes()))
    before = aligner.stats()
    got = aligner.pairwise(pairs)
    for (q, t), g in zip(pairs, got):
        assert g == orc.pairwise(q, t)
    after = aligner.stats()
    assert after["slices"] - before["slices"] == 1 and after["host_jobs"] == before["host_jobs"]


def test_mixed_batch(aligner):
    pairs, ref = mixed()
    assert aligner.pairwise(pairs) == ref


def test_mixed_batch_in_small_slices():
    """The same mix with an arena of 400 KB: a 1,000-row job (256,000 bytes of
    records) fits alone, two do not, and the 20,000-row job runs on the host."""
    pairs, ref = mixed()
    rng = np.random.default_rng(9)
    t = rand(rng, 20000)
    big = (noisy(rng, t, 0.01, 0.01, 0.01)[:20000].tobytes(), t.tobytes())
    a = cx.Aligner(0, max_bytes=400_000)
    try:
        got = a.pairwise(pairs + [big])
        st = a.stats()
    finally:
        a.close()
    assert got[:-1] == ref and got[-1] == orc.pairwise(*big) and got[-1]["score"] > 10000
    assert st["slices"] >= 3 and st["host_jobs"] >= 1
    assert st["jobs"] == sum(1 for q, t in pairs + [big] if cx.pairwise_seed(q, t) is not None)


@pytest.mark.parametrize("nthreads", [1, 4])
def test_batched_prepare_matches_the_oracle(aligner, nthreads):
    zs, ref = family_reference()
    before = aligner.stats()
    got = aligner.prepare_segments(zs, nthreads=nthreads)
    same_lists(got, ref)
    st = aligner.stats()
    assert st["jobs"] > before["jobs"] and st["rounds"] - before["rounds"] >= 2
    assert aligner.info["rounds"] >= 2 and aligner.info["jobs"] == st["jobs"] - before["jobs"]


def _cli_zmws():
    zs, _ = family_reference()
    keep = [z for z in zs if sum(map(len, z)) >= 5000][:60]
    assert len(keep) >= 55
    return keep


def _cli(args, env):
    r = subprocess.run([BIN] + args, capture_output=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def test_cli_gpu_strand_matches_host_and_oracle(tmp_path):
    fa = str(tmp_path / "in.fa")
    write_subreads(fa, _cli_zmws())
    outs = {}
    for on in ("0", "1"):
        r = _cli(["-A", "-j", "4", fa, "/dev/stdout"], dict(CCSX_GPU_STRAND=on, CCSX_TIMING="1"))
        outs[on] = r.stdout
        assert (b"strand check:" in r.stderr) == (on == "1")
        assert b"CCSX_GPU_STRAND:" not in r.stderr  # (no fall-back warning)
    keep = []
    for movie, hole, subs in cx.read_zmws(fa):
        if len(subs) < 5 or not (5000 <= sum(map(len, subs)) <= 500000):
            continue
        keep.append((movie, hole, orc.prepare(subs)))
    ccs, _, _ = batch([p for _, _, p in keep], 0, 16)
    want = b"".join(b">%s/%s/ccs\n%s\n" % (m.encode(), h.encode(), c) for (m, h, _), c in zip(keep, ccs) if c)
    assert outs["1"] == outs["0"] == want and want.count(b">") >= 40


def test_cli_gpu_strand_side_outputs(tmp_path):
    """-q -r -a -s see the same push lists with the strand check on the device."""
    fa = str(tmp_path / "in.fa")
    write_subreads(fa, _cli_zmws())
    files = {}
    for on in ("0", "1"):
        names = [str(tmp_path / f"{k}{on}") for k in ("out", "rep", "paf", "site")]
        _cli(["-A", "-j", "4", "-q", "-r", names[1], "-a", names[2], "-s", names[3], fa, names[0]],
             dict(CCSX_GPU_STRAND=on))
        files[on] = [open(n, "rb").read() for n in names]
    assert files["1"] == files["0"]
    assert all(len(f) > 1000 for f in files["1"][:3])
