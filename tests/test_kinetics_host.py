"""Per-base consensus kinetics, CPU side (SPEC.md §13): the codec, the
definition's invariant on every edge case in both modes, a planted signal
through the reference and through ccsx_prepare_apply_kin, the BAM aux parser and
the SAM tag formatter.  No GPU."""
import numpy as np
import pytest

import ccsx_amd as cx

from . import kinetics_ref as kr
from . import pileup_ref as pu
from .kinetics_cases import PLANT, alternating, aux_array, names, planted_pw, rand_seqs, tagged_records, with_kin, write_bam
from .zmw_cases import edge_cases, raw

MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def test_codec_roundtrip_and_order():
    fr = [cx.kin_frames(b) for b in range(256)]
    assert fr == [int(x) for x in kr.FRAMES]
    assert all(b > a for a, b in zip(fr, fr[1:]))
    assert [fr[0], fr[63], fr[64], fr[127], fr[128], fr[191], fr[192], fr[255]] == [0, 63, 64, 190, 192, 444, 448, 952]
    assert [cx.kin_code(f) for f in fr] == list(range(256))


def test_code_against_table():
    """code(f) for f in 0..1000 against a table built here: the nearest frames
    value, the lower byte on a tie, everything above 952 at 255."""
    fr = [((b & 63) << (b >> 6)) + (64 << (b >> 6)) - 64 for b in range(256)]
    for f in range(1001):
        g = min(f, 952)
        best = min(range(256), key=lambda b: (abs(fr[b] - g), b))
        assert cx.kin_code(f) == best == kr.code(f), f
    assert cx.kin_code(191) == 127 and cx.kin_code(446) == 191 and cx.kin_code(447) == 192
    assert cx.kin_code(2 ** 32 - 1) == 255


@pytest.mark.parametrize("mode", MODES)
def test_invariant_on_edge_cases(mode):
    """fwd n + rev n = the reads that carry the CCS base (SPEC.md §9's match,
    counted independently by the pileup reference) wherever nothing saturates."""
    cases = edge_cases()
    for name in sorted(cases):
        z0 = cases[name]
        z = with_kin(z0, alternating(len(z0.lens)), seed=len(name))
        ccs, recs, n, match = kr.reference(z, mode)
        assert recs.shape == (len(ccs), 8) and not recs[:, 6:].any()
        pccs, prec, *_ = pu.reference(z, mode)
        assert pccs == ccs
        r = prec.astype(np.int64)
        own = (r[:, :4] + r[:, 6:10])[np.arange(len(ccs)), [b"ACGT".index(b) for b in ccs]] if len(ccs) else np.zeros(0)
        ok = ~(prec == 255).any(1) & (recs[:, 2] < 255) & (recs[:, 5] < 255)
        assert (n.sum(1) == match).all()
        assert ((recs[:, 2].astype(np.int64) + recs[:, 5]) == own)[ok].all(), name
        # a strand without reads in the column holds 0, 0, 0
        assert not recs[recs[:, 2] == 0][:, :2].any() and not recs[recs[:, 5] == 0][:, 3:5].any()


def test_planted_signal_saturated():
    """300 identical reads: every base carries a pw fixed by its letter, so every
    record shows its CCS base's value; n saturates at 255, the mean uses 300."""
    rng = np.random.default_rng(3)
    ins = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))
    z = raw([ins] * 300)
    ipd = bytes(int(x) for x in rng.integers(0, 256, len(z.seqs)))
    z = cx.Prepared(z.seqs, z.offs, z.lens, None, ipd, planted_pw(z.seqs))
    ccs, recs, n, _ = kr.reference(z, cx.MODE_PRIMITIVE)
    assert ccs == ins
    assert (recs[:, 2] == 255).all() and (n[:, 0] == 300).all() and not recs[:, 3:].any()
    assert recs[:, 1].tolist() == [PLANT[b] for b in ccs]
    # the ipd mean over all 300 reads, not over 255
    col = np.frombuffer(ipd, np.uint8).reshape(300, 150)
    want = [kr.code((int(kr.FRAMES[col[:, j]].sum()) + 150) // 300) for j in range(150)]
    assert recs[:, 0].tolist() == want


def test_planted_signal_through_prepare_apply_kin():
    """Subreads of alternating strands with pw planted by the subread's own
    letter: after ccsx_prepare_apply_kin a reverse segment's pushed base X
    carries the value of its complement, at the mirrored index."""
    subs, _ = cx.synth_zmw(20201104, 9100, 1200, 7)
    ipd = [bytes((7 * j + k) & 255 for j in range(len(s))) for k, s in enumerate(subs)]
    z = cx.prepare(subs, ipd, [planted_pw(s) for s in subs])
    z0 = cx.prepare(subs)
    assert z.seqs == z0.seqs and z.offs.tolist() == z0.offs.tolist() and z.rev.tolist() == z0.rev.tolist()
    assert z.rev.any() and not z.rev.all()
    cat_i = b"".join(ipd)
    for k in range(len(z.lens)):
        o, ln = int(z.offs[k]), int(z.lens[k])
        seg, pw, ip = z.seqs[o:o + ln], z.pw[o:o + ln], z.ipd[o:o + ln]
        if z.rev[k]:
            assert pw == bytes(PLANT[COMP[c]] for c in seg)
            assert ip == cat_i[o:o + ln][::-1]
        else:
            assert pw == planted_pw(seg) and ip == cat_i[o:o + ln]
    ccs, recs, n, _ = kr.reference(z, cx.MODE_SHRED)
    f, r = recs[:, 2] > 0, recs[:, 5] > 0
    assert f.sum() > len(ccs) // 2 and r.sum() > len(ccs) // 2
    want_f = np.array([PLANT[b] for b in ccs], np.uint8)
    want_r = np.array([PLANT[COMP[b]] for b in ccs], np.uint8)
    assert (recs[:, 1] == want_f)[f].all() and (recs[:, 4] == want_r)[r].all()


def test_bam_parsing(tmp_path):
    rng = np.random.default_rng(11)
    lens = [301, 17, 256]
    recs = []
    want = {}
    # hole 1: B:C; hole 2: B:S with frames above 952
    for hole, sub in ((1, b"C"), (2, b"S")):
        r, w = tagged_records(list(zip(names(hole, lens), rand_seqs(rng, lens))), seed=hole, sub=sub)
        recs += r
        want[str(hole)] = w
    # hole 3: the second subread has no pw; hole 4: a wrong count; hole 5: an aux
    # field cut short (its count runs past the record); hole 6: B:C again (the
    # reader goes on reading after the bad records)
    s3 = rand_seqs(rng, lens)
    r3, _ = tagged_records(list(zip(names(3, lens), s3)), seed=3)
    r3[1] = (r3[1][0], r3[1][1], aux_array(b"ip", b"C", [1] * lens[1]))
    recs += r3
    s4 = rand_seqs(rng, lens)
    r4, _ = tagged_records(list(zip(names(4, lens), s4)), seed=4)
    r4[2] = (r4[2][0], r4[2][1], aux_array(b"ip", b"C", [1] * lens[2]) + aux_array(b"pw", b"C", [2] * (lens[2] - 1)))
    recs += r4
    s5 = rand_seqs(rng, lens)
    r5, _ = tagged_records(list(zip(names(5, lens), s5)), seed=5)
    r5[0] = (r5[0][0], r5[0][1], aux_array(b"ip", b"C", [1] * lens[0]) + aux_array(b"pw", b"C", [2] * 40, count=lens[0]))
    recs += r5
    r6, w6 = tagged_records(list(zip(names(6, lens), rand_seqs(rng, lens))), seed=6)
    recs += r6
    want["6"] = w6
    bam = str(tmp_path / "k.bam")
    write_bam(bam, recs)
    got = {hole: (subs, ipd, pw) for _, hole, subs, ipd, pw in cx.read_zmws(bam, True, kinetics=True)}
    assert sorted(got) == ["1", "2", "3", "4", "5", "6"]
    assert [s for _, _, s in cx.read_zmws(bam, True)] == [got[h][0] for h in sorted(got)]
    for h in ("1", "2", "6"):
        subs, ipd, pw = got[h]
        assert [len(s) for s in subs] == lens
        assert ipd == [w[0] for w in want[h]] and pw == [w[1] for w in want[h]], h
    assert max(got["2"][1][0]) == 255  # (frames above 952 encode as 255)
    for h in ("3", "4", "5"):
        assert got[h][1] is None and got[h][2] is None, h
        assert [len(s) for s in got[h][0]] == lens


def test_tag_formatting():
    rng = np.random.default_rng(2)
    recs = rng.integers(0, 256, (37, 8), dtype=np.uint8)
    recs[:, 6:] = 0
    assert cx.kinetics_tags(recs) == kr.tags(recs)
    t = cx.kinetics_tags(recs).split("\t")
    assert [x[:6] for x in t] == ["fi:B:C", "fp:B:C", "ri:B:C", "rp:B:C"]
    assert t[2].split(",")[1:] == [str(int(x)) for x in recs[::-1, 3]]
    # a ZMW with rn = 0: the reverse arrays are all zero, still len values
    recs[:, 3:6] = 0
    t = cx.kinetics_tags(recs).split("\t")
    assert t[2] == "ri:B:C" + ",0" * 37 and t[3] == "rp:B:C" + ",0" * 37
    assert cx.kinetics_tags(np.zeros((0, 8), np.uint8)) == "fi:B:C\tfp:B:C\tri:B:C\trp:B:C"
