"""Every kernel object against the oracle on shred_cases() of
tests/zmw_cases.py: the shredding loop around the POA call (zmw_body,
find_breakpoint, bp_ok, emit and pass_stats of ccsx_kernel.hip against
ocsx_zmw_log, main.c:541-641).

A wrong cursor or breakpoint changes which bases the next window holds, so it
shows in the CCS; the breakpoint log names the round.  tests/test_shred_cases.py
states, from the oracle's counters, which classes the family reaches -- every
ballot step and lane edge of the scan, the four thresholds of bp_ok at and
around equality, cursor advances that differ between reads and across the
64-read mask words, emission and pass-record chunk edges -- and that each single
wrong rule changes the result of a named case.  Here each kernel object 0..5 is
forced in turn; CCS, cells, breakpoint log, quality bytes and pass records must
equal the oracle's and the references' case by case, through ccsx_gpu_run,
submit / collect on both slots, stage / launch twice / fetch, forced full-caps
re-runs, and on the HBM-read instance, whose cursors live in the workspace.
Everything is integer-exact: no tolerance.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import batch
from tests import pass_ref as pr
from tests import quality_ref as qr
from tests.zmw_cases import hbm_cursor_zmw, raw, shred_cases, synth

pytestmark = pytest.mark.gpu

# cases whose pushed windows and graphs stay within the tight caps (no re-run):
# the ones stage / launch / fetch, which never re-runs, can take
STAGED = ("copies_3001", "copies_14000", "zone_34", "depth_64", "depth_128", "i_mod64_0", "col_n10_c7", "rows_at_i",
          "nogwin_6", "indel", "n65")

# cases that push a read above the 4,096-base tight read cap (push_gt4096 of tests/test_shred_cases.py)
OVER_READ_CAP = ("two_reads", "empty_segment", "ragged_1001", "prefix_6", "prefix_7", "prefix_10", "prefix_20",
                 "prefix_10_read2_from_5", "dirty_2000_then_shared", "dirty_5100", "dirty_7100")

_family: dict = {}
_hbm: dict = {}


def _references(zs):
    """Per ZMW (ccs, cells, log, quality bytes, pass records), the references
    computed side by side (the oracle library releases the GIL).  quality_ref
    and pass_ref assert their CCS and log against Poa().zmw_breakpoints: the
    log returned here is the oracle's."""
    with ThreadPoolExecutor(8) as ex:
        fb = ex.submit(batch, zs, cx.MODE_SHRED, 4)
        q = list(ex.map(lambda z: qr.reference(z, cx.MODE_SHRED), zs))
        p = list(ex.map(lambda z: pr.reference(z, cx.MODE_SHRED), zs))
        ccs, cells, _ = fb.result()
    for i in range(len(zs)):
        assert q[i][0] == ccs[i] and p[i][0] == ccs[i] and q[i][2] == p[i][2]
    return [(ccs[i], cells[i], q[i][2], q[i][1], p[i][1]) for i in range(len(zs))]


def family():
    """(names, prepared ZMWs, references) of the whole family: computed once, shared."""
    if not _family:
        cases = shred_cases()
        _family["names"] = list(cases)
        _family["zs"] = [raw(r) for r in cases.values()]
        _family["want"] = _references(_family["zs"])
    return _family["names"], _family["zs"], _family["want"]


@pytest.fixture
def sengine(engine):
    """The shared engine; every hook these tests set is restored afterwards."""
    try:
        yield engine
    finally:
        engine.set_kernel_cfg(-1)
        engine.set_tight_rows(0)
        engine.set_bp_log(False)
        engine.set_quality(False)
        engine.set_pass_stats(False)


def _first_round(got, want) -> str:
    for r, (g, w) in enumerate(zip(got, want)):
        if tuple(g) != tuple(w):
            return f"round {r}: (breakpoint, columns) {tuple(g)}, oracle {tuple(w)}"
    return f"{len(got)} rounds, oracle {len(want)}"


def _compare(eng, got, names, zs, want, where, slot=-1, log=True):
    bad = []
    for i, z in enumerate(zs):
        ccs, status, cells = got[i]
        wccs, wcells, wlog, wqual, wrec = want[i]
        at = f"{names[i]} {where}"
        if status != 0:
            bad.append(f"{at}: status {status}")
            continue
        if log:
            glog = [tuple(x) for x in eng.bp_log(i)]
            if glog != wlog:
                bad.append(f"{at}: breakpoint log differs at {_first_round(glog, wlog)}")
                continue
        if ccs != wccs:
            bad.append(f"{at}: CCS differs from the oracle ({len(ccs)} bases, oracle {len(wccs)})")
        elif cells != wcells:
            bad.append(f"{at}: {cells} cells, oracle {wcells}")
        elif eng.quality(i, slot) != wqual:
            bad.append(f"{at}: quality bytes differ from the reference")
        else:
            rec = eng.pass_stats(i, slot)
            if rec.shape != (len(z.lens), 6) or not np.array_equal(rec, wrec):
                bad.append(f"{at}: pass records differ from the reference")
    assert not bad, f"{len(bad)} of {len(zs)} cases differ:\n" + "\n".join(bad[:20])


def _on(eng, cfg):
    eng.set_kernel_cfg(cfg)
    eng.set_bp_log(True)
    eng.set_quality(True)
    eng.set_pass_stats(True)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_every_kernel_object(sengine, cfg):
    """One ccsx_gpu_run over the whole family per forced object; the cases that
    push a window above the 4,096-base tight read cap are re-run with full caps."""
    names, zs, want = family()
    _on(sengine, cfg)
    before = sengine.rerun_count()
    got = sengine.run(zs, cx.MODE_SHRED)
    assert sengine.kernel_cfg() == cfg
    _compare(sengine, got, names, zs, want, f"object {cfg}")
    assert sengine.rerun_count() - before >= len(OVER_READ_CAP) and not set(OVER_READ_CAP) - set(names)


@pytest.mark.parametrize("cfg", [0, 5])
def test_submit_collect_and_relaunch(sengine, cfg):
    """The family through submit / collect, its halves on the two slots side by
    side and then swapped; then a staged slice launched twice: cursors and pass
    records start from zero each launch."""
    names, zs, want = family()
    _on(sengine, cfg)
    halves = [list(range(0, len(zs), 2)), list(range(1, len(zs), 2))]
    for order in (halves, halves[::-1]):
        slots = [sengine.submit([zs[i] for i in idx], cx.MODE_SHRED) for idx in order]
        assert sorted(slots) == [0, 1]
        for idx, s in zip(order, slots):
            got = sengine.collect(s)
            _compare(sengine, got, [names[i] for i in idx], [zs[i] for i in idx], [want[i] for i in idx],
                     f"object {cfg} submit slot {s}", slot=s, log=False)
    idx = [names.index(n) for n in STAGED]
    sub = [zs[i] for i in idx]
    sengine.stage(sub, cx.MODE_SHRED)
    sengine.launch(cx.MODE_SHRED)
    sengine.launch(cx.MODE_SHRED)
    got = sengine.fetch()
    assert sengine.kernel_cfg() == cfg
    _compare(sengine, got, list(STAGED), sub, [want[i] for i in idx], f"object {cfg} launched twice", log=False)


@pytest.mark.parametrize("cfg", [0, 5])
def test_forced_reruns(sengine, cfg):
    """A tight row cap of 600: every case's first window outgrows it, so every
    ZMW fails its tight caps mid-loop and is re-run with full caps."""
    names, zs, want = family()
    _on(sengine, cfg)
    sengine.set_tight_rows(600)
    before = sengine.rerun_count()
    got = sengine.run(zs, cx.MODE_SHRED)
    assert sengine.rerun_count() - before == len(zs)
    _compare(sengine, got, names, zs, want, f"object {cfg} re-run")


def hbm_case():
    if not _hbm:
        _hbm["zs"] = [synth(8900, 2500, 6), raw(hbm_cursor_zmw()), raw(shred_cases()["copies_3001"])]
        _hbm["want"] = _references(_hbm["zs"])
    return ["synth", "hbm_cursor_zmw", "copies_3001"], _hbm["zs"], _hbm["want"]


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_hbm_instance_cursors(sengine, cfg):
    """Segments above the LDS read buffer's 100,000 bases whose third window
    (6,000 bases) exceeds the tight read cap: re-run with full caps on the
    HBM-read instance, where the cursors live in the workspace and advance over
    more than 50 rounds.  (The int16 objects 4 and 5 have no HBM instance.)"""
    names, zs, want = hbm_case()
    assert len(want[1][2]) > 50 and want[1][2][0][1] > 6000
    _on(sengine, cfg)
    reruns, hbm = sengine.rerun_count(), sengine.hbm_launches()
    got = sengine.run(zs, cx.MODE_SHRED)
    assert sengine.rerun_count() - reruns == 1 and sengine.hbm_launches() - hbm == 1
    assert sengine.kernel_cfg() == cfg
    _compare(sengine, got, names, zs, want, f"object {cfg} HBM-read instance")
