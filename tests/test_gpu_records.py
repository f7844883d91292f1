"""Every kernel object against the oracle on the constructed case families of
tests/zmw_cases.py (ladder, block_edge, band, tie), MSA byte for MSA byte.

The tidy MSA is the only output that shows each read's own path through the
graph, i.e. what the traceback decided: a consensus vote over the reads
absorbs one read's wrong predecessor.  tests/test_record_cases.py states, from
the oracle's counters, which record classes, band edges and tie rules the
families reach; here each kernel object 0..5 is forced in turn and its
consensus codes and MSA bytes must equal Poa().poa(reads) case by case.  The
families also go through engine.run (CCS, cells, qualities, pass records), and
the far-row families through a far slot record capacity of one row (re-run
with full capacities).  Everything is integer-exact: no tolerance.
"""
import numpy as np
import pytest

import ccsx_amd as cx
from oracle.oracle import Poa, batch
from tests import pass_ref as pr
from tests import quality_ref as qr
from tests.test_gpu_bspoa import _reads, _run, bspoa  # noqa: F401  (the bspoa fixture: the path single_poa binds)
from tests.zmw_cases import RECORD_FAMILIES, raw, synth

pytestmark = pytest.mark.gpu
FAMILIES = list(RECORD_FAMILIES)
MODES = [cx.MODE_SHRED, cx.MODE_PRIMITIVE]
FAR_FAMILIES = ["ladder", "block_edge"]  # rows of more than four predecessors, predecessors beyond every ring

_cases: dict = {}
_want_msa: dict = {}
_want_run: dict = {}


def cases_of(family):
    if family not in _cases:
        _cases[family] = RECORD_FAMILIES[family]()
    return _cases[family]


def want_msa(family):
    """The oracle's (consensus codes, MSA) per case: computed once, shared."""
    if family not in _want_msa:
        p = Poa()
        _want_msa[family] = {name: p.poa(reads) for name, reads in cases_of(family).items()}
    return _want_msa[family]


def want_run(family, mode):
    """The family as prepared ZMWs and the oracle's (CCS, cells) of batch()."""
    if (family, mode) not in _want_run:
        zs = [raw(reads) for reads in cases_of(family).values()]
        ccs, cells, _ = batch(zs, mode, 8)
        _want_run[family, mode] = (zs, ccs, cells)
    return _want_run[family, mode]


@pytest.fixture
def rengine(engine):
    """The shared engine; every hook these tests set is restored afterwards."""
    try:
        yield engine
    finally:
        engine.set_kernel_cfg(-1)
        engine.set_tight_far(0)
        engine.set_quality(False)
        engine.set_pass_stats(False)


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    """Where two MSAs first differ: column, then row (row k + 1 = read k)."""
    if got.shape != want.shape:
        return f"MSA shape {got.shape}, oracle {want.shape}"
    col, row = np.argwhere(got != want)[0]
    who = f"read {row - 1}" if 1 <= row <= got.shape[1] - 4 else "consensus" if row == got.shape[1] - 3 else "filler"
    return f"first differing MSA column {col}, row {row} ({who}): {got[col, row]} != {want[col, row]}"


def test_single_poa_is_the_bspoa_path(rengine, bspoa):  # noqa: F811
    """Engine.single_poa returns what the bspoa-compatible API returns."""
    lib, g = bspoa
    reads = _reads(synth(1, 2000, 8))
    cns, msa = rengine.single_poa(reads)
    bcns, bmsa = _run(lib, g, reads)
    assert cns.dtype == np.uint8 and msa.dtype == np.uint8 and msa.shape[1] == len(reads) + 4
    assert np.array_equal(cns, bcns) and np.array_equal(msa, bmsa)
    wcns, wmsa = Poa().poa(reads)
    assert np.array_equal(cns, wcns) and np.array_equal(msa, wmsa)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("family", FAMILIES)
def test_msa_every_kernel_object(rengine, family, cfg):
    want = want_msa(family)
    rengine.set_kernel_cfg(cfg)
    bad = []
    for name, reads in cases_of(family).items():
        cns, msa = rengine.single_poa(reads)
        assert rengine.kernel_cfg() == cfg, f"{family}/{name}: forced object {cfg}, ran {rengine.kernel_cfg()}"
        wcns, wmsa = want[name]
        if not np.array_equal(msa, wmsa):
            bad.append(f"{family}/{name} object {cfg}: {first_difference(msa, wmsa)}")
        elif not np.array_equal(cns, wcns):
            bad.append(f"{family}/{name} object {cfg}: consensus codes differ at {np.argwhere(cns != wcns)[:1].tolist()}"
                       if len(cns) == len(wcns) else f"{family}/{name} object {cfg}: {len(cns)} consensus codes, oracle {len(wcns)}")
    assert not bad, f"{len(bad)} of {len(want)} cases differ from the oracle:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("cfg", [0, 3, 5])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
def test_run_family(rengine, family, mode, cfg):
    """One engine.run over the whole family with qualities and pass records
    on: CCS and cells equal batch(), the quality bytes tests/quality_ref.py,
    the pass records tests/pass_ref.py."""
    zs, wccs, wcells = want_run(family, mode)
    names = list(cases_of(family))
    rengine.set_kernel_cfg(cfg)
    rengine.set_quality(True)
    rengine.set_pass_stats(True)
    got = rengine.run(zs, mode)
    assert rengine.kernel_cfg() == cfg
    for i, z in enumerate(zs):
        ccs, status, cells = got[i]
        where = f"{family}/{names[i]} object {cfg} mode {mode}"
        assert status == 0 and ccs == wccs[i], f"{where}: CCS differs from the oracle"
        assert cells == wcells[i], f"{where}: {cells} cells, oracle {wcells[i]}"
        rccs, rqual, _ = qr.reference(z, mode)
        assert rccs == ccs and rengine.quality(i) == rqual, f"{where}: qualities differ from the reference"
        rccs, rrec, _ = pr.reference(z, mode)
        rec = rengine.pass_stats(i)
        assert rccs == ccs and rec.shape == (len(z.lens), 6) and np.array_equal(rec, rrec), \
            f"{where}: pass records differ from the reference"


@pytest.mark.parametrize("cfg", [0, 5])
@pytest.mark.parametrize("family", FAR_FAMILIES)
def test_far_rows_tight_capacity(rengine, family, cfg):
    """The far-row families with far slot records for one row only: the DPs
    that meet a second far row fail with kErrSpill, ccsx_gpu_run re-runs them
    with full capacities, and the results stay equal to the oracle's."""
    zs, wccs, wcells = want_run(family, cx.MODE_SHRED)
    names = list(cases_of(family))
    rengine.set_kernel_cfg(cfg)
    rengine.set_tight_far(1)
    before = rengine.rerun_count()
    got = rengine.run(zs, cx.MODE_SHRED)
    assert rengine.rerun_count() - before >= 1
    for i in range(len(zs)):
        ccs, status, cells = got[i]
        assert status == 0 and ccs == wccs[i] and cells == wcells[i], f"{family}/{names[i]} object {cfg}"
