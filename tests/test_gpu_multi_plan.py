"""accumulate_multi_kernel with its per-group plans (multi_plan_kernel, PlanSrc in kiwi_common.hpp) against the same kernel deriving every
group's parameters from the head records (KIWI_HIP_MULTI_PLAN=0) and against the one-source kernels (KIWI_HIP_DUO=0): synthetics, misfits
and global misfits, bit for bit under `exact`, within the contract's tolerances under `fused`.

The trial sources are centroid tables cut from discretised bilateral sources -- a few points with a few time steps each -- so that every
case is a handful of centroid groups of known length, on a database of 16 x 5 nodes with 1100 samples (two 512-sample tiles, five
256-sample tiles, the last one partial) and three receivers."""
import numpy as np
import pytest

from kiwi_amd import synthetic
from kiwi_amd.engine import discretize
from tests.common import Scenario, arith, misfit_close, multi_groups, same_bits

DT = 0.5                  # sample interval of the synthetic database
STEPS = 5                 # time steps per point of the discretised bilateral source below


def _table(params, steps, t_add=0.0):
    """Centroid table of bilateral `params` reduced to len(steps) points, point j keeping the time steps steps[j] (indices into its
    five, or (index, extra seconds) pairs), the whole source delayed by t_add seconds."""
    cent, mo, ri = discretize("bilateral", np.asarray(params, np.float32), 0.5)
    assert len(cent) % STEPS == 0 and len(cent) // STEPS >= len(steps)
    rows = []
    for j, ks in enumerate(steps):
        for k in ks:
            k, extra = k if isinstance(k, tuple) else (k, 0.0)
            row = cent[STEPS * j + k].copy()
            assert np.array_equal(row[:3], cent[STEPS * j][:3])              # the same point: one centroid group
            row[3] += np.float32(t_add + extra)
            rows.append(row)
    return np.array(rows, np.float32), mo


def _scenario(ng, comps_list, variant="probe"):
    sc = Scenario(nx=16, nz=5, ng=ng, L=1100, nrec=3, comps_list=comps_list, variant=variant)
    e = sc.oracle()
    sc.make_references(e)
    e.close()
    return sc


def _evaluate(sc, tables, moments, monkeypatch, capfd, plan, duo):
    """(synthetics of every source, receiver and component; misfits; norm factors; global misfits; groups of four; pairs) of one fresh
    engine: the synthetics from an evaluation that keeps them, the misfits from one that compares inside the kernel's epilogue."""
    monkeypatch.setenv("KIWI_HIP_MULTI_PLAN", "1" if plan else "0")
    monkeypatch.setenv("KIWI_HIP_DUO", "4" if duo else "0")
    monkeypatch.setenv("KIWI_HIP_POISON", "1")             # a plan, descriptor or coefficient line read but not written shows
    monkeypatch.setenv("KIWI_HIP_DEBUG", "1")
    capfd.readouterr()
    p = sc.product()
    sc.apply_setup(p, False)
    p.set_sources(tables, moments=moments)
    p.eval()
    m, n, g = [x.copy() for x in p.get_misfits()]
    p.set_keep_synthetics(1)
    p.eval()
    syn = [p.get_synthetics(s, ir, k, 1)[1].copy() for s in range(len(tables)) for ir in range(1, sc.nrec + 1)
           for k in range(1, len(sc.comps[ir - 1]) + 1)]
    p.close()
    taken = multi_groups(capfd.readouterr().err)
    n4 = max((t[1] for t in taken), default=0)
    n2 = max((t[2] for t in taken), default=0)
    return syn, m, n, g, n4, n2


def _check(sc, tables, moments, monkeypatch, capfd, want4, want2):
    a = _evaluate(sc, tables, moments, monkeypatch, capfd, plan=True, duo=True)
    b = _evaluate(sc, tables, moments, monkeypatch, capfd, plan=False, duo=True)
    c = _evaluate(sc, tables, moments, monkeypatch, capfd, plan=False, duo=False)
    assert (a[4], a[5]) == (want4, want2) and (b[4], b[5]) == (want4, want2) and (c[4], c[5]) == (0, 0)
    assert len(a[0]) == len(b[0]) == len(c[0]) == len(tables) * sum(len(x) for x in sc.comps)
    assert sum(1 for x in a[0] if np.any(x != 0)) >= len(a[0]) // 2
    for x, y, z in zip(a[0], b[0], c[0]):
        assert same_bits(x, y) and same_bits(x, z)
    assert np.all(np.isfinite(a[1])) and np.any(a[1] > 0)
    assert _close(a, b) and _close(a, c)
    assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()            # the references' norm factors: not the kernels' business


def _close(a, b):
    """misfits and global misfits of two evaluations: the same bits under `exact`, the contract's tolerances under `fused`"""
    if arith() == "exact":
        return a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()
    return misfit_close(a[1], b[1], a[2]) and misfit_close(a[3], b[3], glob=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_quads_and_pairs_together(monkeypatch, capfd, ng):
    """Ten sources 0.1 degrees apart in strike, 3 points x 2 time steps: two groups of four and one pair, so both plan kernels run
    and the pair launch consults the wider launch's flags; the second receiver has the vertical component only (multi_taken refuses
    it: no plan is written or read for it and the grouped kernel runs behind)."""
    sc = _scenario(ng, ["ned", "d", "ar"])
    tm = [_table(p, [[0, 1], [1, 2], [2, 3]]) for p in synthetic.bilat_strike_sweep(10, step=0.1)]
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, 2, 1)


@pytest.mark.gpu
def test_members_in_different_cells(monkeypatch, capfd):
    """Members in different cells of the Green's function grid.  The host groups neighbours only (ends within a quarter of the node
    spacing, 1000 m here), so the four sit astride a node line instead of a whole spacing apart: the first receiver is 104 km north of
    the origin, on the line between two cells; the first member's points lie 430 m or more short of it, the last two members' 180 m
    or more beyond.  Their rows differ: the tile sets are built one after the other from every member's own rows, offsets and tile
    origin."""
    sc = _scenario(10, ["ned", "ned", "ned"])
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    tm = []
    for north in (450.0, -100.0, -300.0, -500.0):
        q = base.copy()
        q[1] += north
        tm.append(_table(q, [[0, 1], [1, 2], [2, 3]]))
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("spread", ["halo", "beyond"])
def test_time_sweep(monkeypatch, capfd, spread):
    """Four sources in the same cells with origin times a few samples apart.  `halo`: the shifts of all four fit the tile's halo and
    the four tile sets share one origin, that of the largest shift.  `beyond`: every source's own two time steps are 45 samples
    apart, the four another 14 -- 256 + 59 + 8 positions do not fit the 320 of a tile set, so the sets are built one after the
    other although the rows are the same."""
    sc = _scenario(10, ["ned", "ned", "ned"])
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    delays = [0.0, 1.0, 2.5, 7.0]                           # seconds: 0, 2, 5 and 14 samples
    second = (1, 45 * DT) if spread == "beyond" else 1
    tm = [_table(base, [[0, second], [1, second], [2, 3]], t_add=d) for d in delays]
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, 1, 0)


@pytest.mark.gpu
def test_descriptor_rows_keep_the_record_path(monkeypatch, capfd):
    """A database with gaps and static end values has no compact descriptors: no plans are made and the kernel reads the head records
    and the 512-byte descriptor rows as before, whatever the switch says; a receiver with a missing component goes to the grouped
    kernel."""
    sc = _scenario(10, ["ned", "d", "ned"], variant="static")
    tm = [_table(p, [[0, 1], [1, 2], [2, 3]]) for p in synthetic.bilat_strike_sweep(6, step=0.1)]
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, 1, 1)


@pytest.mark.gpu
def test_variable_group_length(monkeypatch, capfd):
    """Groups of one and of five centroids in the same table, a group of one last (its plan is the last of the buffer: nothing is
    fetched behind it), in a group of four and a pair."""
    sc = _scenario(10, ["ned", "ned", "ned"])
    steps = [[2], [0, 1, 2, 3, 4], [1], [0, 1, 2, 3, 4], [3]]
    tm = [_table(p, steps) for p in synthetic.bilat_strike_sweep(6, step=0.1)]
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, 1, 1)
