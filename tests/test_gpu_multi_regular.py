"""accumulate_multi_kernel applying the centroid groups its plans call REGULAR (every integer shift its predecessor's + 1: PlanSrc::head,
kiwi_common.hpp) with the routines made for them (apply_regular_asm_*) against the same binary with the bit never set
(KIWI_HIP_MULTI_REGULAR=0: every group takes the general routine) and against the one-source kernels (KIWI_HIP_DUO=0): synthetics,
misfits and global misfits, bit for bit under `exact`, within the contract's tolerances under `fused`.

Scenario and tables as tests/test_gpu_multi_plan.py: a database of 16 x 5 nodes with 1100 samples, three receivers, centroid tables cut
from discretised bilateral sources.  The number of regular plans the library reports (KIWI_HIP_DEBUG) is compared with the number the
test derives from its own tables: a plan per (source of a group of four or a pair, centroid group, receiver), regular where the
group's floor(time / dt) grow by one."""
import re

import numpy as np
import pytest

from kiwi_amd import synthetic
from tests.common import same_bits
from kiwi_amd.engine import discretize
from tests.test_gpu_multi_plan import DT, STEPS, _close, _scenario

NREC = 3


def _table(params, steps, t_add=0.0):
    """Centroid table of bilateral `params` reduced to len(steps) points, as tests/test_gpu_multi_plan.py's, with the time steps ON THE
    SAMPLE GRID: step k (an index into the point's five, or (index, extra seconds)) of a point keeps its moment share and gets the time
    of the point's first step moved to a quarter sample behind a sample + k DT -- its integer shift is the first one's + k.  (The
    discretisation's own steps are 0.4 samples short of DT apart: two of five repeat a shift.)"""
    cent, mo, ri = discretize("bilateral", np.asarray(params, np.float32), 0.5)
    assert len(cent) % STEPS == 0 and len(cent) // STEPS >= len(steps)
    rows = []
    for j, ks in enumerate(steps):
        t0 = (np.floor(cent[STEPS * j][3] / DT) + 0.25) * DT
        for k in ks:
            k, extra = k if isinstance(k, tuple) else (k, 0.0)
            row = cent[STEPS * j + k].copy()
            assert np.array_equal(row[:3], cent[STEPS * j][:3])              # the same point: one centroid group
            row[3] = np.float32(t0 + k * DT + t_add + extra)
            rows.append(row)
    return np.array(rows, np.float32), mo


def _groups(table):
    """[integer shifts of a centroid group] of one table: runs of centroids at the same point (the library's rule, restated for tables
    whose groups stay far below its limits of length and of shift spread)"""
    out, point = [], None
    for row in table:
        sh = int(np.floor(np.float32(row[3]) / np.float32(DT)))
        if point is not None and np.array_equal(row[:3], point):
            out[-1].append(sh)
        else:
            out.append([sh])
            point = row[:3]
    assert all(max(g) - min(g) <= 50 and len(g) <= 8 for g in out)
    return out


def _expected(tables, multi_sources):
    """(plans, regular plans) of the sources accumulate_multi_kernel takes, all NREC receivers"""
    plans = regular = 0
    for s in multi_sources:
        for g in _groups(tables[s]):
            plans += NREC
            regular += NREC * int(all(b == a + 1 for a, b in zip(g, g[1:])))
    return plans, regular


def _evaluate(sc, tables, moments, monkeypatch, capfd, regular, duo):
    monkeypatch.setenv("KIWI_HIP_MULTI_REGULAR", "1" if regular else "0")
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
    counts = [(int(a), int(b)) for a, b in re.findall(r"multi plans: (\d+) of a \(source, centroid group, receiver\), (\d+) regular", capfd.readouterr().err)]
    return syn, m, n, g, counts


def _check(sc, tables, moments, monkeypatch, capfd, want):
    """want: (plans, regular ones) of every evaluation that makes plans, or None: none is made"""
    a = _evaluate(sc, tables, moments, monkeypatch, capfd, regular=True, duo=True)
    b = _evaluate(sc, tables, moments, monkeypatch, capfd, regular=False, duo=True)
    c = _evaluate(sc, tables, moments, monkeypatch, capfd, regular=False, duo=False)
    if want is None:
        assert a[4] == b[4] == c[4] == []
    else:
        assert a[4] == [want, want], (a[4], want)                # (two evaluations per engine, one chunk each)
        assert b[4] == [(want[0], 0), (want[0], 0)], (b[4], want)
        assert c[4] == []
    assert len(a[0]) == len(b[0]) == len(c[0]) == len(tables) * sum(len(x) for x in sc.comps)
    assert sum(1 for x in a[0] if np.any(x != 0)) >= len(a[0]) // 2
    for x, y, z in zip(a[0], b[0], c[0]):
        assert same_bits(x, y) and same_bits(x, z)
    assert np.all(np.isfinite(a[1])) and np.any(a[1] > 0)
    assert _close(a, b) and _close(a, c)
    assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()


REGULAR = [[0, 1, 2, 3, 4], [1, 2], [0, 1], [1, 2], [0, 1], [3]]               # groups of five, two and one, the group of one last
ODD = [[0, 1, 2, 3, 4], [1, 2], [0, 2], [1, 1], [0, (1, 45 * DT)], [3]]         # ... a shift + 2, a shift that repeats, a step 45 samples late


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_regular_and_irregular_groups_in_one_workgroup(monkeypatch, capfd, ng):
    """Ten sources 0.1 degrees apart in strike: two groups of four and a pair.  One member of the second group of four and one of the
    pair carry the irregular step lists at three of their six points: the waves of a workgroup take different routines in the same
    centroid group."""
    sc = _scenario(ng, ["ned", "ned", "ned"])
    tm = [_table(p, ODD if i in (5, 8) else REGULAR) for i, p in enumerate(synthetic.bilat_strike_sweep(10, step=0.1))]
    tables = [t for t, _ in tm]
    want = _expected(tables, range(10))
    assert want == (10 * 6 * NREC, (10 * 6 - 2 * 3) * NREC)
    _check(sc, tables, [m for _, m in tm], monkeypatch, capfd, want)


@pytest.mark.gpu
def test_time_sweep_with_a_common_tile_origin(monkeypatch, capfd):
    """Four sources in the same cells with origin times 0, 2, 5 and 14 samples apart: the shifts of all four fit the tile's halo, the
    four tile sets share the origin of the largest shift, and every member's e0 -- its first step's position from that origin -- is
    its own."""
    sc = _scenario(10, ["ned", "ned", "ned"])
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    tm = [_table(base, [[0, 1], [1, 2], [2, 3, 4]], t_add=d) for d in (0.0, 1.0, 2.5, 7.0)]
    tables = [t for t, _ in tm]
    want = _expected(tables, range(4))
    assert want == (4 * 3 * NREC, 4 * 3 * NREC)
    _check(sc, tables, [m for _, m in tm], monkeypatch, capfd, want)


@pytest.mark.gpu
def test_descriptor_rows_make_no_plans(monkeypatch, capfd):
    """A database with gaps and static end values has no compact descriptors: no plans are made, nothing is counted and the kernel
    takes the general routine whatever the switch says."""
    sc = _scenario(10, ["ned", "ned", "ned"], variant="static")
    tm = [_table(p, REGULAR[:4]) for p in synthetic.bilat_strike_sweep(6, step=0.1)]
    _check(sc, [t for t, _ in tm], [m for _, m in tm], monkeypatch, capfd, None)
