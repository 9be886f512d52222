"""accumulate_multi_kernel applying the centroid groups whose REPEATED shifts its plans name (a group of at most five, every integer shift
its predecessor's + 1 or its predecessor's: bits 12 .. 15 of PlanSrc::head, kiwi_common.hpp) with the text made for them
(lines_repeat of tools/gen_apply_asm.py: no tile read for a step that stays) against the same binary with the bits never set
(KIWI_HIP_MULTI_REPEAT=0: those groups take the general routine) and against the one-source kernels (KIWI_HIP_DUO=0): synthetics,
misfits and global misfits, bit for bit under `exact`, within the contract's tolerances under `fused`.

Scenario and tables as tests/test_gpu_multi_regular.py: a database of 16 x 5 nodes with 1100 samples, three receivers, ten sources 0.1
degrees apart (two groups of four and a pair: K = 5 and K = 9), centroid tables cut from discretised bilateral sources with the time
steps on the sample grid -- step index k of a point: the point's first shift + k.  The numbers of regular plans and of plans with named
repeats the library reports (KIWI_HIP_DEBUG) are compared with the numbers the test derives from its own tables."""
import re

import numpy as np
import pytest

from kiwi_amd import synthetic
from tests.common import same_bits
from tests.test_gpu_multi_plan import DT, _close, _scenario
from tests.test_gpu_multi_regular import NREC, _groups, _table

E0_MAX = 0x7f             # kPlanE0Mask: the header word's field for e0


def _expected(tables, multi_sources):
    """(plans, regular plans, plans with named repeats) of the sources accumulate_multi_kernel takes, all NREC receivers.  (e0, the
    first step's position from the tile origin, is at most the spread of the shifts of the group's members here: far below E0_MAX.)"""
    plans = regular = repeat = 0
    for s in multi_sources:
        for g in _groups(tables[s]):
            d = [b - a for a, b in zip(g, g[1:])]
            assert max(g) - min(g) + 14 <= E0_MAX
            plans += NREC
            regular += NREC * int(all(x == 1 for x in d))
            repeat += NREC * int(len(g) <= 5 and all(x in (0, 1) for x in d) and 0 in d)
    return plans, regular, repeat


def _evaluate(sc, tables, moments, monkeypatch, capfd, repeat, duo):
    monkeypatch.setenv("KIWI_HIP_MULTI_REPEAT", "1" if repeat else "0")
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
    err = capfd.readouterr().err
    counts = [(int(a), int(b)) for a, b in re.findall(r"multi plans: (\d+) of a \(source, centroid group, receiver\), (\d+) regular", err)]
    named = [int(a) for a in re.findall(r"multi plans with named repeats: (\d+)", err)]
    return syn, m, n, g, counts, named


def _check(sc, tables, moments, monkeypatch, capfd, want):
    """want: (plans, regular ones, ones with named repeats) of every evaluation"""
    a = _evaluate(sc, tables, moments, monkeypatch, capfd, repeat=True, duo=True)
    b = _evaluate(sc, tables, moments, monkeypatch, capfd, repeat=False, duo=True)
    c = _evaluate(sc, tables, moments, monkeypatch, capfd, repeat=False, duo=False)
    print("plans, regular, named repeats: want", want, "counted", a[4], a[5], "without the switch", b[4], b[5])
    assert a[4] == [want[:2], want[:2]] and a[5] == [want[2], want[2]], (a[4], a[5], want)      # (two evaluations per engine, one chunk each)
    assert b[4] == [want[:2], want[:2]] and b[5] == [0, 0], (b[4], b[5], want)                  # the regular count does not move
    assert c[4] == [] and c[5] == []
    assert len(a[0]) == len(b[0]) == len(c[0]) == len(tables) * sum(len(x) for x in sc.comps)
    assert sum(1 for x in a[0] if np.any(x != 0)) >= len(a[0]) // 2
    for x, y, z in zip(a[0], b[0], c[0]):
        assert same_bits(x, y) and same_bits(x, z)
    assert np.all(np.isfinite(a[1])) and np.any(a[1] > 0)
    assert _close(a, b) and _close(a, c)
    assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()


SIX = [0, 1, 2, 3, 4, (4, DT)]
# by point: groups of five (four of them), of two, of six, of three and of one; a point's group has the same length in every list
REGULAR = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [1, 2], SIX, [0, 1, 2], [3]]
REPEAT = [[2, 2, 2, 2, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 3], [0, 0, 1, 1, 2], [1, 1], [0, 1, 2, 2, 3, 4], [0, 0, 1], [3]]    # (six with a repeat: general)
GENERAL = [[0, 0, 2, 3, 4], [0, 1, 2, 3, (4, 45 * DT)], [0, 1, 2, 3, 4], [0, 1, 1, 2, 2], [0, 2], SIX, [0, 0, 2], [3]]      # (fourth point: a repeat list, third: regular)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_regular_repeating_and_general_groups_in_one_workgroup(monkeypatch, capfd, ng):
    """Ten sources 0.1 degrees apart in strike: two groups of four and a pair.  The second group of four holds a member with the
    regular lists, one with the repeat lists, one with the general lists: at the first, second, fifth and seventh point the waves of a
    workgroup take the three texts in the same centroid group.  The pair: repeat lists beside general ones."""
    sc = _scenario(ng, ["ned", "ned", "ned"])
    lists = {5: REPEAT, 6: GENERAL, 8: REPEAT, 9: GENERAL}
    tm = [_table(p, lists.get(i, REGULAR)) for i, p in enumerate(synthetic.bilat_strike_sweep(10, step=0.1))]
    tables = [t for t, _ in tm]
    want = _expected(tables, range(10))
    # REGULAR: 8 regular plans; REPEAT: 1 regular (the group of one), 6 with named repeats; GENERAL: 3 regular, 1 with named repeats
    assert want == (10 * 8 * NREC, (6 * 8 + 2 * 1 + 2 * 3) * NREC, (2 * 6 + 2 * 1) * NREC)
    _check(sc, tables, [m for _, m in tm], monkeypatch, capfd, want)


@pytest.mark.gpu
def test_time_sweep_with_a_common_tile_origin(monkeypatch, capfd):
    """Four sources in the same cells with origin times 0, 2, 5 and 14 samples apart: the four tile sets share the origin of the largest
    shift, and every member's e0 -- its first step's position from that origin -- is its own."""
    sc = _scenario(10, ["ned", "ned", "ned"])
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    tm = [_table(base, [[0, 0, 1], [1, 1], [2, 2, 3, 4, 4]], t_add=d) for d in (0.0, 1.0, 2.5, 7.0)]
    tables = [t for t, _ in tm]
    want = _expected(tables, range(4))
    assert want == (4 * 3 * NREC, 0, 4 * 3 * NREC)
    _check(sc, tables, [m for _, m in tm], monkeypatch, capfd, want)
