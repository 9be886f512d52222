"""accumulate_multi_kernel's build with the lean group top -- plan rows premultiplied by multi_plan_kernel, the group's header, flags
and rotation from one scalar load, the coefficient pointer carried as a scalar, the halo decision a scalar compare, the weights of
the blends only some waves make loaded a second time -- against the un-staged one-source kernel (KIWI_HIP_ACCUM=direct) on the same
engine set-up: misfits, norm factors, global misfits and kept synthetics, bit for bit under `exact`, within the contract's tolerances
 under `fused`.

Scenario and tables as tests/test_gpu_multi_plan.py: a database of 16 x 5 nodes with 1100 samples (five 256-sample tiles, two
512-sample tiles, the last one partial), three receivers, centroid tables cut from discretised bilateral sources.  Every case is
chosen to take one path of the build; that its parameters really do is checked on the host, from the tables, the receivers and the
database's grid alone (the library's rules restated: _groups, _cells, _quads_and_pairs), before anything runs on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import synthetic
from tests.common import Scenario, arith, misfit_close, same_bits
from tests.test_gpu_multi_plan import DT, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 64                 # positions behind a tile that a tile set holds (kHalo, kiwi_common.hpp)
QUAD_SPAN = 16            # first shifts of the members of a group of four at most this far apart (kiwi_quad_shift_span)
_SCENARIOS = {}


def _scenario(ng):
    """one scenario per component count, its references computed once"""
    if ng not in _SCENARIOS:
        sc = Scenario(nx=16, nz=5, ng=ng, L=1100, nrec=3, comps_list=["ned", "ned", "ned"])
        e = sc.oracle()
        sc.make_references(e)
        sc.receiver_geometry = [e.receiver_geometry(ir + 1) for ir in range(sc.nrec)]
        e.close()
        _SCENARIOS[ng] = sc
    return _SCENARIOS[ng]


# ---------------------------------------------------------------- the library's rules, restated on the host
def _groups(table):
    """[(point, [integer shifts])] of a table: runs of centroids at the same point (kiwi_hip_set_sources' rule, for groups far below
    its limits of length and of shift spread)"""
    out = []
    for row in table:
        sh = int(np.floor(np.float32(row[3]) / np.float32(DT)))
        if out and np.array_equal(row[:3], out[-1][0]):
            out[-1][1].append(sh)
        else:
            out.append((row[:3].copy(), [sh]))
    assert all(max(s) - min(s) <= HALO - 10 for _, s in out)
    return out


def _receiver_xy(sc, ir):
    """north, east of receiver ir from the source location, metres: the CPU oracle's azimuth and distance (the reference's own
    formulas on the oblate earth: 103.86 km for the receiver laid out at 104), laid out in the plane around the source"""
    az, _, d = sc.receiver_geometry[ir]
    return d * np.cos(az), d * np.sin(az)


def _cell(sc, point, ir):
    """(distance cell of the database's grid, metres to the nearer node line) of a centroid for receiver ir.  The centroids lie a
    few kilometres from the source: in the plane their distance is within metres of the sphere's; the set-ups ask for MARGIN."""
    rn, re = _receiver_xy(sc, ir)
    x = (np.hypot(rn - float(point[0]), re - float(point[1])) - sc.gf["firstx"]) / sc.gf["dx"]
    return int(np.floor(x)), float(min(x - np.floor(x), np.ceil(x) - x) * sc.gf["dx"])


def _same_structure(ta, tb, shifts):
    ga, gb = _groups(ta), _groups(tb)
    if len(ta) != len(tb) or [len(s) for _, s in ga] != [len(s) for _, s in gb]:
        return False
    if shifts and abs(ga[0][1][0] - gb[0][1][0]) > QUAD_SPAN:
        return False
    near = 0.25 * 4000.0
    return bool(np.all(np.abs(ta[0][:2] - tb[0][:2]) <= near) and np.all(np.abs(ta[-1][:2] - tb[-1][:2]) <= near))


def _quads_and_pairs(tables):
    """(groups of four, pairs) the host forms of a chunk: aligned neighbours of equal structure"""
    n = len(tables)
    quads = [all(_same_structure(tables[4 * k], tables[4 * k + i], True) for i in (1, 2, 3)) for k in range(n // 4)]
    pairs = [not (k // 2 < len(quads) and quads[k // 2]) and _same_structure(tables[2 * k], tables[2 * k + 1], False) for k in range(n // 2)]
    return sum(quads), sum(pairs)


MARGIN = 250.0            # metres from a node line below which this restatement does not decide a centroid's cell


def _shared(sc, tables, members, margin=MARGIN):
    """per (centroid group, receiver) of a source group: True where all members sit in the same distance cell AND their largest
    shifts agree or fit one tile origin (multi_plan_kernel's `shared`); a member closer than `margin` to a node line fails the
    test's own set-up (the centroids' distances are the oracle's receiver distance moved in the plane: good to metres for the
    kilometres they lie from the source, and the margin is a hundred times that)"""
    out = []
    gs = [_groups(tables[m]) for m in members]
    for j in range(len(gs[0])):
        for ir in range(sc.nrec):
            cells = [_cell(sc, g[j][0], ir) for g in gs]
            assert all(m >= margin for _, m in cells), (j, ir, cells)
            same_rows = len({c for c, _ in cells}) == 1
            smax, smin = [max(g[j][1]) for g in gs], [min(g[j][1]) for g in gs]
            fits = len(set(smax)) == 1 or (max(smax) - min(smin)) + 8 <= HALO
            out.append(same_rows and fits)
    return out


# ---------------------------------------------------------------- evaluation
def _evaluate(sc, trial_lists, monkeypatch, direct, env=()):
    """[(misfits, norm factors, global misfits, synthetics)] of the trial lists, evaluated one after the other on ONE engine"""
    monkeypatch.delenv("KIWI_HIP_ACCUM", raising=False)
    if direct:
        monkeypatch.setenv("KIWI_HIP_ACCUM", "direct")
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KIWI_HIP_POISON", "1")             # a plan, descriptor or coefficient line read but not written shows
    p = sc.product()
    sc.apply_setup(p, False)
    out = []
    for tables, moments in trial_lists:
        p.set_keep_synthetics(0)
        p.set_sources(tables, moments=moments)
        p.eval()
        m, n, g = [x.copy() for x in p.get_misfits()]
        p.set_keep_synthetics(1)
        p.eval()
        syn = [p.get_synthetics(s, ir, k, 1)[1].copy() for s in range(len(tables)) for ir in range(1, sc.nrec + 1)
               for k in range(1, len(sc.comps[ir - 1]) + 1)]
        out.append((m, n, g, syn))
    p.close()
    for k, _ in env:
        monkeypatch.delenv(k, raising=False)
    return out


def _same(a, b):
    """two evaluations of one trial list: misfits, norm factors, global misfits, synthetics"""
    assert a[1].tobytes() == b[1].tobytes()                 # the references' norm factors: not the kernels' business
    assert np.all(np.isfinite(a[0])) and np.any(a[0] > 0)
    if arith() == "exact":
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    else:
        assert misfit_close(a[0], b[0], a[1]) and misfit_close(a[2], b[2], glob=True)
    assert len(a[3]) == len(b[3]) and sum(1 for x in a[3] if np.any(x != 0)) >= len(a[3]) // 2
    for x, y in zip(a[3], b[3]):
        assert same_bits(x, y)


def _check(sc, trial_lists, monkeypatch):
    a = _evaluate(sc, trial_lists, monkeypatch, direct=False)
    b = _evaluate(sc, trial_lists, monkeypatch, direct=True)
    assert len(a) == len(b) == len(trial_lists)
    for x, y in zip(a, b):
        _same(x, y)


# ---------------------------------------------------------------- the cases' trial lists, each with the proof of its path
BASE = np.array(synthetic.TRUE_BILAT, np.float32)
BASE[1] -= 1500.0         # 1.5 km south: every point of the sweeps below is MARGIN or more inside its cell for every receiver
LENGTHS = [[2], [0, 1], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, (4, 1 * DT), (4, 2 * DT)], [3]]        # groups of 1, 2, 5, 7 and 1


def _split(tm):
    return [t for t, _ in tm], [m for _, m in tm]


def trials_sweep(sc, nsrc=10, steps=LENGTHS):
    """a strike sweep at 0.1 degree steps: groups of four and a pair whose every build is shared, group lengths 1, 2, 5 and 7"""
    tables, moments = _split([_table(p, steps) for p in synthetic.bilat_strike_sweep(nsrc, step=0.1, base=BASE)])
    assert _quads_and_pairs(tables) == (nsrc // 4, (nsrc % 4) // 2)
    assert [len(s) for _, s in _groups(tables[0])] == [len(ks) for ks in steps]
    for k in range(nsrc // 4):
        assert all(_shared(sc, tables, range(4 * k, 4 * k + 4)))
    if nsrc % 4 >= 2:
        assert all(_shared(sc, tables, range(nsrc - nsrc % 4, nsrc - nsrc % 4 + 2)))
    return tables, moments


def trials_one_step(sc):
    """one time step per point: every group's shifts span nothing, the halo is the eight positions every group reads"""
    tables, moments = trials_sweep(sc, 6, [[2], [0], [4], [1]])
    assert all(max(s) == min(s) for t in tables for _, s in _groups(t))
    return tables, moments


def trials_five_steps(sc):
    """five time steps per point: the shifts of a group span four or five samples, the halo is wider than the eight"""
    tables, moments = trials_sweep(sc, 4, [[0, 1, 2, 3, 4]] * 3)
    assert all(max(s) - min(s) >= 3 for t in tables for _, s in _groups(t))
    return tables, moments


def _halo_waves(ng, spread):
    """the waves of a workgroup that hold a halo lane of a group whose shifts span `spread` samples: thread 255 - q holds chunk q // ng
    (four samples) of component q % ng for q < 16 ng, and a group reads spread + 8 positions behind its tile (multi_build), lane by lane"""
    return [w for w in range(4) if any(q < 16 * ng and 4 * (q // ng) < spread + 8 for q in range(64 * (3 - w), 64 * (3 - w) + 64))]


def trials_wide_halo(sc, ng):
    """groups whose two time steps lie 20 and 45 samples apart: the halo reaches into the lanes of wave 2 (ten components: beyond 24
    positions; eight: beyond 32) and of wave 1 (ten components: beyond 48; eight: never) -- every other case here keeps it in wave 3"""
    tables, moments = trials_sweep(sc, 4, [[0, (1, 20 * DT)], [1, (2, 45 * DT)], [2, 3]])
    spreads = [max(s) - min(s) for _, s in _groups(tables[0])]
    assert 20 <= spreads[0] <= 22 and 45 <= spreads[1] <= 47 and spreads[2] <= 2
    want = {10: [[2, 3], [1, 2, 3], [3]], 8: [[3], [2, 3], [3]]}[ng]
    assert [_halo_waves(ng, s) for s in spreads] == want
    assert all([max(s) - min(s) for _, s in _groups(t)] == spreads for t in tables)
    return tables, moments


def trials_straddle(sc):
    """a group of four astride a node line of the first receiver (104 km: a node of the 4 km grid that starts at 100 km): the first
    member's points lie short of it, the last two members' beyond -- their rows differ, the tile sets are built one by one"""
    base = np.array(synthetic.TRUE_BILAT, np.float32)
    tm = []
    for north in (450.0, -100.0, -300.0, -500.0):
        q = base.copy()
        q[1] += north
        tm.append(_table(q, [[0, 1], [1, 2], [2, 3]]))
    tables, moments = _split(tm)
    assert _quads_and_pairs(tables) == (1, 0)
    first = [_cell(sc, _groups(tables[0])[j][0], 0) for j in range(3)]
    last = [_cell(sc, _groups(tables[3])[j][0], 0) for j in range(3)]
    assert all(m >= MARGIN for _, m in first + last)        # receiver 1: the first and the last member surely in different cells
    assert len({c for c, _ in first}) == len({c for c, _ in last}) == 1 and first[0][0] != last[0][0]
    assert not any(_shared(sc, tables, range(4), margin=0.0)[0::sc.nrec])
    return tables, moments


def trials_time_sweep(sc):
    """four sources in the same cells, origin times 0, 2, 5 and 14 samples apart: different largest shifts that fit one tile origin"""
    tables, moments = _split([_table(BASE, [[0, 1], [1, 2], [2, 3]], t_add=d) for d in (0.0, 1.0, 2.5, 7.0)])
    assert _quads_and_pairs(tables) == (1, 0)
    gs = [_groups(t) for t in tables]
    for j in range(3):
        smax = [max(g[j][1]) for g in gs]
        assert len(set(smax)) == 4 and max(smax) - min(min(g[j][1]) for g in gs) + 8 <= HALO
    assert all(_shared(sc, tables, range(4)))
    return tables, moments


def trials_window_edges(sc):
    """a group of four 20 samples late and one 20 samples early against the references' windows: the first tile of the late ones
    starts in front of the first stored sample of their rows, the last tile of the early ones ends behind the last -- the clamped
    row form; the tiles between them lie inside every row"""
    sweep = synthetic.bilat_strike_sweep(8, step=0.1, base=BASE)
    steps = [[0, 1], [1, 2], [2, 3]]
    tables, moments = _split([_table(p, steps, t_add=(10.0 if i < 4 else -10.0)) for i, p in enumerate(sweep)])
    assert _quads_and_pairs(tables) == (2, 0)
    true_groups = _groups(_table(BASE, [[0, 1, 2, 3, 4]] * 3)[0])
    first = sc.gf["first"][:, 0, 0]
    L = sc.gf["data"].shape[-1]
    for ir in range(sc.nrec):
        lo, d = sc.refs[(ir + 1, 1)]
        cells = {_cell(sc, pt, ir)[0] for pt, _ in true_groups}
        row_lo, row_hi = max(first[c + 1] for c in cells), min(first[c] for c in cells) + L       # inside EVERY row of the cells
        late, early = _groups(tables[0]), _groups(tables[4])
        # tile 0 of a late member reads from trace sample lo - smax - 1 on; the last tile of an early one up to its origin + 256 + 64
        assert all(lo - max(s) - 1 < row_lo - 8 for _, s in late)
        ntile = (len(d) + 255) // 256
        assert all(lo + 256 * (ntile - 1) - max(s) - 1 + 256 + HALO > row_hi + 8 for _, s in early)
        assert all(lo + 256 - max(s) - 1 >= row_lo and lo + 256 - max(s) - 1 + 256 + HALO <= row_hi for g in (late, early) for _, s in g)
    return tables, moments


# ---------------------------------------------------------------- the tests
@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_shared_builds_of_every_group_length(monkeypatch, ng):
    """Ten sources: two groups of four and a pair, every build shared, groups of 1, 2, 5 and 7 centroids, ten and eight components."""
    sc = _scenario(ng)
    _check(sc, [trials_sweep(sc)], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", ["one", "five"])
def test_halo_width(monkeypatch, steps):
    """Groups whose shifts span nothing, and groups whose shifts span four samples or more."""
    sc = _scenario(10)
    _check(sc, [trials_one_step(sc) if steps == "one" else trials_five_steps(sc)], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_halo_lanes_in_waves_one_and_two(monkeypatch, ng):
    """Shift spreads of 20 and 45 samples: the per-wave threshold of the scalar halo decision decides for waves 1 and 2 as well."""
    sc = _scenario(ng)
    _check(sc, [trials_wide_halo(sc, ng)], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [10, 8])
def test_builds_one_by_one(monkeypatch, ng):
    """Members in different cells: rows, offsets and tile origin of every member from its own plan line."""
    sc = _scenario(ng)
    _check(sc, [trials_straddle(sc)], monkeypatch)


@pytest.mark.gpu
def test_merged_tile_origin(monkeypatch):
    sc = _scenario(10)
    _check(sc, [trials_time_sweep(sc)], monkeypatch)


@pytest.mark.gpu
def test_rows_that_end_inside_the_window(monkeypatch):
    sc = _scenario(10)
    _check(sc, [trials_window_edges(sc)], monkeypatch)


@pytest.mark.gpu
def test_two_evaluations_rewrite_the_plans(monkeypatch):
    """Two trial lists of different shape one after the other on one engine: the plan buffers of the first are rewritten."""
    sc = _scenario(10)
    _check(sc, [trials_sweep(sc), trials_straddle(sc), trials_one_step(sc)], monkeypatch)


_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import pytest
from tests import test_gpu_multi_lean as t
sc = t._scenario(10)
mp = pytest.MonkeyPatch()
(m, n, g, syn), = t._evaluate(sc, [t.trials_sweep(sc)], mp, direct=False)
mp.undo()
np.savez(sys.argv[1], m=m, n=n, g=g, **{"s%%d" %% i: x for i, x in enumerate(syn)})
"""


@pytest.mark.gpu
def test_record_path_in_a_fresh_process(monkeypatch, tmp_path):
    """KIWI_HIP_MULTI_PLAN=0, set before a fresh process loads the library: the same kernel text without plans, its results those of
    the one-source kernel as before."""
    sc = _scenario(10)
    out = str(tmp_path / "noplan.npz")
    env = dict(os.environ, KIWI_HIP_MULTI_PLAN="0", KIWI_HIP_POISON="1")
    env.pop("KIWI_HIP_ACCUM", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    child = (z["m"], z["n"], z["g"], [z["s%d" % i] for i in range(len(z.files) - 3)])
    ref, = _evaluate(sc, [trials_sweep(sc)], monkeypatch, direct=True)
    _same(child, ref)
