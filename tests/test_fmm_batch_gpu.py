"""The device march (kiwi_amd/csrc/kiwi_fmm_device.hpp: one fast-marching solve per wavefront) against the host's routines.

Every comparison is bit for bit on EVERY node -- with `discard` too: the device march is the reference's sequence of steps, so
the nodes it leaves undone hold what the plain routine leaves in them.  No solve of these inputs may fall back to the host.
The case with a zero and a negative speed runs last."""
import numpy as np
import pytest

from kiwi_amd import Engine, engine as ke
from kiwi_amd import lib as klib
from tests.common import Scenario
from tests.test_fast_marching import product
from tests.test_fmm_batch import mixed_batch, plain_times, assert_same_bits, cfg4_field, cfg4_starts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_mixed_batch_on_the_device_gives_the_plain_routines_bits(eng):
    sp, og, dl, st, di = mixed_batch()
    got, fb = ke.fast_marching_batch(sp, og, dl, st, di, engine=eng)
    assert fb == 0
    assert_same_bits(got, plain_times(sp, og, dl, st, di))
    up, kern, down = eng.eikonal_solver_ms()
    assert kern > 0.0 and up > 0.0 and down > 0.0


def test_equal_keys_by_the_hundred(eng):
    """Uniform fields on square cells, the start in a cell centre: fourfold and eightfold symmetric fronts, hundreds of equal
    keys -- the order among them is heap.f90's, and the times depend on it."""
    sp, og, dl, st = [], [], [], []
    for seed in range(16):
        rng = np.random.default_rng(9000 + seed)
        nx, ny = int(rng.integers(30, 140)), int(rng.integers(30, 140))
        if seed % 4 == 0:
            ny = nx
        sp.append(np.full((ny, nx), np.float32(3000.0 * rng.uniform(0.5, 1.0)), np.float32))
        d = np.float32(rng.uniform(20, 900))
        origin = rng.uniform(-5000, 0, 2).astype(np.float32)
        cell = np.array([nx // 2, ny // 2]) if seed % 4 == 0 else np.array([rng.integers(0, nx), rng.integers(0, ny)])
        og.append(origin); dl.append(np.array([d, d], np.float32))
        st.append((origin + (cell + 0.5) * np.array([d, d], np.float32)).astype(np.float32))
    got, fb = ke.fast_marching_batch(sp, og, dl, st, engine=eng)
    assert fb == 0
    want = plain_times(sp, og, dl, st, [np.nan] * len(sp))
    assert_same_bits(got, want)
    assert max(len(t.ravel()) - len(np.unique(t)) for t in want) > 300          # (equal times by the hundred indeed)


def test_one_cfg4_sized_grid_and_256_of_them(eng, monkeypatch):
    speed, origin, delta, dis = cfg4_field()
    one, fb = ke.fast_marching_batch([speed], [origin], [delta], [np.array([2300., -1000.], np.float32)], [dis], engine=eng)
    assert fb == 0
    want, _ = product(speed, origin, delta, np.array([2300., -1000.], np.float32), discard=dis, plain=1)
    assert np.array_equal(one[0].view(np.uint32), want.view(np.uint32))
    n = 256
    starts = cfg4_starts(n)
    # per solve another rupture speed (the cfg4-nukl sweep varies both), same geometry
    fac = np.random.default_rng(3).uniform(0.6, 1.0, n).astype(np.float32)
    sp = [speed * f for f in fac]
    di = [float(np.float32(dis) * f) for f in fac]
    host, hfb = ke.fast_marching_batch(sp, [origin] * n, [delta] * n, starts, di)
    assert hfb == 0
    for k in range(0, n, 37):                                   # (the host's march itself against the plain statements, a sample)
        w, _ = product(sp[k], origin, delta, starts[k], discard=di[k], plain=1)
        assert np.array_equal(host[k].view(np.uint32), w.view(np.uint32))
    dev, fb = ke.fast_marching_batch(sp, [origin] * n, [delta] * n, starts, di, engine=eng)
    assert fb == 0
    assert_same_bits(dev, host)
    launches, hiwater = eng.eikonal_solver_stats()
    assert launches == 1 and 500 < hiwater <= 2048             # (the front of this field: about a thousand entries of the 4096)
    print("256 cfg4-sized solves: upload %.1f ms, kernel %.1f ms, download %.1f ms" % eng.eikonal_solver_ms())
    # a workspace bound of 100 MB holds 14 of these solves (16 bytes per node): several launches, the same bits
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "100")
    small = Engine(0)
    try:
        dev2, fb = ke.fast_marching_batch(sp[:40], [origin] * 40, [delta] * 40, starts[:40], di[:40], engine=small)
        assert fb == 0
        assert_same_bits(dev2, host[:40])
        assert small.device_bytes() < 120 * 2 ** 20
        assert small.eikonal_solver_stats()[0] == 3             # 15 + 15 + 10 solves
    finally:
        small.close()


def test_switch_getter_and_environment_agree(monkeypatch):
    monkeypatch.delenv("KIWI_HIP_EIK_DEVICE", raising=False)
    e = Engine(0)
    assert e.eikonal_solver == "host"
    assert e.eikonal_solver_ms() == (0.0, 0.0, 0.0)
    e.set_eikonal_solver("device")
    assert e.eikonal_solver == "device"
    e.set_eikonal_solver("host")
    assert e.eikonal_solver == "host"
    with pytest.raises(ValueError):
        e.set_eikonal_solver("gpu")
    assert klib.load().kiwi_hip_set_eikonal_solver(e.h, 2) != 0
    e.close()
    monkeypatch.setenv("KIWI_HIP_EIK_DEVICE", "1")
    e = Engine(0)
    assert e.eikonal_solver == "device"
    e.close()
    e = Engine(0, eikonal_solver="host")
    assert e.eikonal_solver == "host"
    e.close()
    monkeypatch.setenv("KIWI_HIP_EIK_DEVICE", "0")
    e = Engine(0, ndev=1, eikonal_solver="device")
    assert e.eikonal_solver == "device"
    e.close()


G = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "eikonal_vectors.npz"))
CP = np.array([[0, 0, 6500.0], [0, 0, 15500.0], [0, -2000.0, 0]], np.float32)
CN = np.array([[0, 0, -1.0], [0, 0, 1.0], [0.2, -1.0, 0]], np.float32)


def shape_sweep(stype, n):
    """Trial list with nucleation point and rupture velocity varied (no two solves alike), one trial the discretiser rejects
    for its nucleation point, one for an empty rupture area, and trials that differ from an earlier one only in moment / rise
    time."""
    st = 4 if stype == "eikonal" else 5
    rng = np.random.default_rng(40 + st)
    trials = []
    for i in range(n):
        common = [0.05 * (i % 7), 30.0 * (i % 11), -20.0 * (i % 5), 10500.0 + 100 * (i % 3)]
        bord = [100.0, -50.0, 2500.0 + 100 * (i % 4)]
        nukl = [rng.uniform(-1200, 1200), rng.uniform(-900, 900)]
        relv = rng.uniform(0.6, 0.95)
        if st == 5:
            t = common + [1.0, 80.0, 70.0] + bord + nukl + [relv] + list(rng.standard_normal(6) * 7e17) + [0.4 * (i % 3)]
        else:
            t = common + [7e18, 80.0, 70.0, -170.0] + bord + nukl + [relv, 0.4 * (i % 3)]
        trials.append(t)
    trials = np.array(trials, np.float32)
    irise = 19 if st == 5 else 14
    for i in (9, 20, n - 2):                                  # same rupture as the trial before, other moment and rise time
        trials[i] = trials[i - 1]
        trials[i, 4] *= 1.5
        trials[i, irise] += 0.7
    trials[6, 10 if st == 5 else 11] = 9000.0                 # nucleation point far outside
    trials[n - 5, 3] = 300.0                                  # above the upper constraint: empty rupture area
    return trials


def eikonal_engine(make, sc):
    e = sc.oracle()
    sc.make_references(e)
    p = make()
    g = sc.gf
    first, nsamp, data = sc.odb.dense_tables()
    p.set_database(g["dt"], g["dx"], g["dz"], g["firstx"], g["firstz"], data, first, nsamp)
    p.set_receivers(sc.lat, sc.lon, sc.depth, sc.comps)
    p.set_source_location(40.0, 30.0, 0.0)
    p.set_effective_dt(sc.effective_dt)
    p.set_local_interpolation("bilinear" if sc.bilinear else "nearest")
    sc.apply_setup(p, False)
    p.set_source_crust(G["rupture_profile"], G["origin_profile"])
    p.set_source_crustal_thickness_limit(9000.0)
    p.set_source_constraints(CP, CN)
    return p


@pytest.mark.parametrize("stype", ["mt_eikonal", "eikonal"])
@pytest.mark.parametrize("multi", [False, True])
def test_trial_lists_do_not_depend_on_the_solver(stype, multi):
    """make_misfits_for_sources over a rupture-shape sweep with the host and with the device solver: misfits, norm factors,
    global misfits and failings bit for bit the same, for the default piece (150 trials: a piece of 128 and the ramp) and
    for pieces of 5; through a one-device and through a multi-device context."""
    sc = Scenario(nz=6)
    n = 150
    trials = shape_sweep(stype, n)
    p = eikonal_engine((lambda: Engine(0, ndev=1)) if multi else (lambda: Engine(0)), sc)
    res = {}
    for solver in ("host", "device"):
        p.set_eikonal_solver(solver)
        assert p.eikonal_solver == solver
        for piece in (0, 5):
            m, nf, g, status = p.misfits_for_params(stype, trials, piece)
            mis, nor, failings = p.make_misfits_for_sources(stype, trials, piece)
            res[solver, piece] = (m, nf, g, status, mis, nor, failings)
        if solver == "device" and not multi:
            assert p.eikonal_solver_ms()[1] > 0.0
    want = res["host", 0]
    assert want[6] == [6, n - 5] and list(np.nonzero(want[3])[0]) == [6, n - 5] and want[3][6] == 6 and want[3][n - 5] == 5
    assert np.count_nonzero(want[0]) > 0.9 * want[0].size
    for key, got in res.items():
        for a, b in zip(got[:6], want[:6]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
        assert got[6] == want[6], key
    # the uploaded-batch path (kiwi_hip_set_sources_params) too
    p.set_eikonal_solver("device")
    p.set_source_params(stype, trials[:12])
    p.eval()
    dm = p.get_misfits()
    p.set_eikonal_solver("host")
    p.set_source_params(stype, trials[:12])
    p.eval()
    hm = p.get_misfits()
    for a, b in zip(dm, hm):
        assert a.tobytes() == b.tobytes()
    assert hm[0][:6].tobytes() == want[0][:6].tobytes()
    p.close()


def _cache_stats(reset=0):
    import ctypes as C
    h, m = C.c_longlong(0), C.c_longlong(0)
    klib.load().kiwi_hip_eikonal_cache_stats(C.byref(h), C.byref(m), reset)
    return h.value, m.value


def test_location_grid_hits_the_solve_cache_alike_in_both_modes(monkeypatch):
    """A location grid repeats a handful of solves: with the device solver the cache answers them as with the host's (same hit
    and miss counts; one discretiser thread, so that the host's counts do not depend on which thread stores first), solves
    the cache answers do not go to the device, and the misfits are the same bits."""
    monkeypatch.setenv("KIWI_HIP_DISC_THREADS", "1")
    sc = Scenario(nz=6)
    base = shape_sweep("mt_eikonal", 30)[0]
    trials = []
    for dn in (0.0, 150.0, -300.0, 450.0):
        for de in (0.0, 100.0, 250.0):
            for depth in (0.0, 1500.0):
                t = base.copy()
                t[1] += dn; t[2] += de; t[3] += depth
                trials.append(t)
    trials = np.array(trials, np.float32)
    p = eikonal_engine(lambda: Engine(0), sc)
    p.set_source_constraints(CP[:2], CN[:2])                   # (depth limits only: a shift north or east leaves the rupture's outline alone)
    out = {}
    for solver in ("host", "device"):
        p.set_eikonal_solver(solver)
        _cache_stats(reset=3)
        m1 = p.misfits_for_params("mt_eikonal", trials, 0)
        first = _cache_stats()
        m2 = p.misfits_for_params("mt_eikonal", trials, 7)
        out[solver] = (first, _cache_stats(), m1, m2)
    assert out["host"][0] == out["device"][0] and out["host"][1] == out["device"][1], (out["host"][:2], out["device"][:2])
    hits, misses = out["device"][0]
    assert misses <= 4 and hits >= len(trials) - 4
    for k in (2, 3):
        for a, b in zip(out["host"][k], out["device"][k]):
            assert a.tobytes() == b.tobytes()
    p.close()


def test_inputs_outside_of_the_hosts_state_encoding_end_like_any_other(eng):
    """A zero and a negative speed (infinite, negative and NaN times): input the plain routine handles, and the device march is
    the plain routine -- its loops are bounded by the grid's size whatever the times are.  Same bits; a counted fallback
    would be allowed here and is not needed."""
    speed = np.full((6, 9), 2000.0, np.float32)
    speed[2, 3] = 0.0
    speed[4, 6] = -1500.0
    ok = np.full((6, 9), 2000.0, np.float32)
    origin, delta, start = np.zeros(2, np.float32), np.array([100., 120.], np.float32), np.array([450., 350.], np.float32)
    got, fb = ke.fast_marching_batch([ok, speed, ok], [origin] * 3, [delta] * 3, [start] * 3, engine=eng)
    assert fb in (0, 1)
    assert_same_bits(got, plain_times([ok, speed, ok], [origin] * 3, [delta] * 3, [start] * 3, [np.nan] * 3))
