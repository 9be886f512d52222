"""kiwi_hip_linear_fit_time_scan on the device.  The yardstick is the parent's own code: offset 0 is kiwi_hip_linear_fit, and offset
k is kiwi_hip_linear_fit on a context whose references and tapers are moved by -k samples (route B of the time scan), whatever K,
the number of groups, the number of offsets against the kernel's offsets per pass, the window against its tile, the step, the
first source, the chunking, the pieces and the kind of context; the degenerate groups; what the call leaves behind; the
refusals; the moment-tensor helper, the grid and the example.  Comparison rule: the same bits under the `exact` arithmetic
contract; under `fused` the two calls' synthetics may come from different instantiations of the accumulate kernel, and
tests/test_linfit_gpu.py assert_same_fit's condition-number bound applies."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import gridsearch, mtfit
from kiwi_amd.lib import KiwiHipError
from tests import common
from tests import linfit_timescan_cases as lc
from tests.linfit_cases import PLANTED, mt_row
from tests.test_linfit_gpu import COMPS, FILTER, assert_same_fit, build, colocated_groups, multi_engine, scattered_groups
from tests.timescan_cases import OFFSETS, offsets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts


def assert_best(fit):
    assert np.array_equal(fit.best, lc.first_best(fit)), (fit.best, lc.first_best(fit))


# ------------------------------------------------------------------------------------------------ 1: offset 0 is linear_fit
@pytest.mark.parametrize("K", [1, 2, 6, 8])
def test_offset_zero_equals_linear_fit(K):
    sc, p = lc.standard()
    try:
        for ngroup in (1, 7):
            rows = scattered_groups(np.random.default_rng(100 * K + ngroup), ngroup, K)
            p.set_source_params("moment_tensor", rows)
            for anarchy in (False, True):
                want = p.linear_fit(0, ngroup, K, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True)
                got = p.linear_fit_time_scan(0, ngroup, K, 0, 1, 1, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True)
                assert got.coef.shape == (ngroup, 1, K) and got.normal.shape == (ngroup, 1, K * (K + 1) // 2 + K + 1)
                assert np.all(want.status == 0) and np.all(np.isfinite(got.coef))
                assert_same_fit(lc.flat(got), want, "K=%d ngroup=%d anarchy=%s" % (K, ngroup, anarchy))
                assert np.all(got.best == 0)
        ms = p.linear_fit_time_scan_ms()
        assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[3] >= 0
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: route B
def test_references_and_tapers_moved_the_other_way():
    """basis sources with fractional centroid times and rise times of 0, 1 and 2 s in one batch"""
    K, ngroup = 6, 3
    sc, p = lc.standard(planted=False)
    try:
        tabs, moments, rises = lc.scattered_tables(np.random.default_rng(17), ngroup, K)
        assert set(rises) == {0.0, 1.0, 2.0}
        p.set_sources(tabs, moments, rises)
        got = p.linear_fit_time_scan(0, ngroup, K, *OFFSETS, receiver_weights=WEIGHTS, normal=True)
        want = lc.stacked(lc.route_b(p, sc, offsets(*OFFSETS), lambda: p.linear_fit(0, ngroup, K, receiver_weights=WEIGHTS, normal=True)))
        assert np.all(got.status == 0)
        assert np.all(got.coef[:, 0] != got.coef[:, -1]), "the offsets change the coefficients"
        assert_same_fit(lc.flat(got), want, "route B")
        assert_best(got)
        print("route B: misfits per offset of group 0", got.misfit[0], "best", got.best)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: the kernel's constants
def _shape_scans(J):
    scans = []
    for nk in sorted({1, J - 1, J, J + 1, 9} - {0}):
        scans.append((-30, 5, nk))                            # from the largest shift one way, five samples apart ...
        scans.append((30 - (nk - 1), 1, nk))                  # ... and up to the largest shift the other way, one sample apart
    return scans


@pytest.mark.parametrize("K", [6, 8])
@pytest.mark.parametrize("which_window", ["100", "257", "tile + 1", "2 tile + 3"])
def test_offsets_per_pass_tiles_and_steps(which_window, K):
    """|k| up to 30: the onset of the synthetic crosses the window's edge, 20 samples behind the reference's first; a synthetics
    factor other than one; rise times folded"""
    import ctypes as C
    from kiwi_amd import lib as klib
    j, t = C.c_int(), C.c_int()
    assert klib.load().kiwi_hip_linear_fit_time_scan_shape(K, C.byref(j), C.byref(t)) == 0
    window = {"100": 100, "257": 257, "tile + 1": t.value + 1, "2 tile + 3": 2 * t.value + 3}[which_window]
    ngroup = 2
    sc, p = lc.standard(window, planted=False)
    try:
        J, T = p.linear_fit_time_scan_shape(K)
        assert (J, T) == (j.value, t.value) and J >= 2 and T % 256 == 0
        assert len(p.get_reference(3, 1, 2)[1]) == window
        scans = _shape_scans(J)
        assert {s[2] for s in scans} >= {1, J - 1, J, J + 1, 9} - {0}
        tabs, moments, rises = lc.scattered_tables(np.random.default_rng(window + K), ngroup, K)
        p.set_synthetics_factor(0.5)
        p.set_sources(tabs, moments, rises)
        ks = sorted(set(k for s in scans for k in offsets(*s)))
        assert min(ks) == -30 and max(ks) == 30
        per_k = lc.route_b(p, sc, ks, lambda: p.linear_fit(0, ngroup, K, normal=True))
        for scan in scans:
            got = p.linear_fit_time_scan(0, ngroup, K, *scan, normal=True)
            want = lc.stacked([per_k[ks.index(k)] for k in offsets(*scan)])
            assert np.all(got.status == 0)
            assert_same_fit(lc.flat(got), want, "window %d K %d scan %s" % (window, K, scan))
            assert_best(got)
        assert np.any(per_k[0].coef != per_k[-1].coef)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: however it is packed
def test_first_source_chunks_pieces_and_contexts(_arith, monkeypatch):
    ngroup, K = lc.CHUNK_GROUPS, lc.CHUNK_K
    rows = lc.chunk_rows()
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    sc, p = lc.standard()
    try:
        p.set_source_params("moment_tensor", rows)
        base = p.linear_fit_time_scan(0, ngroup, K, *lc.CHUNK_SCAN, normal=True)
        assert np.all(base.status == 0)
        assert_best(base)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        shifted = p.linear_fit_time_scan(5, ngroup, K, *lc.CHUNK_SCAN, normal=True)
        assert_same_fit(lc.flat(base), lc.flat(shifted), "isrc0 = 5")
        assert_best(shifted)
        for piece in (K, 3 * K, 0):
            got = p.linear_fit_time_scan_params("moment_tensor", rows, K, *lc.CHUNK_SCAN, normal=True, piece=piece)
            assert_same_fit(lc.flat(base), lc.flat(got), "piece %d" % piece)
            assert_best(got)
            assert p.nsrc == (len(rows) if piece == 0 else piece)
            p.eval()                                          # the engine holds the head of the list and knows how long it is
    finally:
        p.close()
    # several chunks: KIWI_HIP_CHUNK_MB is read when a context is made -- a process of its own
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_linfit_timescan_child_%d.npz" % os.getpid())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "linfit_timescan_cases.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, KIWI_HIP_CHUNK_MB="1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = dict(np.load(out))
    os.remove(out)
    assert z["launches"][1] >= 2, z["launches"]               # a chunk boundary between groups
    from kiwi_amd.engine import ScanFit
    chunked = ScanFit(z["coef"], z["misfit"], z["status"], z["pivot_min"], z["best"], z["normal"])
    assert_same_fit(lc.flat(base), lc.flat(chunked), "chunks")
    assert_best(chunked)
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = lc.standard(engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        for piece in (0, 2 * K):
            got = m2.linear_fit_time_scan_params("moment_tensor", rows, K, *lc.CHUNK_SCAN, normal=True, piece=piece)
            assert_same_fit(lc.flat(base), lc.flat(got), "two devices, piece %d" % piece)
            assert_best(got)
    finally:
        m2.close()


# ------------------------------------------------------------------------------------------------ 5: status 1 and status 2
def test_a_group_with_an_all_zero_basis_source():
    sc, p = lc.standard()
    try:
        rows = scattered_groups(np.random.default_rng(3), 3, 2)
        rows[3, 4:10] = 0.0                                   # group 1: second basis source without moment
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit_time_scan(0, 3, 2, *OFFSETS, normal=True)
        assert np.all(fit.status[1] == 1) and np.all(fit.pivot_min[1] == 0.0) and fit.best[1] == -1
        assert np.all(np.isnan(fit.coef[1])) and np.all(np.isnan(fit.misfit[1]))
        assert np.all(fit.status[[0, 2]] == 0) and np.all(np.isfinite(fit.coef[[0, 2]]))
        assert_best(fit)
    finally:
        p.close()


def test_a_rejected_basis_source_gives_its_group_status_two():
    """the rows of tests/test_timescan_gpu.py test_a_rejected_source_reads_as_zeros_with_best_minus_one, in groups of two"""
    sc, p = build(None, planted=False)
    try:
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (6, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((6, 6)) * 1e18
        eik[2, 3] = 500.0                                     # "Empty rupture area": above the constraining planes
        fit = p.linear_fit_time_scan_params("mt_eikonal", eik, 2, *OFFSETS, normal=True)
        assert np.all(fit.status[1] == 2) and fit.best[1] == -1
        assert np.all(np.isnan(fit.coef[1])) and np.all(np.isnan(fit.misfit[1]))
        assert np.all(fit.status[[0, 2]] == 0)
        good = p.linear_fit_time_scan_params("mt_eikonal", eik[[0, 1, 4, 5]], 2, *OFFSETS, normal=True)
        sub = type(fit)(fit.coef[[0, 2]], fit.misfit[[0, 2]], fit.status[[0, 2]], fit.pivot_min[[0, 2]], fit.best[[0, 2]], fit.normal[[0, 2]])
        assert_same_fit(lc.flat(sub), lc.flat(good), "groups beside a rejected one")
        assert_best(fit)
        # a piece in which nothing could be discretised: nothing is uploaded for it
        eik[3, 3] = 500.0
        alone = p.linear_fit_time_scan_params("mt_eikonal", eik, 2, *OFFSETS, normal=True, piece=2)
        assert np.all(alone.status[1] == 2) and alone.best[1] == -1 and np.all(alone.normal[1] == 0.0)
        assert_same_fit(lc.flat(sub), lc.flat(type(fit)(*[getattr(alone, f)[[0, 2]] for f in fit._fields])), "pieces of one group")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: the context afterwards
def test_context_afterwards():
    rows = colocated_groups(np.random.default_rng(1), 4)
    sc, p = lc.standard()
    try:
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        fit_before = p.linear_fit(0, 4, 6, normal=True)
        p.linear_fit_time_scan(0, 4, 6, -30, 12, 6)
        after = p.get_misfits()                               # what the scan leaves: the plain evaluation of the basis sources
        for a, b in zip(after, before):
            assert common.same_bits(a, b) if common.arith() == "exact" else common.misfit_close(
                a, b, norm=before[1] if a.ndim == 2 else None, glob=a.ndim == 1)
        p.eval()
        for a, b in zip(p.get_misfits(), before):
            assert np.array_equal(a, b)
        again = p.linear_fit(0, 4, 6, normal=True)
        for name in ("coef", "misfit", "status", "pivot_min", "normal"):
            assert np.array_equal(getattr(again, name), getattr(fit_before, name)), name
        p.linear_fit_time_scan(6, 2, 6, 0, 1, 2)              # a range inside the batch
        for a, b in zip(p.get_misfits(6, 12), before):
            assert np.all(a > 0)
            assert common.same_bits(a, b[6:18]) if common.arith() == "exact" else common.misfit_close(
                a, b[6:18], norm=before[1][6:18] if a.ndim == 2 else None, glob=a.ndim == 1)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = lc.standard()
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)

        def refused(match, scan=(0, 1, 2), K=6, ngroup=2, isrc0=0, listed=True):
            with pytest.raises(KiwiHipError, match=match):
                p.linear_fit_time_scan(isrc0, ngroup, K, *scan)
            if listed:
                with pytest.raises(KiwiHipError, match=match):
                    p.linear_fit_time_scan_params("moment_tensor", rows, K, *scan)
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)

        p.set_misfit_filter(2, *FILTER)
        refused("misfit filter")
        p.set_misfit_filter(2, [], [])
        still_usable()
        p.set_misfit_method("l1norm")
        refused("l2norm")
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(1, -1.0, 1.0)
        refused("floating")
        p.set_misfit_method("l2norm")
        still_usable()
        with pytest.raises(KiwiHipError, match="basis sources per group"):
            p.linear_fit_time_scan(0, 1, 9, 0, 1, 2)
        from kiwi_amd.lib import c_double_p, c_int_p
        buf, ibuf = np.zeros(1024), np.zeros(64, np.int32)
        rc = p.L.kiwi_hip_linear_fit_time_scan(p.h, 0, 1, 9, 0, 1, 2, None, 0, buf.ctypes.data_as(c_double_p), buf.ctypes.data_as(c_double_p),
                                               ibuf.ctypes.data_as(c_int_p), None, None, None)
        assert rc != 0
        with pytest.raises(KiwiHipError, match="basis sources per group"):
            p._ck(rc, "linear_fit_time_scan")
        refused("need at least one offset", scan=(0, 1, 0))
        refused("257 offsets; at most 256", scan=(-128, 1, 257))
        refused("kstep = 0", scan=(0, 0, 3))
        refused(r"offsets 1025 \.\. 1025 samples; the largest shift is 1024", scan=(1025, 1, 1))
        refused("the largest shift is 1024", scan=(-1025, 1, 2))
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            refused("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, listed=False)
        still_usable()
        fit = p.linear_fit_time_scan(0, 2, 6, -1024, 2048, 2)  # the largest shift either way
        assert fit.status.shape == (2, 2)
        still_usable()
    finally:
        p.close()
    # an enabled receiver without a taper
    from tests.common import Scenario
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[2]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.linear_fit_time_scan(0, 2, 6, 0, 1, 2)
        p.eval()
        assert np.all(p.get_misfits()[0] > 0)
        p.switch_receiver(2, False)                           # disabled: it does not matter any more
        assert np.all(p.linear_fit_time_scan(0, 2, 6, 0, 1, 2).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 8: the moment-tensor helper
def _planted_later(sc_kw=None, shift=2):
    """(scenario, engine) whose references are the planted tensor `shift` samples later than the rows the tests fit"""
    from tests.common import Scenario
    probe = Scenario()
    dt = probe.gf["dt"]
    true_row = mt_row(PLANTED, location=[shift * dt, 0., 0., 10000.])
    sc = Scenario(true_type=6, true_params=true_row, **(sc_kw or {}))
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    return sc, p, dt


def test_planted_tensor_at_a_planted_offset_through_fit_moment_tensors_time_scan():
    sc, p, dt = _planted_later()
    try:
        rows = np.stack([mt_row(np.zeros(6)), mt_row(np.ones(6), location=[0., 800., -500., 11000.])])
        tensors, misfit, status, pivot, best = mtfit.fit_moment_tensors_time_scan(p, "moment_tensor", rows, -3, 1, 8)
        assert tensors.shape == (2, 8, 6) and misfit.shape == status.shape == pivot.shape == (2, 8)
        assert np.all(status == 0) and best[0] == 5            # offsets -3 .. 4: +2 is index 5
        rel = np.abs(tensors[0, 5] - PLANTED) / np.abs(PLANTED)
        print("planted tensor at offset +2: relative error", rel, "misfits over the offsets", misfit[0], "pivot_min", pivot[0])
        assert np.all(rel <= 1e-5) and misfit[0, 5] <= 1e-5
        assert np.all(np.delete(misfit[0], 5) > 100 * misfit[0, 5]) and misfit[1].min() > 10 * misfit[0, 5]
        dev, dmis, dstatus, dpiv, dbest = mtfit.fit_moment_tensors_time_scan(p, "moment_tensor", rows, -3, 1, 8, deviatoric=True)
        assert np.all(dstatus == 0) and np.all(np.abs(dev[..., :3].sum(-1)) <= 1e-12 * np.abs(dev).max(-1))
        assert np.all(dmis >= misfit) and dbest.shape == (2,)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 9: the grid
def test_grid_search_over_depth_and_time_with_a_free_tensor_per_node():
    from tests.common import Scenario
    dt = Scenario().gf["dt"]
    true_row = mt_row(PLANTED, location=[2 * dt, 0., 0., 11000.])
    sc = Scenario(true_type=6, true_params=true_row)
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        times = dt * np.arange(-2, 5)
        grid = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("depth", [10000., 11000., 12000.]), ("time", times)])
        assert len(grid.sources) == 21
        grid.compute_mt_time_scan(p)
        best = grid.best_source
        print("grid: best node", best[:4], "misfit", grid.fit_misfits[grid.ibest], "second best", np.sort(grid.fit_misfits)[1])
        assert grid.syntheses_saved == 6 * 18
        assert best[3] == 11000.0 and best[0] == np.float32(2 * dt)
        assert np.all(np.abs(best[4:10] - PLANTED) <= 1e-5 * np.abs(PLANTED))
        assert np.all(grid.fit_status == 0) and grid.fit_misfits[grid.ibest] <= 1e-5
        assert np.sort(grid.fit_misfits)[1] > 100 * grid.fit_misfits[grid.ibest]
        # the fitted sources evaluated like any grid: the row at ibest reproduces the fit's misfit
        g, _ = gridsearch.make_global_misfits(grid.misfits_by_src, grid.norms_by_src, receiver_mask=grid.receiver_mask)
        print("grid: evaluated fitted source %.3g, fit %.3g" % (g[grid.ibest], grid.fit_misfits[grid.ibest]))
        assert abs(g[grid.ibest] - grid.fit_misfits[grid.ibest]) <= 1e-5 and int(np.nanargmin(g)) == grid.ibest
        grid.postprocess(bootstrap_iterations=20, rng=np.random.default_rng(0))
        assert grid.ibest == int(np.argmin(grid.fit_misfits)) and grid.stats["depth"].best == 11000.0
        assert grid.stats["time"].best == float(np.float32(2 * dt))
        lean = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("depth", [10000., 11000., 12000.]), ("time", times)])
        lean.compute_mt_time_scan(p, evaluate_fitted=False)
        assert lean.misfits_by_src is None and lean.ibest == grid.ibest
        with pytest.raises(ValueError, match="exactly one `time` axis"):
            gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("depth", [10000.])]).compute_mt_time_scan(p)
        with pytest.raises(ValueError, match="not evenly spaced by a whole number of samples"):
            gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("time", [0.0, 0.3 * dt])]).compute_mt_time_scan(p)
        with pytest.raises(ValueError, match="linear_mt"):
            grid.compute(p, time_scan=True, linear_mt=True)    # compute() itself is as it was
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 10: the example
def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith(), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_moment_tensor_timescan.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted node found" in out.stdout and "syntheses saved" in out.stdout, out.stdout
