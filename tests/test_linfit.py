"""kiwi_hip_linear_fit without a device: the numpy restatement of the device arithmetic (tests/linfit_restatement.py) on the
ORACLE's tapered traces -- does the linear model hold through the whole pipeline, does the fit find a planted tensor, does
it predict the misfits an evaluation of the fitted tensor gives, what do degenerate groups answer -- and the plumbing of
the new entry points (header, export map, loader, Fortran binding).  The device is pinned to the restatement bit for bit
in tests/test_linfit_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from kiwi_amd import lib as klib
from kiwi_amd import mtfit
from tests import linfit_restatement as lr
from tests.common import Scenario, misfit_close
from tests.linfit_cases import LOCATION, PLANTED, UNIT, basis_rows, mt_row, oracle_traces, slots_as_receivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(sc):
    e = sc.oracle()
    sc.make_references(e)
    sc.apply_setup(e, True)
    return e


def test_planted_tensor_comes_back_and_matches_lstsq():
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = _oracle(sc)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(PLANTED)), 6)
    out = lr.fit(syn, ref, receivers, sc.gf["dt"])
    assert out["status"][0] == 0
    tensor = out["coef"][0] * UNIT
    rel = np.abs(tensor - PLANTED.astype(np.float64)) / np.abs(PLANTED.astype(np.float64))
    print("planted tensor: relative error per component", rel, "misfit", out["misfit"][0], "pivot_min", out["pivot_min"][0])
    assert np.all(rel <= 1e-5)
    # against numpy's least squares on the stacked traces: the normal equations lose cond(G) eps
    A = np.concatenate([s[0].astype(np.float64).T for s in syn], 0)
    d = np.concatenate([r.astype(np.float64) for r in ref])
    x = np.linalg.lstsq(A, d, rcond=None)[0]
    G, _, _ = lr.full_matrix(out["normal"][0], 6)
    cond = np.linalg.cond(G)
    bound = 8.0 * cond * 6 * 2.0 ** -52
    err = np.max(np.abs(out["coef"][0] - x)) / np.max(np.abs(x))
    print("cond(G) %.2f, restatement vs lstsq %.3g, bound %.3g" % (cond, err, bound))
    assert err <= bound
    assert out["misfit"][0] <= 1e-5                      # (the residual is round-off of the fp32 pipeline: 1e-7 seen)


def test_fitted_tensor_predicts_the_oracles_misfits_for_bilateral_data(monkeypatch):
    sc = Scenario()                                      # data: the default bilateral rupture
    e = _oracle(sc)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(PLANTED)), 6)
    out = lr.fit(syn, ref, receivers, sc.gf["dt"])
    assert out["status"][0] == 0 and out["pivot_min"][0] > 0.5
    fitted = (out["coef"][0] * UNIT).astype(np.float32)
    e.set_source_params(6, mt_row(fitted))
    m, n, g = e.get_misfits()
    # what the quadratic form predicts for the tensor the oracle was given (the fp32 rounding of the parameters included)
    coef = fitted.astype(np.float64) / UNIT
    per_slot = lr.gram_by_receiver(syn, ref, slots_as_receivers(receivers), sc.gf["dt"])[0]
    pm = lr.predicted_slot_misfits(per_slot, coef)
    print("slots: worst |predicted - oracle| / max(misfit, norm) %.3g; global predicted %.9f oracle %.9f" % (
        np.max(np.abs(pm - m) / np.maximum(m, n)), out["misfit"][0], g))
    monkeypatch.setenv("KIWI_HIP_ARITH", "fused")        # the rule on the scale of the norm factors (tests/common.py)
    assert misfit_close(pm, m, norm=n)
    assert misfit_close(out["misfit"][0], g, glob=True)
    rng = np.random.default_rng(5)
    for _ in range(20):
        other = (fitted * (1.0 + 0.05 * rng.standard_normal(6))).astype(np.float32)
        e.set_source_params(6, mt_row(other))
        assert e.get_misfits()[2] >= g


def test_degenerate_groups():
    comps = ["d", "ned", "ned", "ned", "ned", "ned"]
    sc = Scenario(comps_list=comps)
    e = _oracle(sc)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(PLANTED)), 6)
    dt = sc.gf["dt"]
    # every slot: well conditioned
    out = lr.fit(syn, ref, receivers, dt)
    print("all slots: pivot_min %.3f" % out["pivot_min"][0])
    assert out["status"][0] == 0 and out["pivot_min"][0] > 0.5
    # a weighting that leaves one vertical slot: the tensor acts through four combinations only, rank 4
    w = np.zeros(6)
    w[0] = 1.0
    one = lr.fit(syn, ref, receivers, dt, weights=w)
    print("single vertical slot: status %d pivot_min %.3g" % (one["status"][0], one["pivot_min"][0]))
    assert one["status"][0] == 1 or one["pivot_min"][0] < 1e-9
    if one["status"][0] == 1:
        assert np.all(np.isnan(one["coef"][0])) and np.isnan(one["misfit"][0])
    # K = 2, one basis source all zero: zero diagonal
    two = [np.stack([s[:, 0], np.zeros_like(s[:, 0])], 1) for s in syn]
    z = lr.fit(two, ref, receivers, dt)
    assert z["status"][0] == 1 and z["pivot_min"][0] == 0.0
    assert np.all(np.isnan(z["coef"][0])) and np.isnan(z["misfit"][0])
    assert np.all(np.isfinite(z["normal"][0])) and z["normal"][0][lr.tri(2, 1, 1)] == 0.0
    # two identical basis sources
    same = [np.stack([s[:, 0], s[:, 0]], 1) for s in syn]
    t = lr.fit(same, ref, receivers, dt)
    print("identical basis sources: status %d pivot_min %.3g" % (t["status"][0], t["pivot_min"][0]))
    assert t["status"][0] == 1 or t["pivot_min"][0] < 1e-9
    # no data: R = 0
    r0 = lr.fit(syn, [np.zeros_like(r) for r in ref], receivers, dt)
    assert r0["status"][0] == 1 and np.isnan(r0["misfit"][0])
    # anarchy: a receiver without data has weight 0 and the others are divided by their norms
    ref2 = [r.copy() for r in ref]
    ref2[0][:] = 0.0
    a = lr.fit(syn, ref2, receivers, dt, anarchy=True)
    nbr = lr.gram_by_receiver(syn, ref2, receivers, dt)
    wa = np.array([0.0] + [1.0 / np.sqrt(nbr[0, r, -1]) for r in range(1, 6)])
    b = lr.solve(nbr, 6, wa, False)
    assert a["status"][0] == 0 and np.allclose(a["coef"], b["coef"], rtol=1e-12, atol=0)


def test_elementary_params_and_deviatoric():
    rows = np.arange(22, dtype=np.float32).reshape(2, 11)
    el = mtfit.elementary_params("moment_tensor", rows, unit=2.0)
    assert el.shape == (12, 11) and el.dtype == np.float32
    assert np.array_equal(el[:, 4:10], np.tile(2.0 * np.eye(6, dtype=np.float32), (2, 1)))
    assert np.array_equal(el[:6, [0, 1, 2, 3, 10]], np.tile(rows[0, [0, 1, 2, 3, 10]], (6, 1)))
    assert np.array_equal(el[6:, [0, 1, 2, 3, 10]], np.tile(rows[1, [0, 1, 2, 3, 10]], (6, 1)))
    rows = np.arange(20, dtype=np.float32)[None, :]
    el = mtfit.elementary_params("mt_eikonal", rows)
    assert el.shape == (6, 20)
    assert np.array_equal(el[:, 13:19], np.float32(1e18) * np.eye(6, dtype=np.float32))
    keep = [c for c in range(20) if not 13 <= c < 19]
    assert np.array_equal(el[:, keep], np.tile(rows[:, keep], (6, 1)))
    for st in ("bilateral", "circular", "eikonal", "point_lp"):
        with pytest.raises(klib.KiwiHipError):
            mtfit.elementary_params(st, np.zeros((1, 14)))
    # the trace-free problem from the normal equations of the default scenario
    sc = Scenario()
    e = _oracle(sc)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(PLANTED)), 6)
    out = lr.fit(syn, ref, receivers, sc.gf["dt"])
    x, mis, st, piv = mtfit.solve_deviatoric(out["normal"][0])
    print("deviatoric: trace %.3g of %.3g, misfit %.9f (free %.9f), pivot %.3f" % (x[:3].sum(), np.abs(x).max(), mis, out["misfit"][0], piv))
    assert st == 0 and piv > 0.1
    assert abs(x[:3].sum()) <= 16 * 2.0 ** -52 * np.abs(x).max()
    assert mis >= out["misfit"][0]
    assert np.allclose(mtfit.DEVIATORIC_BASIS.T @ mtfit.DEVIATORIC_BASIS, np.eye(5), atol=1e-15)
    assert np.allclose(mtfit.DEVIATORIC_BASIS[:3].sum(0), 0.0, atol=1e-15)


def test_entry_points_are_declared_exported_loaded_and_bound():
    L = klib.load()
    assert L.kiwi_hip_linear_fit_max_basis() == 8                       # answers without a device
    names = ["kiwi_hip_linear_fit", "kiwi_hip_linear_fit_params", "kiwi_hip_linear_fit_max_basis", "kiwi_hip_get_linear_fit_ms"]
    declared = klib.declared_symbols()
    raw = C.CDLL(klib.LIB_PATH)
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for name in names:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
        assert "name='%s'" % name in binding, name
    assert len(L.kiwi_hip_linear_fit.argtypes) == 12 and len(L.kiwi_hip_linear_fit_params.argtypes) == 14
