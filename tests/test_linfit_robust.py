"""kiwi_hip_linear_fit_robust without a device: the numpy restatement of the device arithmetic
(tests/linfit_robust_restatement.py) against an independent answer -- the l1 regression solved exactly as a linear program
--, its monotone descent on the smoothed objective, what it does with gross outliers, what it forwards, and the plumbing of
the new entry points.  The device is pinned to the restatement bit for bit in tests/test_linfit_robust_gpu.py.

Bounds.  The reweighting with om = 1 / max(|e|, a) is the majorise-minimise step of the Huber function H_a, and
|e| - a / 2 <= H_a(e) <= |e|.  So the smoothed objective does not increase (up to the round-off of its own sum), and
misfit(x_n) <= objective(x_n) + gap <= objective(x_0) + gap <= misfit(x_0) + gap with gap = sum_r v_r (a_r / 2) dt T_r /
sum_r v_r D_r.  The linear program's optimum is the global minimum of the misfit, so no iterate lies below it."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.optimize import linprog

from kiwi_amd import lib as klib
from tests import linfit_restatement as lr
from tests import linfit_robust_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE_JSON = os.path.join(ROOT, "profiles", "linfit_robust_rate.json")
DT = 0.5
U = 2.0 ** -52


def random_case(rng, K, nrec, nslot, wlen, ngroup=1, noise=0.05):
    """(syn, ref, receivers, planted [K]): smooth random basis traces, references = their planted combination + noise"""
    planted = rng.uniform(0.5, 2.0, K) * rng.choice([-1.0, 1.0], K)
    syn, ref, receivers, m = [], [], [], 0
    for r in range(nrec):
        receivers.append(list(range(m, m + nslot)))
        for _ in range(nslot):
            s = np.cumsum(rng.standard_normal((ngroup, K, wlen)), 2).astype(np.float32) * np.float32(1.0 + r)
            d = (planted[None, :, None] * s[:1].astype(np.float64)).sum(1)[0]
            syn.append(s)
            ref.append((d + noise * np.std(d) * rng.standard_normal(wlen)).astype(np.float32))
            m += 1
    return syn, ref, receivers, planted


def outlier_case():
    """K = 6, 7 receivers of one slot of 100 samples; the data are the planted combination exactly (as fp32 rounds it), but
    receiver 2 is buried in noise 20 x its signal and receiver 4 carries a burst of spikes"""
    rng = np.random.default_rng(20)
    syn, ref, receivers, planted = random_case(rng, 6, 7, 1, 100, noise=0.0)
    ref[2] = (ref[2] + 20.0 * np.std(ref[2]) * rng.standard_normal(100)).astype(np.float32)
    ref[4] = ref[4].copy()
    ref[4][40:48] += np.float32(50.0 * np.std(ref[4])) * rng.choice([-1.0, 1.0], 8).astype(np.float32)
    return syn, ref, receivers, planted


def l1_problem(syn, ref, receivers, dt, weights=None, anarchy=False, g=0):
    """(A [n, K], d [n], c [n], scale): the misfit of mode A at x is sum(c |d - A x|) / scale, in plain fp64"""
    dt64 = np.float64(np.float32(dt))
    A, d, c, scale = [], [], [], 0.0
    for r, slots in enumerate(receivers):
        w = 1.0 if weights is None else float(weights[r])
        if not slots or w == 0.0:
            continue
        Dr = dt64 * sum(np.abs(np.asarray(ref[m], np.float64)).sum() for m in slots)
        v = (w / Dr if Dr > 0 else 0.0) if anarchy else w
        for m in slots:
            A.append(np.asarray(syn[m][g], np.float64).T)
            d.append(np.asarray(ref[m], np.float64))
            c.append(np.full(len(ref[m]), v * dt64))
        scale += v * Dr
    return np.concatenate(A, 0), np.concatenate(d), np.concatenate(c), scale


def l1_misfit(problem, x):
    A, d, c, scale = problem
    return float(np.sum(c * np.abs(d - A @ x)) / scale)


def lp_optimum(problem):
    """the global minimum of the l1 misfit: min c.t, -t <= d - A x <= t.  The solver's vertex is polished: an optimal vertex
    of an l1 regression interpolates K samples, so x is solved from the K samples of smallest residual in fp64, and the
    misfit is evaluated there (it can only be at or above the true minimum; the lower of the two evaluations is returned)."""
    A, d, c, scale = problem
    n, K = A.shape
    eye = np.eye(n)
    res = linprog(np.concatenate([np.zeros(K), c]), A_ub=np.block([[A, -eye], [-A, -eye]]), b_ub=np.concatenate([d, -d]),
                  bounds=[(None, None)] * K + [(0, None)] * n, method="highs")
    assert res.status == 0, res.message
    x = res.x[:K]
    idx = np.argsort(np.abs(d - A @ x))[:K]
    best = l1_misfit(problem, x)
    try:
        xv = np.linalg.solve(A[idx], d[idx])
        if l1_misfit(problem, xv) <= best:
            x, best = xv, l1_misfit(problem, xv)
    except np.linalg.LinAlgError:
        pass
    return x, best


def threshold_gap(start, receivers, ref, dt, eps, weights=None, anarchy=False, g=0):
    """eps / 2 * sum_r v_r a_r' / sum_r v_r D_r with a_r' = a_r dt T_r / eps = sqrt(R_r dt T_r)"""
    dt64 = np.float64(np.float32(dt))
    num = den = 0.0
    for r, slots in enumerate(receivers):
        w = 1.0 if weights is None else float(weights[r])
        Rr = start["by_receiver"][g, r, -1]
        if not slots or w == 0.0 or not Rr > 0:
            continue
        T = sum(len(ref[m]) for m in slots)
        Dr = dt64 * sum(np.abs(np.asarray(ref[m], np.float64)).sum() for m in slots)
        v = w / Dr if anarchy else w
        num += v * np.sqrt(Rr * dt64 * T)
        den += v * Dr
    return 0.5 * eps * num / den


def nterms(syn, K):
    """terms in the longest sum behind one trace entry: every sample of every slot, K + 2 operations each"""
    return sum(s.shape[2] for s in syn) * (K + 2)


@pytest.mark.parametrize("anarchy", [False, True])
def test_mode_a_against_the_linear_program(anarchy):
    rng = np.random.default_rng(7)
    syn, ref, receivers, planted = random_case(rng, 3, 4, 2, 40, noise=0.3)
    w = np.array([1.0, 2.0, 0.5, 1.5])
    eps, niter = 1e-3, 8
    out = rr.fit(syn, ref, receivers, DT, "A", w, anarchy, niter, eps)
    assert out["status"][0] == 0
    problem = l1_problem(syn, ref, receivers, DT, w, anarchy)
    x_lp, opt = lp_optimum(problem)
    slack = 4 * nterms(syn, 3) * U
    print("mode A, anarchy %s: LP optimum %.12f, misfit per iterate %s" % (anarchy, opt, out["trace"][0, :, 1]))
    # the restated misfit is the l1 misfit of plain numpy at the same coefficients
    assert abs(out["misfit"][0] - l1_misfit(problem, out["coef"][0])) <= slack * opt
    assert out["misfit"][0] == out["trace"][0, niter, 1]
    assert np.all(out["trace"][0, :, 1] >= opt * (1.0 - slack))
    gap = threshold_gap(out["start"], receivers, ref, DT, eps, w, anarchy)
    assert out["trace"][0, niter, 1] <= out["trace"][0, 0, 1] + gap
    assert np.all(out["trace"][0, :, 0] <= out["trace"][0, :, 1]) and np.all(out["trace"][0, :, 0] >= out["trace"][0, :, 1] - gap * (1 + slack))
    assert out["trace"][0, niter, 1] < out["trace"][0, 0, 1]            # and it did move towards the l1 minimum


@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("anarchy", [False, True])
def test_smoothed_objective_descends(mode, anarchy):
    rng = np.random.default_rng(11)
    K, ngroup = 4, 3
    syn, ref, receivers, planted = random_case(rng, K, 5, 2, 300, ngroup=ngroup, noise=0.5)
    out = rr.fit(syn, ref, receivers, DT, mode, None, anarchy, 12, 1e-3)
    assert np.all(out["status"] == 0)
    obj = out["trace"][:, :, 0]
    slack = nterms(syn, K) * U
    print("mode %s anarchy %s: objective of group 0 per iterate %s" % (mode, anarchy, obj[0]))
    assert np.all(obj[:, 1:] <= obj[:, :-1] * (1.0 + slack))
    assert np.all(obj[:, -1] < obj[:, 0])


def test_outliers_do_not_drag_the_fit_and_the_gap_to_the_optimum_is_gated():
    syn, ref, receivers, planted = outlier_case()
    eps, niter = 1e-3, 8
    err = {}
    for mode in ("A", "B"):
        out = rr.fit(syn, ref, receivers, DT, mode, None, False, niter, eps)
        assert out["status"][0] == 0
        err[mode] = np.max(np.abs(out["coef"][0] - planted))
        err["l2"] = np.max(np.abs(out["start"]["coef"][0] - planted))
        if mode == "A":
            a = out
    print("largest coefficient error: l2 %.3g, mode A %.3g, mode B %.3g" % (err["l2"], err["A"], err["B"]))
    assert err["A"] < err["l2"] and err["B"] < err["l2"]
    problem = l1_problem(syn, ref, receivers, DT)
    x_lp, opt = lp_optimum(problem)
    slack = 4 * nterms(syn, 6) * U
    assert np.all(a["trace"][0, :, 1] >= opt * (1.0 - slack))
    gap = a["misfit"][0] / opt - 1.0
    recorded = json.load(open(RATE_JSON))["restatement_gap_to_lp_optimum"]
    print("mode A misfit %.12f above the LP optimum %.12f by %.3g relative (recorded %.3g)" % (a["misfit"][0], opt, gap, recorded["relative_gap"]))
    assert recorded["eps"] == eps and recorded["niter"] == niter
    assert gap <= 10.0 * recorded["relative_gap"]


def test_forwarding_and_the_start():
    rng = np.random.default_rng(3)
    syn, ref, receivers, planted = random_case(rng, 5, 4, 2, 130, ngroup=2)
    w = np.array([1.0, 0.0, 2.0, 0.3])
    start = lr.fit(syn, ref, receivers, DT, w, True)
    for mode in ("A", "B"):
        out = rr.fit(syn, ref, receivers, DT, mode, w, True, 0, 1e-3)
        assert np.array_equal(out["coef"], start["coef"]) and np.array_equal(out["status"], start["status"])
        assert out["trace"].shape == (2, 1, 2) and np.array_equal(out["trace"][:, 0, 1], out["misfit"])
    fw = rr.forwarded(syn, ref, receivers, DT, w, True, 5)
    for name in ("coef", "misfit", "status"):
        assert np.array_equal(fw[name], start[name])
    assert np.array_equal(fw["trace"][:, 0, 0], start["misfit"]) and np.array_equal(fw["trace"][:, 0, 1], start["misfit"])
    assert np.all(np.isnan(fw["trace"][:, 1:]))
    # a group without an l2 start stays without an answer; a reweighted system that breaks down keeps the iterate before
    bad = [s.copy() for s in syn]
    for s in bad:
        s[1, 4] = s[1, 3]                                     # group 1: twice the same basis source
    for mode in ("A", "B"):
        out = rr.fit(bad, ref, receivers, DT, mode, w, False, 3, 1e-3)
        assert out["status"][0] == 0 and np.all(np.isfinite(out["trace"][0]))
        assert out["status"][1] in (1, 3)
        if out["status"][1] == 1:
            assert np.all(np.isnan(out["coef"][1])) and np.all(np.isnan(out["trace"][1]))
        else:
            assert np.all(np.isfinite(out["coef"][1])) and np.isfinite(out["misfit"][1])


def test_entry_points_are_declared_exported_loaded_and_bound():
    L = klib.load()
    names = ["kiwi_hip_linear_fit_robust", "kiwi_hip_linear_fit_robust_params", "kiwi_hip_get_linear_fit_robust_ms"]
    declared = klib.declared_symbols()
    raw = C.CDLL(klib.LIB_PATH)
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for name in names:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
        assert "name='%s'" % name in binding, name
    assert len(L.kiwi_hip_linear_fit_robust.argtypes) == 13 and len(L.kiwi_hip_linear_fit_robust_params.argtypes) == 15
