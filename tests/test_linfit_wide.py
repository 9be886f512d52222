"""kiwi_hip_linear_fit_wide without a device: the numpy restatement of the device arithmetic
(tests/linfit_wide_restatement.py) against scipy's non-negative least squares on random problems of strongly overlapping
wavelets, what it answers for dependent columns, the helpers of kiwi_amd/slipfit.py, and the plumbing of the new entry points
(header, export map, loader, Fortran binding).  The device is pinned to the restatement bit for bit in
tests/test_linfit_wide_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.optimize

from kiwi_amd import lib as klib
from kiwi_amd import slipfit, synthetic
from tests import linfit_restatement as lr
from tests import linfit_wide_restatement as lw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.5
WEIGHTS = np.array([1.0, 2.5, 0.7])
SHAPES = {5: (1, 5, 1, 1), 17: (1, 17, 1, 1), 64: (4, 4, 2, 2)}      # (ny, nx, nrake, nwin) of the penalty


def wavelet_problem(K, seed, wlen=300, noise=0.05):
    """three receivers of one slot each; basis: Ricker-like wavelets 0.35 widths apart (strongly overlapping), fp32; data: a
    non-negative combination with zeros plus `noise` of its RMS.  (syn, ref, receivers, true x)"""
    rng = np.random.default_rng(seed)
    t = np.arange(wlen)[None, :]
    syn, ref = [], []
    x = np.where(rng.uniform(size=K) < 0.5, 0.0, rng.uniform(0.5, 2.0, K))
    x[0] = 1.0
    width = 12.0
    for _ in range(3):
        c = 40.0 + rng.uniform(-3, 3) + 0.35 * width * np.arange(K)[:, None] * (200.0 / max(0.35 * width * K, 200.0))
        u = (t - c) / width
        s = ((1.0 - 2.0 * u * u) * np.exp(-u * u) * rng.uniform(0.5, 1.5, (K, 1))).astype(np.float32)
        d = x @ s.astype(np.float64)
        d = d + noise * np.sqrt(np.mean(d * d)) * rng.standard_normal(wlen)
        syn.append(s[None])
        ref.append(d.astype(np.float32))
    return syn, ref, [[0], [1], [2]], x


def trace_matrix(syn, ref, weights):
    """the weighted stacked traces: |W (d - S x)|^2 is the quadratic form of the folded sums"""
    S = np.concatenate([weights[m] * np.sqrt(DT) * syn[m][0].astype(np.float64).T for m in range(len(syn))], 0)
    d = np.concatenate([weights[m] * np.sqrt(DT) * ref[m].astype(np.float64) for m in range(len(ref))])
    return S, d


def penalty_factor(P, K, lam):
    """F with F^T F = lam P (P is only semi-definite: the symmetric root from its eigenvectors stands in for a Cholesky factor)"""
    full = np.zeros((K, K))
    full[np.triu_indices(K)] = P
    full = full + np.triu(full, 1).T
    ev, V = np.linalg.eigh(lam * full)
    return (V * np.sqrt(np.clip(ev, 0.0, None))) @ V.T, lam * full


def test_entry_points_are_declared_exported_loaded_and_bound():
    L = klib.load()
    assert L.kiwi_hip_linear_fit_wide_max_basis() == 64                 # answers without a device
    assert L.kiwi_hip_linear_fit_max_basis() == 8                       # the narrow fit keeps its limit
    names = ["kiwi_hip_linear_fit_wide", "kiwi_hip_linear_fit_wide_params", "kiwi_hip_linear_fit_wide_max_basis",
             "kiwi_hip_get_linear_fit_wide_ms"]
    declared = klib.declared_symbols()
    raw = C.CDLL(klib.LIB_PATH)
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for name in names:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
        assert "name='%s'" % name in binding, name
    assert len(L.kiwi_hip_linear_fit_wide.argtypes) == 17 and len(L.kiwi_hip_linear_fit_wide_params.argtypes) == 19


@pytest.mark.parametrize("K", [1, 6, 8, 17])
def test_unconstrained_restatement_equals_the_narrow_one(K):
    syn, ref, receivers, _ = wavelet_problem(K, 10 + K)
    for anarchy in (False, True):
        a = lr.fit(syn, ref, receivers, DT, WEIGHTS, anarchy)
        b = lw.fit(syn, ref, receivers, DT, WEIGHTS, anarchy)
        for name in ("coef", "misfit", "status", "pivot_min", "normal", "by_receiver"):
            assert np.array_equal(a[name], b[name], equal_nan=True), name
        assert b["status"][0] == 0 and b["nsolves"][0] == 1 and b["npositive"][0] == np.sum(b["coef"][0] > 0)


@pytest.mark.parametrize("with_penalty", [False, True])
@pytest.mark.parametrize("K", [5, 17, 64])
def test_nonneg_restatement_against_scipy_nnls(K, with_penalty):
    """objective within 1e-10 |d| of scipy's (3e-14 seen over 300 problems), KKT conditions, at most 3 K solves"""
    worst, most = 0.0, 0
    for seed in range(4):
        syn, ref, receivers, _ = wavelet_problem(K, 100 * K + seed)
        P = slipfit.laplacian_penalty(*[SHAPES[K][i] for i in (1, 0, 2, 3)]) * 0.1 if with_penalty else None
        out = lw.fit(syn, ref, receivers, DT, WEIGHTS, False, nonneg=True, penalty=P, penalty_relative=True)
        assert out["status"][0] == 0
        x = out["coef"][0]
        S, d = trace_matrix(syn, ref, WEIGHTS)
        G, b, R = lr.full_matrix(out["normal"][0], K)
        assert np.allclose(S.T @ S, G, rtol=1e-12, atol=1e-12 * G.max()) and np.isclose(d @ d, R, rtol=1e-12)
        Gp = G
        if with_penalty:
            F, lamP = penalty_factor(P, K, np.trace(G) / K)
            Gp = G + lamP
            Sx, dx = np.concatenate([S, F], 0), np.concatenate([d, np.zeros(K)])
        else:
            Sx, dx = S, d
        xs, _ = scipy.optimize.nnls(Sx, dx, maxiter=30 * K)
        ours, theirs = np.linalg.norm(Sx @ x - dx), np.linalg.norm(Sx @ xs - dx)
        worst = max(worst, (ours - theirs) / np.linalg.norm(d))
        most = max(most, int(out["nsolves"][0]))
        assert ours - theirs <= 1e-10 * np.linalg.norm(d)
        # KKT in the scaled variables: x >= 0, and where an index is neither passive nor barred the gradient, summed in the
        # stated order, is not above the stated threshold 10 K 2^-52 max |c|
        assert np.all(x >= 0.0) and out["npositive"][0] == np.sum(x > 0.0)
        one = lw.solve_one(out["normal"][0], K, nonneg=True, penalty=P, penalty_relative=True)
        assert np.array_equal(one["coef"], x) and one["barred"] == []
        A, c, xsc = one["scaled"]
        thr = lw.nonneg_threshold(c, K)
        assert thr == 10 * K * 2.0 ** -52 * np.max(np.abs(c))
        free = [i for i in range(K) if i not in one["passive"] and i not in one["barred"]]
        assert sorted(free + one["passive"]) == list(range(K)) and np.all(xsc[free] == 0.0) and np.all(xsc[one["passive"]] > 0.0)
        w = np.array([lw.gradient(A, c, xsc, one["passive"], i) for i in range(K)])
        assert np.all(w[free] <= thr)
        # the same matrix and gradient from the traces in plain numpy (a Cholesky solve is backward stable: in the passive set
        # the residual is of the order K eps |A| |x|)
        s = 1.0 / np.sqrt(np.diag(Gp))
        assert np.allclose(A, Gp * s[:, None] * s[None, :], rtol=1e-12, atol=1e-12) and np.allclose(c, b * s, rtol=1e-12)
        slack = K * 2.0 ** -52 * (np.abs(c) + np.abs(A) @ np.abs(xsc))
        assert np.all(np.abs(w[one["passive"]]) <= 64 * slack[one["passive"]])
        assert 1 <= out["nsolves"][0] <= 3 * K
        # the misfit is the DATA misfit
        assert np.isclose(out["misfit"][0], np.linalg.norm(S @ x - d) / np.linalg.norm(d), rtol=1e-9)
    print("K=%d penalty=%s: objective above scipy's by at most %.3g |d|, at most %d solves (%.2f K)" % (K, with_penalty, worst, most, most / K))


def test_removal_branch_runs_and_planted_zeros_come_back():
    syn, ref, receivers, x0 = wavelet_problem(17, 7, noise=0.0)
    out = lw.fit(syn, ref, receivers, DT, None, False, nonneg=True)
    free = lw.fit(syn, ref, receivers, DT, None, False)
    print("noise-free K=17: nsolves %d npositive %d, planted positives %d; smallest free coefficient %.3g" % (
        out["nsolves"][0], out["npositive"][0], np.sum(x0 > 0), free["coef"][0].min()))
    assert out["status"][0] == 0 and np.all(out["coef"][0] >= 0.0)
    assert out["misfit"][0] <= free["misfit"][0] + 1e-6      # the planted non-negative combination is in reach
    noisy = wavelet_problem(17, 7, noise=0.3)
    fn = lw.fit(*noisy[:3], DT, None, False)
    on = lw.fit(*noisy[:3], DT, None, False, nonneg=True)
    assert fn["coef"][0].min() < 0.0                          # the free solution oscillates ...
    assert on["nsolves"][0] > on["npositive"][0]              # ... and the non-negative one had to take indices out again
    assert on["misfit"][0] >= fn["misfit"][0] and on["status"][0] == 0


def test_dependent_columns():
    """A column in the span of the others.  An exact copy of ONE column is never selected: once its twin is in the passive
    set its gradient is round-off (and before that the twin, of lower index, wins the tie).  A column that is the sum of two
    others can be selected while both are in (its gradient is then (rounding of the fp32 sum) . residual, of either sign): it
    fails the pivot test and is barred.  Either way: status 0, the fit of the problem without the column, and the free fit of
    the same sums is refused by its pivot"""
    syn, ref, receivers, _ = wavelet_problem(6, 4)
    base = lw.fit([s[:, :5] for s in syn], ref, receivers, DT, None, False, nonneg=True)
    for kind in ("copy", "sum"):
        dup = [s.copy() for s in syn]
        for s in dup:
            s[0, 5] = s[0, 1] if kind == "copy" else s[0, 1] + s[0, 2]
        free = lw.fit(dup, ref, receivers, DT, None, False)
        assert free["status"][0] == 1 and free["pivot_min"][0] <= 6 * 2.0 ** -52 and np.all(np.isnan(free["coef"][0]))
        N = lw.fold(lr.gram_by_receiver(dup, ref, receivers, DT))
        one = lw.solve_one(N[0], 6, nonneg=True)
        print("column 5 a %s: barred %s, coef %s, nsolves %d" % (kind, one["barred"], one["coef"], one["nsolves"]))
        assert one["status"] == 0 and np.all(one["coef"] >= 0.0)
        assert np.isclose(one["misfit"], base["misfit"][0], rtol=1e-9)
        if kind == "copy":
            assert one["barred"] == [] and one["coef"][5] == 0.0
            assert np.allclose(one["coef"][:5], base["coef"][0], rtol=1e-9)
        else:
            assert one["barred"] == [5] and one["coef"][5] == 0.0 and one["nsolves"] == one["npositive"] + 1
            assert np.allclose(one["coef"][:5], base["coef"][0], rtol=1e-6)


def test_laplacian_penalty():
    for nx, ny, nrake, nwin in ((4, 4, 2, 2), (5, 1, 1, 1), (3, 2, 1, 2)):
        K = nx * ny * nrake * nwin
        P = slipfit.laplacian_penalty(nx, ny, nrake, nwin)
        assert P.shape == (K * (K + 1) // 2,)
        full = np.zeros((K, K))
        full[np.triu_indices(K)] = P
        full = full + np.triu(full, 1).T
        ev = np.linalg.eigvalsh(full)
        assert ev.min() >= -1e-12 * ev.max() and ev.max() > 0
        assert np.all(full @ np.ones(K) == 0.0)               # constants (and a constant per layer) cost nothing
        layer = np.zeros(K)
        layer[0::nrake * nwin] = 1.0
        assert np.all(full @ layer == 0.0)
        bump = np.zeros(K)
        bump[0] = 1.0
        assert bump @ full @ bump > 0
        # layers are not tied to each other
        if nrake * nwin > 1:
            assert full[0, 1] == 0.0 and full[0, nrake * nwin] != 0.0


def test_patch_basis_rows_and_order():
    rakes = (45.0, 135.0)
    rows = slipfit.patch_basis("moment_tensor", origin=(1.0, 100.0, -200.0, 9000.0), strike=30.0, dip=60.0, rakes=rakes, nx=4, ny=3,
                               patch_length=2000.0, patch_width=1500.0, nwin=2, window=1.5, rupture_velocity=2500.0, unit=1e17)
    assert rows.shape == (4 * 3 * 2 * 2, 11) and rows.dtype == np.float32
    r = rows.reshape(3, 4, 2, 2, 11)
    # the window is fastest and shifts the time by its length; the rise time is the window
    assert np.allclose(r[..., 1, 0] - r[..., 0, 0], 1.5) and np.all(r[..., 10] == np.float32(1.5))
    # then the rake: the tensor changes, nothing else
    for ir, rake in enumerate(rakes):
        assert np.allclose(r[:, :, ir, :, 4:10], np.asarray(synthetic.mt_from_sdr(30.0, 60.0, rake, m0=1e17), np.float32))
    assert np.array_equal(r[:, :, 0, :, :4], r[:, :, 1, :, :4])
    # then along strike, then down dip: the centre of the plane is the origin, depth grows down dip only
    assert np.allclose(r[..., 1].mean(), 100.0, atol=1e-2) and np.allclose(r[..., 2].mean(), -200.0, atol=1e-2)
    assert np.allclose(r[..., 3].mean(), 9000.0, atol=1e-2)
    assert np.allclose(r[:, 1:, 0, 0, 3], r[:, :-1, 0, 0, 3]) and np.allclose(np.diff(r[:, 0, 0, 0, 3]), 1500.0 * np.sin(np.radians(60.0)))
    step = r[0, 1, 0, 0, 1:3] - r[0, 0, 0, 0, 1:3]
    assert np.allclose(step, 2000.0 * np.array([np.cos(np.radians(30.0)), np.sin(np.radians(30.0))]), atol=1e-2)
    # the delay is the distance from the origin over the rupture velocity
    dist = np.sqrt(((np.arange(4) - 1.5) * 2000.0)[None, :] ** 2 + ((np.arange(3) - 1.0) * 1500.0)[:, None] ** 2)
    assert np.allclose(r[:, :, 0, 0, 0], 1.0 + dist / 2500.0, atol=1e-5)
    with pytest.raises(klib.KiwiHipError):
        slipfit.patch_basis("bilateral")


def test_data_that_are_not_finite_have_no_nonneg_solution():
    """a scaled b_i (or matrix element) that is not finite: status 1 and NaN before the active-set loop, whose comparisons
    would not be the same in every lane of the device's wavefront"""
    syn, ref, receivers, _ = wavelet_problem(6, 3)
    ref[1][40] = np.float32(np.inf)
    out = lw.fit(syn, ref, receivers, DT, None, False, nonneg=True)
    assert out["status"][0] == 1 and out["pivot_min"][0] == 0.0 and out["nsolves"][0] == 0 and out["npositive"][0] == 0
    assert np.all(np.isnan(out["coef"][0])) and np.isnan(out["misfit"][0])
