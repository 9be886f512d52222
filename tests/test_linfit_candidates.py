"""kiwi_hip_linear_fit_candidates without a device: the numpy restatement of the device arithmetic
(tests/linfit_candidates_restatement.py) against the truth formed directly from the CPU oracle's traces, against the existing
restatements bit for bit, its rules for the best candidate, the double-couple grid of kiwi_amd/mtfit.py, and the plumbing of the
new entry points.  The device is pinned to the restatement bit for bit in tests/test_linfit_candidates_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import lib as klib, mtfit, synthetic
from tests import linfit_candidates_restatement as cr
from tests import linfit_restatement as lr
from tests import linfit_robust_restatement as rr
from tests.common import Scenario
from tests.linfit_cases import PLANTED, UNIT, basis_rows, mt_row, oracle_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_linear_fit_candidates", "kiwi_hip_linear_fit_candidates_params", "kiwi_hip_get_linear_fit_candidates_ms",
           "kiwi_hip_linear_fit_candidates_shape"]
DT = 0.5
U = 2.0 ** -52


def random_case(rng, K, nrec, nslot, wlen, ngroup=1, noise=0.05):
    """(syn, ref, receivers): smooth random basis traces, references = a combination of group 0's + noise"""
    planted = rng.uniform(0.5, 2.0, K) * rng.choice([-1.0, 1.0], K)
    syn, ref, receivers, m = [], [], [], 0
    for r in range(nrec):
        receivers.append(list(range(m, m + nslot)))
        for _ in range(nslot):
            s = np.cumsum(rng.standard_normal((ngroup, K, wlen)), 2).astype(np.float32) * np.float32(1.0 + r)
            d = np.zeros(wlen)
            for i in range(K):
                d = d + planted[i] * s[0, i].astype(np.float64)
            syn.append(s)
            ref.append((d + noise * np.std(d) * rng.standard_normal(wlen)).astype(np.float32))
            m += 1
    return syn, ref, receivers


def test_restated_quadratic_form_against_the_residual_formed_directly():
    """Per receiver and candidate, the restated val_r = max((R_r - 2 x.b_r) + x.G_r.x, 0) against dt sum_t (sum_i x_i s_i[t] -
    d[t])^2 formed directly from the oracle's traces in extended precision (products of fp32 values and their sums carry 64 bits
    there: its own error is 2^-11 of the bound below).

    The bound, from the number of rounded operations a term passes through.  The expansion of the square is exact:
    dt sum_t (x.s - d)^2 = R_r - 2 sum_i x_i b_i + sum_ij x_i G_ij x_j with the exact sums.  The products s_i s_j, s_i d, d d are
    exact in fp64.  An entry of (G_r, b_r, R_r) is summed by linfit_gram_kernel: a thread adds its ceil(T / 256) samples of every
    slot in turn (n_seq = sum over the slots of ceil(wlen / 256) additions), the tree adds 6 + 2 levels, and the total is multiplied
    by dt: n_seq + 9 roundings.  The evaluation multiplies an entry by x_j and adds it into a row (K additions at most), multiplies
    the row by x_i and adds it into x.G.x (K additions at most): 2 + 2 K roundings; x.b has fewer; 2 x.b is exact; the last two
    additions: 2.  To first order every term of the expansion is therefore off by at most P u of its size with
    P = n_seq + 2 K + 13 and u = 2^-52, and val by at most
        P u (R_r + 2 sum_i |x_i b_i| + sum_ij |x_i G_ij x_j|)
    (the sizes of the terms as the sums give them).  The factor 1.01 covers the higher orders (P u < 1e-12).  The clamp at 0 only
    moves val towards the direct value, which is never negative."""
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    sc.apply_setup(e, True)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(PLANTED)), 6)
    e.close()
    K, dt = 6, sc.gf["dt"]
    nbr = lr.gram_by_receiver(syn, ref, receivers, dt)
    fit = lr.solve(nbr, K)
    rng = np.random.default_rng(5)
    cand = np.concatenate([PLANTED.astype(np.float64)[None, :] / UNIT, rng.uniform(-8.0, 8.0, (24, K))], 0)
    out = cr.evaluate(nbr, fit["normal"], None, False, cand, "l1norm")
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    dt_l = np.longdouble(np.float32(dt))
    worst = 0.0
    for r, slots in enumerate(receivers):
        n_seq = sum((len(ref[m]) + lr.THREADS - 1) // lr.THREADS for m in slots)
        P = n_seq + 2 * K + 13
        q = nbr[0, r]
        for c in range(len(cand)):
            direct = np.longdouble(0.0)
            for m in slots:
                res = -np.asarray(ref[m], np.longdouble)
                for i in range(K):
                    res = res + np.longdouble(cand[c, i]) * np.asarray(syn[m][0, i], np.longdouble)
                for t in range(len(res)):
                    direct = direct + res[t] * res[t]
            direct = float(dt_l * direct)
            size = q[NN - 1]
            for i in range(K):
                size += 2.0 * abs(cand[c, i] * q[NG + i])
                for j in range(K):
                    size += abs(cand[c, i] * q[lr.tri(K, min(i, j), max(i, j))] * cand[c, j])
            bound = 1.01 * P * U * size
            err = abs(out["receiver_val"][0, c, r] - direct)
            worst = max(worst, err / bound)
            assert err <= bound, (r, c, out["receiver_val"][0, c, r], direct, bound)
    print("restated quadratic form against the direct residual: largest error / bound %.3g" % worst)
    # the planted tensor is the best of these candidates, and nothing is left of the data under it
    assert out["best_index"][0] == 0 and out["best_misfit"][0] <= 1e-5 and np.all(out["misfit"][0, 1:] > 100 * out["misfit"][0, 0])


@pytest.mark.parametrize("anarchy", [False, True])
def test_the_fits_own_coefficients_give_the_existing_restatements_bits(anarchy):
    rng = np.random.default_rng(13)
    K, ngroup = 5, 3
    syn, ref, receivers = random_case(rng, K, 5, 2, 130, ngroup=ngroup, noise=0.4)
    w = np.array([1.0, 0.0, 2.0, 0.3, 1.5])
    start = lr.fit(syn, ref, receivers, DT, w, anarchy)
    assert np.all(start["status"] == 0)
    others = rng.uniform(-2.0, 2.0, (3, K))
    cand = np.concatenate([others[:1], start["coef"], others[1:]], 0)           # group g's coefficients are candidate 1 + g
    l2 = cr.evaluate(start["by_receiver"], start["normal"], w, anarchy, cand, "l2norm")
    l1 = cr.evaluate(start["by_receiver"], start["normal"], w, anarchy, cand, "l1norm")
    robust = rr.fit(syn, ref, receivers, DT, "B", w, anarchy, 0, 1e-3)
    for g in range(ngroup):
        assert l2["misfit"][g, 1 + g] == start["misfit"][g]                        # linfit_solve_kernel's misfit expression
        assert l1["misfit"][g, 1 + g] == robust["misfit"][g] == robust["trace"][g, 0, 1]      # iterate 0 of mode B
        assert l2["best_index"][g] == 1 + g                                        # the l2 minimum is the fit's
    assert np.all(l2["status"] == 0) and np.all(l1["status"] == 0)
    assert np.all(l1["receiver_misfit"][:, :, 1] == 0) and np.all(l1["receiver_norm"][:, 1] == 0)       # weight 0: skipped


def _sums(K, rows):
    """[1, nrec, NN] sums with G = identity, b and R as given per receiver: val = R - 2 x.b + x.x"""
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    nbr = np.zeros((1, len(rows), NN))
    for r, (b, R) in enumerate(rows):
        for i in range(K):
            nbr[0, r, lr.tri(K, i, i)] = 1.0
        nbr[0, r, NG:NG + K] = b
        nbr[0, r, NN - 1] = R
    return nbr


def test_the_best_candidate_ties_nan_and_no_data():
    K = 2
    nbr = _sums(K, [([1.0, 0.0], 4.0), ([0.0, 1.0], 4.0)])
    normal = lr.solve(nbr, K)["normal"]
    # (1, 0) and (0, 1) are mirror images under both norms; (3, 3) is worse: the tie goes to the lowest index
    cand = np.array([[3.0, 3.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    for norm in ("l1norm", "l2norm"):
        out = cr.evaluate(nbr, normal, None, False, cand, norm)
        assert out["misfit"][0, 1] == out["misfit"][0, 2] == out["misfit"][0, 3] < out["misfit"][0, 0]
        assert out["best_index"][0] == 1 and out["best_misfit"][0] == out["misfit"][0, 1] and out["status"][0] == 0
    # a direction with u.G.u = 0 answers NaN and is passed over, also in first place; all NaN: no best candidate
    out = cr.evaluate(nbr, normal, None, False, np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 0.0]]), "l2norm", True)
    assert np.isnan(out["misfit"][0, 0]) and np.isnan(out["scale"][0, 2]) and out["best_index"][0] == 1
    assert np.all(np.isnan(out["receiver_misfit"][0, 0])) and np.all(np.isfinite(out["receiver_misfit"][0, 1]))
    out = cr.evaluate(nbr, normal, None, False, np.zeros((2, 2)), "l2norm", True)
    assert out["best_index"][0] == -1 and np.isnan(out["best_misfit"][0]) and out["status"][0] == 0
    assert cr.first_minimum(np.array([np.nan, 2.0, 1.0, 1.0, np.nan])) == (2, 1.0)
    # every receiver skipped (weight 0, or no reference energy): status 1, NaN, no best candidate, zeros per receiver
    for weights, sums in ((np.zeros(2), nbr), (None, _sums(K, [([0.0, 0.0], 0.0), ([0.0, 0.0], 0.0)]))):
        folded = lr.solve(sums, K, weights)["normal"]
        for norm in ("l1norm", "l2norm"):
            out = cr.evaluate(sums, folded, weights, False, cand, norm)
            assert out["status"][0] == 1 and out["best_index"][0] == -1 and np.all(np.isnan(out["misfit"]))
            assert np.all(out["receiver_misfit"] == 0) and np.all(out["receiver_norm"] == 0)


def test_free_scale_is_a_second_evaluation_at_the_scaled_direction():
    rng = np.random.default_rng(17)
    K = 6
    syn, ref, receivers = random_case(rng, K, 4, 2, 90, ngroup=2, noise=0.3)
    w = np.array([1.0, 2.0, 0.5, 1.5])
    start = lr.fit(syn, ref, receivers, DT, w, True)
    u = rng.uniform(-1.0, 1.0, (9, K))
    u[4] = -u[3]                                                       # the opposite mechanism: the same misfit, the scale negated
    free = cr.evaluate(start["by_receiver"], start["normal"], w, True, u, "l2norm", True)
    assert np.all(np.isfinite(free["scale"])) and np.array_equal(free["scale"][:, 4], -free["scale"][:, 3])
    assert np.array_equal(free["misfit"][:, 4], free["misfit"][:, 3]) and np.all(free["best_index"] != 4)
    for g in range(2):
        again = cr.evaluate(start["by_receiver"][g:g + 1], start["normal"][g:g + 1], w, True, free["scale"][g][:, None] * u, "l2norm")
        assert np.array_equal(again["misfit"][0], free["misfit"][g])
        assert np.array_equal(again["receiver_misfit"][0], free["receiver_misfit"][g])
        assert again["best_index"][0] == free["best_index"][g]
        # the scale is the minimum along the direction: a step either way does not fit better
        for f in (0.99, 1.01):
            moved = cr.evaluate(start["by_receiver"][g:g + 1], start["normal"][g:g + 1], w, True, f * free["scale"][g][:, None] * u, "l2norm")
            assert np.all(moved["misfit"][0] >= free["misfit"][g])
    # no candidate of any scale beats the free fit
    assert np.all(free["misfit"] >= start["misfit"][:, None])


def test_double_couple_candidates_are_the_grid_of_the_benchmark():
    """Against the tensor columns of synthetic.mt_sdr_grid (float32): half an fp32 ulp of the column's value for its rounding,
    plus 16 fp64 ulps of the moment for the two evaluations' own fp64 roundings (a dozen operations on values <= the moment)"""
    grid = synthetic.mt_sdr_grid()
    cand, sdr = mtfit.double_couple_candidates(range(0, 360, 10), range(0, 91, 10), range(-180, 180, 10), 7e18)
    assert cand.shape == (12960, 6) and cand.dtype == np.float64 and sdr.shape == (12960, 3)
    cols = grid[:, 4:10].astype(np.float64)
    assert np.all(np.abs(cand - cols) <= 2.0 ** -24 * np.abs(cols) + 16 * U * 7e18)
    assert list(sdr[0]) == [0, 0, -180] and list(sdr[1]) == [0, 0, -170] and list(sdr[36]) == [0, 10, -180] and list(sdr[-1]) == [350, 90, 170]
    for n in (0, 777, 12959):
        assert np.allclose(cand[n], synthetic.mt_from_sdr(*sdr[n], 7e18), rtol=0, atol=16 * U * 7e18)
    assert mtfit.COMPONENTS == ("mxx", "myy", "mzz", "mxy", "mxz", "myz")
    unit, _ = mtfit.double_couple_candidates([30.], [60.], [-90.])
    assert abs(np.sqrt((np.sum(unit[0, :3] ** 2) + 2 * np.sum(unit[0, 3:] ** 2)) / 2.0) - 1.0) <= 8 * U       # scalar moment 1


def test_symbols_are_exported_mapped_declared_in_the_ctypes_table_and_bound_in_fortran():
    L = klib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", klib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in dyn.splitlines() if line.strip())
    text = open(os.path.join(ROOT, "kiwi_amd", "csrc", "kiwi_hip.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    globs = re.search(r"global:(.*?);\s*local:", text, re.S).group(1).replace(";", " ").split()
    declared = klib.declared_symbols()
    header = open(os.path.join(ROOT, "include", "kiwi_hip.h")).read()
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for s in SYMBOLS:
        assert s in exported, s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        assert s in declared and re.search(r"\bint %s\(" % s, header), s
        f = getattr(L, s)
        assert f.restype is C.c_int and f.argtypes is not None, s
        assert "name='%s'" % s in binding, s
    assert len(L.kiwi_hip_linear_fit_candidates.argtypes) == 19 and len(L.kiwi_hip_linear_fit_candidates_params.argtypes) == 21
    assert L.kiwi_hip_get_linear_fit_candidates_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_linear_fit_candidates_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    shapes = set()
    for K in range(1, kmax + 1):
        c, s = C.c_int(), C.c_int()
        assert L.kiwi_hip_linear_fit_candidates_shape(K, C.byref(c), C.byref(s)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and s.value >= 1
        assert s.value * lr.nn_of(K) * 8 <= 160 * 1024                          # a stage of rows fits the LDS of a workgroup
        shapes.add((c.value, s.value))
    assert len(shapes) == 1
    c, s = C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_linear_fit_candidates_shape(K, C.byref(c), C.byref(s)) != 0
    assert L.kiwi_hip_linear_fit_candidates_shape(6, None, C.byref(s)) != 0
