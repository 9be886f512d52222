"""kiwi_hip_linear_fit_candidates_time_scan without a device: the folds over the offsets of the numpy restatement
(tests/linfit_candidates_timescan_restatement.py) on sums made by hand, the yardstick of the GPU tests on the CPU oracle -- the
candidates on the sums of basis sources moved by k samples (route A) give the bits of the candidates on the sums with references
and tapers moved by -k samples (route B) --, a planted double couple at a planted offset, and the plumbing of the new entry
points.  The device is pinned to the restatement bit for bit in tests/test_linfit_candidates_timescan_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib, mtfit, synthetic
from tests import linfit_candidates_restatement as cr
from tests import linfit_candidates_timescan_restatement as ctr
from tests import linfit_restatement as lr
from tests import linfit_timescan_restatement as ltr
from tests.common import Scenario
from tests.linfit_cases import UNIT, mt_row, oracle_traces, receivers_of
from tests.test_linfit_timescan import COMPS, KS, LOCATION, WINDOW, _basis, _fresh, _raw_rows, _scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_linear_fit_candidates_time_scan", "kiwi_hip_linear_fit_candidates_time_scan_params",
           "kiwi_hip_get_linear_fit_candidates_time_scan_ms", "kiwi_hip_linear_fit_candidates_time_scan_shape"]


def _sums(K, offsets):
    """[1, nk, nrec, NN] sums with G = g x identity, b and R as given per (offset, receiver): val = R - 2 x.b + g x.x"""
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    nbr = np.zeros((1, len(offsets), len(offsets[0]), NN))
    for j, rows in enumerate(offsets):
        for r, (g, b, R) in enumerate(rows):
            for i in range(K):
                nbr[0, j, r, lr.tri(K, i, i)] = g
            nbr[0, j, r, NG:NG + K] = b
            nbr[0, j, r, NN - 1] = R
    return nbr


def _folded(nbr, K, weights=None):
    return np.stack([lr.solve(nbr[:, j], K, weights)["normal"] for j in range(nbr.shape[1])], 1)


def test_ties_across_offsets_and_across_a_tile_boundary():
    K = 2
    near, far = [(1.0, [1.0, 0.0], 4.0), (1.0, [0.0, 1.0], 4.0)], [(1.0, [0.25, 0.0], 4.0), (1.0, [0.0, 0.25], 4.0)]
    nbr = _sums(K, [far, near, far, near])                  # offsets 1 and 3 hold the same sums
    normal = _folded(nbr, K)
    cand = np.full((300, 2), 3.0)
    cand[255] = cand[256] = [1.0, 0.0]                      # equal candidates on either side of a tile of 256
    cand[299] = [0.0, 1.0]                                  # and their mirror image: the same misfit again
    for norm in ("l1norm", "l2norm"):
        out = ctr.evaluate(nbr, normal, None, False, cand, norm)
        assert np.all(out["best_index"][0] == 255) and out["best_offset"][0] == 1 and out["status"][0] == 0
        assert out["best_misfit"][0, 1] == out["best_misfit"][0, 3] < out["best_misfit"][0, 0] == out["best_misfit"][0, 2]
        assert np.array_equal(out["misfit"][0, :, 255], out["misfit"][0, :, 256]) and np.array_equal(out["misfit"][0, :, 255], out["misfit"][0, :, 299])
        assert np.all(out["cand_offset"][0, [255, 256, 299]] == 1)                 # the first of the two equal offsets
        assert np.array_equal(out["cand_misfit"][0], out["misfit"][0].min(0))
        assert np.all(np.isnan(out["best_scale"]) == False) and np.all(out["best_scale"] == 1.0)       # noqa: E712 (ones without free_scale)
    assert ctr.best_offset(np.array([-1, 4, 2, -1]), np.array([0.5, 2.0, 2.0, 0.1])) == 1
    assert ctr.best_offset(np.array([-1, -1]), np.array([np.nan, np.nan])) == -1
    cm, co, cs = ctr.marginal(np.array([[np.nan, 2.0, np.nan], [1.0, 2.0, np.nan], [1.0, 1.5, np.nan]]), np.arange(9.0).reshape(3, 3))
    assert list(co) == [1, 2, -1] and cm[0] == 1.0 and cm[1] == 1.5 and np.isnan(cm[2]) and cs[0] == 3.0 and cs[1] == 7.0 and np.isnan(cs[2])


def test_an_offset_whose_candidates_are_all_nan_and_a_group_without_data():
    K = 2
    good = [(1.0, [1.0, 0.5], 4.0), (1.0, [0.5, 1.0], 4.0)]
    flat = [(0.0, [1.0, 0.5], 4.0), (0.0, [0.5, 1.0], 4.0)]        # G = 0: no direction has a scale at this offset
    nbr = _sums(K, [flat, good, flat])
    normal = _folded(nbr, K)
    u = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 0.0], [-1.0, -1.0]])
    out = ctr.evaluate(nbr, normal, None, False, u, "l2norm", True)
    assert out["status"][0] == 0 and list(out["best_index"][0]) == [-1, 1, -1] and out["best_offset"][0] == 1
    assert np.all(np.isnan(out["misfit"][0, [0, 2]])) and np.all(np.isnan(out["best_misfit"][0, [0, 2]])) and np.all(np.isnan(out["best_scale"][0, [0, 2]]))
    assert list(out["cand_offset"][0]) == [1, 1, -1, 1] and np.isnan(out["cand_misfit"][0, 2]) and np.isnan(out["cand_scale"][0, 2])
    assert out["cand_scale"][0, 3] == -out["cand_scale"][0, 1] and out["cand_misfit"][0, 3] == out["cand_misfit"][0, 1]
    # best_scale is a = (u.b) / (u.G.u) of the winner on the folded row of its offset, formed anew
    xb, xgx = cr.quad(normal[0, 1], [np.array([u[1, i]]) for i in range(K)], K)
    assert out["best_scale"][0, 1] == (xb / xgx)[0] == out["scale"][0, 1, 1]
    # every offset NaN: no best offset
    out = ctr.evaluate(nbr[:, [0, 2]], normal[:, [0, 2]], None, False, u, "l2norm", True)
    assert out["best_offset"][0] == -1 and np.all(out["cand_offset"] == -1) and np.all(np.isnan(out["cand_misfit"])) and out["status"][0] == 0
    # a group without data (no reference energy, or every weight 0): status 1 whatever the offset
    empty = _sums(K, [[(1.0, [0.0, 0.0], 0.0)] * 2] * 3)
    for weights, sums in ((None, empty), (np.zeros(2), nbr)):
        for norm in ("l1norm", "l2norm"):
            out = ctr.evaluate(sums, _folded(sums, K, weights), weights, False, u, norm)
            assert out["status"][0] == 1 and out["best_offset"][0] == -1 and np.all(out["best_index"] == -1)
            assert np.all(np.isnan(out["misfit"])) and np.all(out["receiver_misfit"] == 0) and np.all(out["receiver_norm"] == 0)


def _dc_scenario(sdr, moment, shift):
    tensor, _ = mtfit.double_couple_candidates([sdr[0]], [sdr[1]], [sdr[2]], moment)
    sc = Scenario(comps_list=COMPS, true_type=6,
                  true_params=mt_row(tensor[0].astype(np.float32), location=[LOCATION[0] + shift * 0.5] + LOCATION[1:], risetime=0.5))
    e = sc.oracle()
    sc.make_references(e)
    e.close()
    for ir in range(1, sc.nrec + 1):
        sc.tapers[ir] = synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, WINDOW, sc.gf["dt"], 10.0)
    return sc, tensor[0]


def test_route_a_equals_route_b_on_the_oracle():
    sc = _scenario(LOCATION[0] + 2 * 0.5)
    dt = sc.gf["dt"]
    cand = np.random.default_rng(3).uniform(-8.0, 8.0, (12, 6))
    w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
    a_sums, b_evals = [], []
    for k in KS:
        e = _fresh(sc)
        syn_a, ref_a, receivers = oracle_traces(e, sc.comps, 6, _basis(k * dt), 6)                 # route A: the basis k dt later
        e.close()
        a_sums.append(lr.fit(syn_a, ref_a, receivers, dt, w, True))
        e = _fresh(sc, ref_shift=-k, taper_shift=-k * dt)
        syn_b, ref_b, _ = oracle_traces(e, sc.comps, 6, _basis(), 6)                               # route B: references and tapers k dt earlier
        e.close()
        b = lr.fit(syn_b, ref_b, receivers, dt, w, True)
        b_evals.append({norm: cr.evaluate(b["by_receiver"], b["normal"], w, True, cand, norm, free) for norm, free in (("l1norm", False), ("l2norm", True))})
    nbr, normal = np.stack([a["by_receiver"] for a in a_sums], 1), np.stack([a["normal"] for a in a_sums], 1)
    for norm, free in (("l1norm", False), ("l2norm", True)):
        scan = ctr.evaluate(nbr, normal, w, True, cand, norm, free)
        for j in range(len(KS)):
            want = b_evals[j][norm]
            for name in ("best_index", "best_misfit", "misfit", "scale", "receiver_misfit"):
                assert np.array_equal(scan[name][:, j], want[name], equal_nan=True), (norm, KS[j], name)
            assert np.array_equal(scan["status"], want["status"]) and np.array_equal(scan["receiver_norm"], want["receiver_norm"])
        assert np.any(scan["misfit"][:, 0] != scan["misfit"][:, -1]), "the offsets change the misfits"


def test_planted_double_couple_at_a_planted_offset_is_found():
    dt, S = 0.5, 4
    sdr, moment = (60.0, 60.0, -90.0), 3.0e18
    sc, tensor = _dc_scenario(sdr, moment, 2)               # the references: the planted mechanism two samples later than the basis
    raw, taper, ref, _ = _raw_rows(sc, _basis(), S)
    receivers = receivers_of(sc.comps)
    fits = [lr.fit(ltr.shifted_traces(raw, taper, S, k), ref, receivers, dt) for k in range(-3, 5)]
    nbr, normal = np.stack([f["by_receiver"] for f in fits], 1), np.stack([f["normal"] for f in fits], 1)
    grid = (range(0, 360, 30), range(0, 91, 30), range(-180, 180, 30))
    cand, _ = mtfit.double_couple_candidates(*grid, moment / UNIT)
    directions, _ = mtfit.double_couple_candidates(*grid)
    for norm, free, x in (("l1norm", False, cand), ("l2norm", False, cand), ("l2norm", True, directions)):
        out = ctr.evaluate(nbr, normal, None, False, x, norm, free)
        j, c = out["best_offset"][0], out["best_index"][0, 5]
        print("%s free=%s: best offset %d, misfits of the best mechanism per offset %s" % (norm, free, j, out["best_misfit"][0]))
        assert j == 5 and out["cand_offset"][0, c] == 5     # offsets -3 .. 4: +2 is index 5
        found = x[c] * (out["best_scale"][0, 5] if free else 1.0) * UNIT
        assert np.all(np.abs(found - tensor) <= 1e-4 * moment), (found, tensor)
        assert out["best_misfit"][0, 5] <= 1e-4 and np.all(np.delete(out["best_misfit"][0], 5) > 100 * out["best_misfit"][0, 5])
        assert out["cand_misfit"][0, c] == out["best_misfit"][0, 5] == np.nanmin(out["cand_misfit"][0])


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
    assert len(L.kiwi_hip_linear_fit_candidates_time_scan.argtypes) == 28
    assert len(L.kiwi_hip_linear_fit_candidates_time_scan_params.argtypes) == 30
    assert L.kiwi_hip_get_linear_fit_candidates_time_scan_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_linear_fit_candidates_time_scan_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    shapes = set()
    for K in range(1, kmax + 1):
        c, s = C.c_int(), C.c_int()
        assert L.kiwi_hip_linear_fit_candidates_time_scan_shape(K, C.byref(c), C.byref(s)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and s.value >= 1
        assert s.value * lr.nn_of(K) * 8 <= 160 * 1024                          # a stage of rows fits the LDS of a workgroup
        shapes.add((c.value, s.value))
    assert len(shapes) == 1
    c, s = C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_linear_fit_candidates_time_scan_shape(K, C.byref(c), C.byref(s)) != 0
    assert L.kiwi_hip_linear_fit_candidates_time_scan_shape(6, None, C.byref(s)) != 0
