"""kiwi_hip_linear_fit_candidates_floating without a device: the numpy restatement of the device arithmetic
(tests/linfit_candidates_floating_restatement.py) on hand-made sums -- the first minimum among equal shifts, the clamp, a skipped
receiver, both outer norms, anarchy --, the maths against the CPU oracle's own floating_l2norm evaluation of about 50 double
couples, and the plumbing of the new entry points.  The device is pinned to the restatement bit for bit in
tests/test_linfit_candidates_floating_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib, synthetic
from tests import linfit_candidates_floating_restatement as fr
from tests import linfit_candidates_restatement as cr
from tests import linfit_restatement as lr
from tests.common import MISFIT_RTOL, Scenario
from tests.linfit_cases import UNIT, basis_rows, mt_row, oracle_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_linear_fit_candidates_floating", "kiwi_hip_linear_fit_candidates_floating_params",
           "kiwi_hip_get_linear_fit_candidates_floating_ms", "kiwi_hip_linear_fit_candidates_floating_shape"]
COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # tests/test_linfit_gpu.py's receivers of 1 to 5 components


def _identity_sums(K, nrec):
    """[1, nrec, NN] with G_r = identity (b, R of the unshifted row are not read): val_q = R[q] - 2 x.b[q] + x.x"""
    nbr = np.zeros((1, nrec, lr.nn_of(K)))
    for r in range(nrec):
        for i in range(K):
            nbr[0, r, lr.tri(K, i, i)] = 1.0
    return nbr


def _shifts(rows):
    """(shift_b, shift_R) of one group from per-receiver lists of (b [K], R) per shift"""
    return ([np.array([[b for b, _ in rec]], np.float64) for rec in rows], [np.array([[R for _, R in rec]], np.float64) for rec in rows])


def test_first_minimum_clamp_and_skipped_receivers():
    K = 2
    nbr = _identity_sums(K, 3)
    # receiver 0: shifts 1 and 2 give the same val for x = (1, 0): the FIRST one wins; receiver 1: val < 0 at its second shift is
    # clamped to 0 and wins; receiver 2: no reference energy at any shift: skipped
    rows = [[([0.0, 0.0], 4.0), ([1.0, 0.0], 4.0), ([1.0, 0.0], 4.0), ([0.5, 0.0], 4.0)],
            [([0.0, 1.0], 9.0), ([2.0, 0.0], 1.0)],
            [([0.0, 0.0], 0.0), ([0.0, 0.0], 0.0)]]
    b, R = _shifts(rows)
    lo = [-1, 5, 0]
    x = np.array([[1.0, 0.0]])
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            out = fr.evaluate(nbr, b, R, lo, None, anarchy, x, norm)
            assert list(out["cand_shift"][0, 0]) == [0, 6, 0] and list(out["best_shift"][0]) == [0, 6, 0]
            assert list(out["receiver_val"][0, 0]) == [3.0, 0.0, 0.0]          # 4 - 2 + 1; 1 - 4 + 1 clamped; skipped
            n0, n1 = (2.0 + 2.0 + 2.0 + 2.0) / 4.0, (3.0 + 1.0) / 2.0
            assert list(out["receiver_norm"][0]) == [np.float32(n0), np.float32(n1), 0.0]
            assert out["status"][0] == 0 and out["best_index"][0] == 0
            v0, v1 = (1.0 / n0, 1.0 / n1) if anarchy else (1.0, 1.0)
            if norm == "l1norm":
                want = (v0 * np.sqrt(3.0) + v1 * 0.0) / (v0 * n0 + v1 * n1)
            else:
                want = np.sqrt(((v0 * v0) * 3.0 + (v1 * v1) * 0.0) / ((v0 * v0) * (n0 * n0) + (v1 * v1) * (n1 * n1)))
            assert out["misfit"][0, 0] == want
    # a receiver of weight 0 is skipped as well; with every receiver skipped: status 1, NaN, no winner, zeros
    out = fr.evaluate(nbr, b, R, lo, np.array([0.0, 1.0, 1.0]), False, x, "l1norm")
    assert list(out["cand_shift"][0, 0]) == [0, 6, 0] and out["receiver_norm"][0, 0] == 0 and out["misfit"][0, 0] == 0.0
    out = fr.evaluate(nbr, b, R, lo, np.array([0.0, 0.0, 1.0]), False, x, "l2norm")
    assert out["status"][0] == 1 and out["best_index"][0] == -1 and np.isnan(out["best_misfit"][0]) and np.all(np.isnan(out["misfit"]))
    assert np.all(out["best_shift"] == 0) and np.all(out["cand_shift"] == 0) and np.all(out["receiver_norm"] == 0)


def test_one_shift_per_receiver_is_the_candidate_restatement_under_l1norm():
    """ranges of one shift: the l1norm outputs are tests/linfit_candidates_restatement.py's, bit for bit"""
    rng = np.random.default_rng(3)
    K, nrec, ng = 5, 4, 2
    nbr = np.zeros((ng, nrec, lr.nn_of(K)))
    NG = K * (K + 1) // 2
    for g in range(ng):
        for r in range(nrec):
            A = rng.standard_normal((K + 1, 40))
            M = A @ A.T
            for i in range(K):
                for j in range(i, K):
                    nbr[g, r, lr.tri(K, i, j)] = M[i, j]
            nbr[g, r, NG:NG + K] = M[:K, K]
            nbr[g, r, -1] = M[K, K]
    nbr[:, 2, -1] = 0.0                                               # no reference energy: skipped by both
    w = np.array([1.0, 0.0, 2.0, 0.5])
    cand = rng.uniform(-1.0, 1.0, (7, K))
    b = [nbr[:, r, None, NG:NG + K] for r in range(nrec)]
    R = [nbr[:, r, None, -1] for r in range(nrec)]
    for anarchy in (False, True):
        want = cr.evaluate(nbr, lr.solve(nbr, K, w, anarchy)["normal"], w, anarchy, cand, "l1norm")
        got = fr.evaluate(nbr, b, R, [0] * nrec, w, anarchy, cand, "l1norm")
        for name in ("misfit", "receiver_misfit", "receiver_norm", "best_index", "best_misfit", "status", "receiver_val"):
            assert np.array_equal(want[name], got[name], equal_nan=True), name
        assert np.all(got["cand_shift"] == 0)


# ------------------------------------------------------------------------------------------------ the maths on the CPU oracle
PLANTED_SDR = (40.0, 60.0, 100.0, 5e18)
DELAYS = [2, -1, 0, 3, -2, 1]                                # whole samples by which each station's data are late
RANGES = [(-4, 2), (-1, 3), (-2, 2), (-6, 2), (-1, 4), (-3, 3)]      # 7, 5, 5, 9, 6, 7 shifts; each holds the shift -delay
NCAND = 50
PAD = 8


def test_predicted_receiver_misfits_shifts_and_global_misfit_against_the_oracle():
    """Basis synthetics of the six elementary tensors and the shifted tapered references from oracle/libko.so, the sums formed in
    numpy (tests/linfit_restatement.py's Gram order), and for 50 random double couples the restatement's m_r, shift_r and the
    global misfit against the oracle's own floating_l2norm evaluation of the combined `moment_tensor` source.

    m_r against sqrt(sum_k m_k^2) of the oracle's slot misfits, and the global misfits, under misfit_close's rule for two
    comparators (tests/common.py): |a - b| <= MISFIT_RTOL max(b, norm factor), for the global misfit with norm factor 1 on
    sqrt(g^2 + 1).  The global misfit is formed as the oracle forms it -- sqrt(sum_r min val_r) over sqrt(sum_k n_k^2) with the
    per-SLOT norm factors n_k (the oracle's) --: the call's own n_r is receiver-level (include/kiwi_hip.h).  Shifts must be
    equal except where the oracle's own two smallest sums over the shifts (roots of sum_k m_k^2) differ by less than that
    bound; such pairs may be at most 5 % of all (candidate, receiver) pairs."""
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    rng = np.random.default_rng(77)
    for (ir, k), (lo, d) in list(sc.refs.items()):         # (padded: the data cover the taper at every shift of the ranges)
        padded = np.zeros(len(d) + 2 * PAD)
        padded[PAD + DELAYS[ir - 1]:PAD + DELAYS[ir - 1] + len(d)] = d
        sc.refs[(ir, k)] = (lo - PAD, (padded + 0.02 * np.std(d) * rng.standard_normal(len(padded))).astype(np.float32))
    sc.apply_setup(e, True)
    e.set_misfit_method(1)
    K, dt, nrec = 6, sc.gf["dt"], sc.nrec
    syn, ref0, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(np.zeros(6))), K)
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    nbr = lr.gram_by_receiver(syn, ref0, receivers, dt)
    ns = [hi - lo + 1 for lo, hi in RANGES]
    shift_b = [np.zeros((1, n, K)) for n in ns]
    shift_R = [np.zeros((1, n)) for n in ns]
    for j in range(max(ns)):
        sh = [RANGES[r][0] + min(j, ns[r] - 1) for r in range(nrec)]
        refq = []
        for r in range(nrec):
            e.shift_ref_seismogram(r + 1, sh[r])
            for k in range(len(sc.comps[r])):
                refq.append(e.reference(r + 1, k + 1, 2)[1])
                assert len(refq[-1]) == len(ref0[len(refq) - 1])
            e.shift_ref_seismogram(r + 1, -sh[r])
        if all(s == 0 for s in sh):
            assert all(np.array_equal(a, b) for a, b in zip(refq, ref0))
        q = lr.gram_by_receiver(syn, refq, receivers, dt)
        for r in range(nrec):
            if j < ns[r]:
                shift_b[r][0, j], shift_R[r][0, j] = q[0, r, NG:NG + K], q[0, r, NN - 1]
                if sh[r] == 0:
                    assert np.array_equal(q[0, r], nbr[0, r])            # shift 0: the unshifted sums, bit for bit
    sdr = np.stack([rng.uniform(0., 360., NCAND), rng.uniform(0., 90., NCAND), rng.uniform(-180., 180., NCAND)], 1)
    sdr[0] = PLANTED_SDR[:3]
    tensors = np.array([synthetic.mt_from_sdr(s, d, r, PLANTED_SDR[3]) for s, d, r in sdr]).astype(np.float32)
    cand = tensors.astype(np.float64) / UNIT
    out = fr.evaluate(nbr, shift_b, shift_R, [lo for lo, _ in RANGES], None, False, cand, "l2norm")
    assert np.all(out["status"] == 0)
    assert list(out["cand_shift"][0, 0]) == [-d for d in DELAYS]       # the planted mechanism finds the planted delays

    e.set_misfit_method(7)
    slot_r = [r for r in range(nrec) for _ in sc.comps[r]]
    nties, worst_m, worst_g = 0, 0.0, 0.0
    for c in range(NCAND):
        e.set_source_params(6, mt_row(tensors[c]))
        per_shift = np.full((nrec, max(ns)), np.inf)
        for j in range(max(ns)):
            for r in range(nrec):
                s = RANGES[r][0] + min(j, ns[r] - 1)
                e.set_floating_shiftrange(r + 1, s, s)
            m = e.get_misfits()[0].astype(np.float64)
            for r in range(nrec):
                if j < ns[r]:
                    per_shift[r, j] = np.sqrt(sum(m[k] ** 2 for k in range(len(m)) if slot_r[k] == r))
        for r in range(nrec):
            e.set_floating_shiftrange(r + 1, *RANGES[r])
        m, n, g = e.get_misfits()
        m, n = m.astype(np.float64), n.astype(np.float64)
        for r in range(nrec):
            mr = np.sqrt(sum(m[k] ** 2 for k in range(len(m)) if slot_r[k] == r))
            nr = np.sqrt(sum(n[k] ** 2 for k in range(len(n)) if slot_r[k] == r))
            bound = MISFIT_RTOL * max(mr, nr)
            err = abs(np.sqrt(out["receiver_val"][0, c, r]) - mr)
            worst_m = max(worst_m, err / bound)
            assert err <= bound, (c, r, np.sqrt(out["receiver_val"][0, c, r]), mr, bound)
            osh = e.floating_shift(r + 1)
            assert mr == per_shift[r, osh - RANGES[r][0]]                  # the oracle's winner is among its own sums
            if out["cand_shift"][0, c, r] != osh:
                two = np.sort(per_shift[r, :ns[r]])[:2]
                assert two[1] - two[0] < bound, (c, r, out["cand_shift"][0, c, r], osh, two, bound)
                nties += 1
        gp = np.sqrt(np.sum(out["receiver_val"][0, c])) / np.sqrt(np.sum(n * n))
        worst_g = max(worst_g, abs(gp - g) / (MISFIT_RTOL * np.sqrt(g * g + 1.0)))
        assert abs(gp - g) <= MISFIT_RTOL * np.sqrt(g * g + 1.0), (c, gp, g)
    e.close()
    print("50 double couples against the oracle's floating_l2norm: largest |m_r error| / bound %.3g, global %.3g, %d of %d shifts "
          "differ at a tie" % (worst_m, worst_g, nties, NCAND * nrec))
    assert nties <= 0.05 * NCAND * nrec


# ------------------------------------------------------------------------------------------------ plumbing
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
    assert len(L.kiwi_hip_linear_fit_candidates_floating.argtypes) == 18
    assert len(L.kiwi_hip_linear_fit_candidates_floating_params.argtypes) == 20
    assert L.kiwi_hip_get_linear_fit_candidates_floating_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_linear_fit_candidates_floating_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    shapes = set()
    for K in range(1, kmax + 1):
        c, j, s = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_linear_fit_candidates_floating_shape(K, C.byref(c), C.byref(j), C.byref(s)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and j.value >= 1 and s.value >= 1
        assert j.value * (K + 1) * 2 <= 128                                     # a pass's fp64 accumulators stay in registers
        assert (s.value * (K + 1) + lr.nn_of(K)) * 8 <= 160 * 1024              # a stage of rows fits the LDS of a workgroup
        shapes.add((c.value, j.value, s.value))
    assert len(shapes) == 1
    c, j, s = C.c_int(), C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_linear_fit_candidates_floating_shape(K, C.byref(c), C.byref(j), C.byref(s)) != 0
    assert L.kiwi_hip_linear_fit_candidates_floating_shape(6, None, C.byref(j), C.byref(s)) != 0
    assert L.kiwi_hip_linear_fit_candidates_floating_shape(6, C.byref(c), C.byref(j), None) != 0
