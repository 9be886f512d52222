"""kiwi_hip_linear_fit_candidates_bootstrap without a device: the plumbing of the four entry points, the shape call, and the numpy
restatement (tests/linfit_candidates_bootstrap_restatement.py) on hand-made sums -- that it IS the composition of the two parents'
restatements, the ties, the excluded draws, and the float identity the l2 route relies on.  The device is pinned to the host
route and to the restatement bit for bit in tests/test_linfit_candidates_bootstrap_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib
from tests import linfit_candidates_bootstrap_restatement as br
from tests import linfit_candidates_timescan_restatement as ctr
from tests import linfit_restatement as lr
from tests import outer_restatement as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_linear_fit_candidates_bootstrap", "kiwi_hip_linear_fit_candidates_bootstrap_params",
           "kiwi_hip_get_linear_fit_candidates_bootstrap_ms", "kiwi_hip_linear_fit_candidates_bootstrap_shape"]


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
    assert len(L.kiwi_hip_linear_fit_candidates_bootstrap.argtypes) == 22
    assert len(L.kiwi_hip_linear_fit_candidates_bootstrap_params.argtypes) == 24
    assert L.kiwi_hip_get_linear_fit_candidates_bootstrap_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape.argtypes == [C.c_int, klib.c_int_p, klib.c_int_p, klib.c_int_p]
    assert "kiwi_hip_linear_fit_candidates_bootstrap_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    assert kmax == 8
    for K in range(1, kmax + 1):
        c, t, r = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(K, C.byref(c), C.byref(t), C.byref(r)) == 0
        assert c.value == 256 and t.value >= 1 and r.value >= 64
        # a candidate's column of float misfits, the weight rows of a draw tile and the receiver weights fit a workgroup's LDS
        assert r.value * (c.value * 4 + t.value * 8 + 8) <= 160 * 1024
        assert t.value * 2 <= 128                                               # a tile's fp64 accumulators stay in registers
    c, t, r = C.c_int(), C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(K, C.byref(c), C.byref(t), C.byref(r)) != 0
    assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(6, None, C.byref(t), C.byref(r)) != 0
    assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(6, C.byref(c), None, C.byref(r)) != 0
    assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(6, C.byref(c), C.byref(t), None) != 0


# ------------------------------------------------------------------------------------------------ the restatement
def _sums(rng, ng, nk, nrec, K):
    """(by_receiver [ng, nk, nrec, NN]) of random traces: the data of a receiver are the same at every offset (R_r does not depend
    on the offset), the basis traces differ"""
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    nbr = np.zeros((ng, nk, nrec, NN))
    for g in range(ng):
        for r in range(nrec):
            d = rng.standard_normal((1, 40))
            for j in range(nk):
                A = np.concatenate([rng.standard_normal((K, 40)), d])
                M = A @ A.T
                for i in range(K):
                    for k in range(i, K):
                        nbr[g, j, r, lr.tri(K, i, k)] = M[i, k]
                nbr[g, j, r, NG:NG + K] = M[:K, K]
                nbr[g, j, r, -1] = M[K, K]
    return nbr


def _normal(nbr, K, w, anarchy):
    return np.stack([lr.solve(nbr[:, j], K, w, anarchy)["normal"] for j in range(nbr.shape[1])], 1)


def _draws(rng, nrec, skipped):
    """ones, two resampled rows, all zeros, a row that is non-zero only on the skipped receivers"""
    dw = np.ones((5, nrec))
    dw[1:3] = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=2)
    dw[3] = 0.0
    dw[4] = 0.0
    dw[4, skipped] = 2.0
    return dw


def test_restatement_is_the_composition_of_the_parents_restatements():
    rng = np.random.default_rng(11)
    K, ng, nk, nrec, ncand = 3, 2, 3, 5, 7
    nbr = _sums(rng, ng, nk, nrec, K)
    nbr[:, :, 3, -1] = 0.0                                    # no reference energy: skipped
    w = np.array([1.0, 0.0, 2.0, 0.5, 1.5])                   # weight 0: skipped
    cand = rng.uniform(-1.0, 1.0, (ncand, K))
    dw = _draws(rng, nrec, [1, 3])
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            normal = _normal(nbr, K, w, anarchy)
            got = br.evaluate(nbr, normal, w, anarchy, cand, norm, dw)
            scan = ctr.evaluate(nbr, normal, w, anarchy, cand, norm, False)
            m = scan["receiver_misfit"].reshape(ng * nk * ncand, nrec)
            n = np.repeat(scan["receiver_norm"], nk * ncand, axis=0)
            bv, bi, _ = orr.outer_misfits(m, n, np.arange(nrec), nrec, norm, w, anarchy, dw)
            assert np.array_equal(got["best_value"], bv, equal_nan=True)
            has = ~np.isnan(bv)
            assert np.array_equal(has, [True, True, True, False, False])        # zeros; only skipped receivers: excluded
            flat = (got["best_group"] * nk + got["best_offset"]) * ncand + got["best_cand"]
            assert np.array_equal(flat[has], bi[has])
            for name in ("best_group", "best_offset", "best_cand"):
                assert np.all(got[name][~has] == -1) and got[name].dtype == np.int32
            assert np.all(np.isnan(got["group_value"][:, 3:])) and np.all(got["group_cand"][:, 3:] == -1)
            assert np.all(got["group_offset"][:, 3:] == -1)
            for g in range(ng):
                lo = g * nk * ncand
                gv, gi, _ = orr.outer_misfits(m[lo:lo + nk * ncand], n[lo:lo + nk * ncand], np.arange(nrec), nrec, norm, w, anarchy, dw)
                assert np.array_equal(got["group_value"][g], gv, equal_nan=True)
                assert np.array_equal((got["group_offset"][g] * ncand + got["group_cand"][g])[has], gi[has])
            # the call's best is the best of the groups' bests, the lower group among equals
            for d in np.nonzero(has)[0]:
                g = got["best_group"][d]
                assert got["group_value"][g, d] == got["best_value"][d] == np.nanmin(got["group_value"][:, d])
                assert got["group_offset"][g, d] == got["best_offset"][d] and got["group_cand"][g, d] == got["best_cand"][d]
            assert np.array_equal(got["status"], scan["status"]) and np.all(got["status"] == 0)
            # a draw of ones on the receiver-level l1 fold: the candidate call's own misfit where the norms are floats already
            if norm == "l1norm" and not anarchy:
                assert np.allclose(got["best_value"][0], np.nanmin(scan["misfit"]), rtol=1e-6)


def test_ties_go_to_the_lowest_group_offset_and_candidate():
    rng = np.random.default_rng(12)
    K, nk, nrec = 2, 2, 4
    one = _sums(rng, 1, nk, nrec, K)
    nbr = np.concatenate([one, one])                          # two groups with identical rows
    nbr[:, 1] = nbr[:, 0]                                     # two offsets with identical rows
    cand = rng.uniform(-1.0, 1.0, (5, K))
    cand[3] = cand[1]                                         # two identical candidates
    dw = np.concatenate([np.ones((1, nrec)), rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=6)])
    for norm in ("l1norm", "l2norm"):
        got = br.evaluate(nbr, _normal(nbr, K, None, True), None, True, cand, norm, dw)
        assert np.all(got["best_group"] == 0) and np.all(got["best_offset"] == 0) and np.all(got["best_cand"] != 3)
        assert np.array_equal(got["group_value"][0], got["group_value"][1])
        assert np.all(got["group_offset"] == 0) and np.array_equal(got["group_cand"][0], got["group_cand"][1])
        # the same candidates in the opposite order: the tie still goes to the lower index, now the other copy
        back = br.evaluate(nbr, _normal(nbr, K, None, True), None, True, cand[::-1], norm, dw)
        assert np.array_equal(back["best_value"], got["best_value"]) and np.all(back["best_cand"] != 3)
        assert np.array_equal(back["best_cand"], np.where(got["best_cand"] == 1, 1, 4 - got["best_cand"]))


def test_a_group_without_data_is_excluded_from_every_draw():
    rng = np.random.default_rng(13)
    K, nk, nrec = 2, 1, 3
    nbr = _sums(rng, 2, nk, nrec, K)
    nbr[0, :, :, -1] = 0.0                                    # group 0: no reference energy at all: status 1
    cand = rng.uniform(-1.0, 1.0, (4, K))
    dw = _draws(rng, nrec, [])
    for norm in ("l1norm", "l2norm"):
        got = br.evaluate(nbr, _normal(nbr, K, None, False), None, False, cand, norm, dw)
        assert list(got["status"]) == [1, 0]
        assert np.all(np.isnan(got["group_value"][0])) and np.all(got["group_cand"][0] == -1) and np.all(got["group_offset"][0] == -1)
        assert np.all(got["best_group"][:3] == 1) and np.all(got["best_group"][3:] == -1) and np.all(np.isnan(got["best_value"][3:]))


def test_root_of_the_square_of_a_float_is_the_float():
    """under l2norm the host route forms sqrt(mv * mv) of the float misfit widened to fp64; the device uses mv.  The product of two
    24-bit significands is exact in fp64, far from its overflow and underflow, so the root is exact"""
    rng = np.random.default_rng(14)
    f = np.concatenate([rng.uniform(0.0, 1.0, 200000).astype(np.float32),
                        np.exp(rng.uniform(np.log(1e-45), np.log(3e38), 200000)).astype(np.float32),
                        np.array([0.0, np.finfo(np.float32).tiny, np.finfo(np.float32).max, 1e-45, 1.0, 3.0], np.float32)])
    mv = f.astype(np.float64)
    assert np.array_equal(np.sqrt(mv * mv), mv)
