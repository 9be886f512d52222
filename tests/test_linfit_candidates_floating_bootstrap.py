"""kiwi_hip_linear_fit_candidates_floating_bootstrap without a device: the plumbing of the four entry points, the shape call, the
refusals the header and INTEGRATION.md list, and the numpy restatement
(tests/linfit_candidates_floating_bootstrap_restatement.py) on hand-made sums -- that it IS the composition of the two parents'
restatements, the ties, the excluded draws, a receiver without norm.  The device is pinned to the host route and to the
restatement bit for bit in tests/test_linfit_candidates_floating_bootstrap_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib
from tests import linfit_candidates_floating_bootstrap_restatement as fbr
from tests import linfit_candidates_floating_restatement as fr
from tests import linfit_restatement as lr
from tests import outer_restatement as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kiwi_hip_linear_fit_candidates_floating_bootstrap"
SYMBOLS = [NAME, NAME + "_params", "kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms", NAME + "_shape"]


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
    assert len(getattr(L, NAME).argtypes) == 19
    assert len(getattr(L, NAME + "_params").argtypes) == 21
    assert L.kiwi_hip_get_linear_fit_candidates_floating_bootstrap_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert getattr(L, NAME + "_shape").argtypes == [C.c_int, klib.c_int_p, klib.c_int_p, klib.c_int_p]
    assert NAME + "_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()
    # the number of arguments of the two calls in the header is the ctypes table's
    for s in SYMBOLS[:2]:
        args = re.search(r"\bint %s\((.*?)\);" % s, header, re.S).group(1)
        assert len(args.split(",")) == len(getattr(L, s).argtypes), s


def test_engine_and_helper_are_there():
    from kiwi_amd import mtfit
    from kiwi_amd.engine import CandidateFloatingBootstrap, Engine
    for name in ("", "_params", "_ms", "_shape"):
        assert callable(getattr(Engine, "linear_fit_candidates_floating_bootstrap" + name))
    assert CandidateFloatingBootstrap._fields == ("best_value", "best_group", "best_cand", "best_shift", "status", "group_value",
                                                  "group_cand", "group_shift")
    assert callable(mtfit.bootstrap_double_couples_floating)
    assert os.path.exists(os.path.join(ROOT, "examples", "invert_double_couple_station_shifts_bootstrap.py"))


def test_shape_answers_without_a_device_within_the_lds_limit():
    L = klib.load()
    shape = getattr(L, NAME + "_shape")
    kmax = L.kiwi_hip_linear_fit_max_basis()
    assert kmax == 8
    stage = C.c_int()
    for K in range(1, kmax + 1):
        c, t, r, j = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert shape(K, C.byref(c), C.byref(t), C.byref(r)) == 0
        assert L.kiwi_hip_linear_fit_candidates_floating_shape(K, C.byref(j), C.byref(j), C.byref(stage)) == 0
        assert c.value == 256 and t.value >= 1 and r.value >= 64
        # G_r and a stage of shift rows, the wavefronts' bests of a draw tile, and per receiver a candidate column of float misfits,
        # the weight row of a draw tile and the receiver weight: inside the 160 KiB a workgroup may hold
        fixed = (lr.nn_of(K) + stage.value * (K + 1)) * 8 + (c.value // 64) * t.value * 12
        assert fixed + r.value * (c.value * 4 + t.value * 8 + 8) <= 160 * 1024
        assert t.value * 2 <= 128                                               # a tile's fp64 accumulators stay in registers
    c, t, r = C.c_int(), C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert shape(K, C.byref(c), C.byref(t), C.byref(r)) != 0
    assert shape(6, None, C.byref(t), C.byref(r)) != 0
    assert shape(6, C.byref(c), None, C.byref(r)) != 0
    assert shape(6, C.byref(c), C.byref(t), None) != 0


def test_the_headers_refusals_are_listed_in_integration_md():
    header = open(os.path.join(ROOT, "include", "kiwi_hip.h")).read()
    block = header[header.index("JOINT BOOTSTRAP of a candidate search WITH PER-RECEIVER TIME SHIFTS"):header.index("int %s(" % NAME)]
    doc = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    at = doc.index("kiwi_hip_linear_fit_candidates_floating_bootstrap")
    assert '"linear_fit_candidates_floating_bootstrap:"' in re.sub(r"\s+", " ", block)
    for phrase in ("ndraw < 1", "null draw_weights", "not finite", "max_receivers", "only some of the three group_", "floating_l2norm",
                   "16 bits"):
        assert phrase in re.sub(r"[\s*]+", " ", block), phrase
        assert phrase in doc[at:], phrase


# ------------------------------------------------------------------------------------------------ the restatement
def _sums(rng, ng, nrec, K, ns):
    """(by_receiver [ng, nrec, NN], shift_b[r] [ng, ns_r, K], shift_R[r] [ng, ns_r]) of random traces: the basis traces of a
    receiver are the same at every shift, the data are another window of one long trace"""
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    nbr = np.zeros((ng, nrec, NN))
    sb = [np.zeros((ng, n, K)) for n in ns]
    sR = [np.zeros((ng, n)) for n in ns]
    for g in range(ng):
        for r in range(nrec):
            A = rng.standard_normal((K, 40))
            long = rng.standard_normal(40 + ns[r])
            M = A @ A.T
            for i in range(K):
                for k in range(i, K):
                    nbr[g, r, lr.tri(K, i, k)] = M[i, k]
            for q in range(ns[r]):
                d = long[q:q + 40]
                sb[r][g, q], sR[r][g, q] = A @ d, d @ d
            nbr[g, r, NG:NG + K], nbr[g, r, -1] = sb[r][g, 0], sR[r][g, 0]
    return nbr, sb, sR


def _draws(rng, nrec, skipped):
    """ones, all zeros, a row that is non-zero only on the skipped receivers, three resampled rows"""
    dw = np.ones((6, nrec))
    dw[1] = 0.0
    dw[2] = 0.0
    dw[2, skipped] = 2.0
    dw[3:] = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=3)
    return dw


def test_restatement_is_the_composition_of_the_parents_restatements():
    rng = np.random.default_rng(21)
    K, ng, nrec, ncand = 3, 2, 5, 7
    ns, lo = [1, 3, 4, 2, 5], [0, -1, 2, -3, -2]
    nbr, sb, sR = _sums(rng, ng, nrec, K, ns)
    sR[3][:] = 0.0                                            # no reference energy at any shift: n_r = 0, never counts
    w = np.array([1.0, 0.0, 2.0, 0.5, 1.5])                   # weight 0: skipped
    cand = rng.uniform(-1.0, 1.0, (ncand, K))
    dw = _draws(rng, nrec, [1, 3])
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            got = fbr.evaluate(nbr, sb, sR, lo, w, anarchy, cand, norm, dw)
            scan = fr.evaluate(nbr, sb, sR, lo, w, anarchy, cand, norm)
            m = scan["receiver_misfit"].reshape(ng * ncand, nrec)
            n = np.repeat(scan["receiver_norm"], ncand, axis=0)
            assert np.all(scan["receiver_norm"][:, [1, 3]] == 0) and np.all(scan["receiver_norm"][:, [0, 2, 4]] > 0)
            bv, bi, _ = orr.outer_misfits(m, n, np.arange(nrec), nrec, norm, w, anarchy, dw)
            assert np.array_equal(got["best_value"], bv, equal_nan=True)
            has = ~np.isnan(bv)
            assert np.array_equal(has, [True, False, False, True, True, True])      # zeros; only skipped receivers: excluded
            assert np.array_equal((got["best_group"] * ncand + got["best_cand"])[has], bi[has])
            for name in ("best_group", "best_cand"):
                assert np.all(got[name][~has] == -1) and got[name].dtype == np.int32
            assert got["best_shift"].shape == (6, nrec) and got["best_shift"].dtype == np.int32 and not np.any(got["best_shift"][~has])
            assert got["group_shift"].shape == (ng, 6, nrec) and got["group_shift"].dtype == np.int32 and not np.any(got["group_shift"][:, ~has])
            assert np.all(np.isnan(got["group_value"][:, 1:3])) and np.all(got["group_cand"][:, 1:3] == -1)
            cs = scan["cand_shift"].reshape(ng * ncand, nrec)
            assert np.array_equal(got["best_shift"][has], cs[bi[has]])              # the winner's row of cand_shift
            assert not np.any(got["best_shift"][:, [1, 3]]) and np.any(got["best_shift"][:, [2, 4]])
            for r in (0, 2, 4):
                assert np.all((got["best_shift"][has, r] >= lo[r]) & (got["best_shift"][has, r] < lo[r] + ns[r]))
            for g in range(ng):
                gv, gi, _ = orr.outer_misfits(m[g * ncand:(g + 1) * ncand], n[g * ncand:(g + 1) * ncand], np.arange(nrec), nrec, norm, w, anarchy, dw)
                assert np.array_equal(got["group_value"][g], gv, equal_nan=True)
                assert np.array_equal(got["group_cand"][g][has], gi[has])
                assert np.array_equal(got["group_shift"][g][has], scan["cand_shift"][g, gi[has]])
            # the call's best is the best of the groups' bests, the lower group among equals, its shifts with it
            for d in np.nonzero(has)[0]:
                g = got["best_group"][d]
                assert got["group_value"][g, d] == got["best_value"][d] == np.nanmin(got["group_value"][:, d])
                assert got["group_cand"][g, d] == got["best_cand"][d] and np.array_equal(got["group_shift"][g, d], got["best_shift"][d])
            assert np.array_equal(got["status"], scan["status"]) and np.all(got["status"] == 0)


def test_ties_go_to_the_lowest_group_and_candidate():
    rng = np.random.default_rng(22)
    K, nrec = 2, 4
    ns, lo = [3, 1, 4, 2], [-1, 0, 0, -2]
    one = _sums(rng, 1, nrec, K, ns)
    nbr = np.concatenate([one[0], one[0]])                    # two groups with identical rows
    sb = [np.concatenate([b, b]) for b in one[1]]
    sR = [np.concatenate([R, R]) for R in one[2]]
    cand = rng.uniform(-1.0, 1.0, (5, K))
    cand[3] = cand[1]                                         # two identical candidates
    dw = np.concatenate([np.ones((1, nrec)), rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=6)])
    for norm in ("l1norm", "l2norm"):
        got = fbr.evaluate(nbr, sb, sR, lo, None, True, cand, norm, dw)
        assert np.all(got["best_group"] == 0) and np.all(got["best_cand"] != 3)
        assert np.array_equal(got["group_value"][0], got["group_value"][1]) and np.array_equal(got["group_cand"][0], got["group_cand"][1])
        assert np.array_equal(got["group_shift"][0], got["group_shift"][1]) and np.array_equal(got["best_shift"], got["group_shift"][0])
        # the same candidates in the opposite order: the tie still goes to the lower index, now the other copy
        back = fbr.evaluate(nbr, sb, sR, lo, None, True, cand[::-1], norm, dw)
        assert np.array_equal(back["best_value"], got["best_value"]) and np.all(back["best_cand"] != 3)
        assert np.array_equal(back["best_cand"], np.where(got["best_cand"] == 1, 1, 4 - got["best_cand"]))
        assert np.array_equal(back["best_shift"], got["best_shift"])


def test_an_all_zero_draw_and_a_group_without_data():
    rng = np.random.default_rng(23)
    K, nrec = 2, 3
    ns, lo = [2, 3, 1], [0, -1, 0]
    nbr, sb, sR = _sums(rng, 2, nrec, K, ns)
    for R in sR:
        R[0] = 0.0                                            # group 0: no reference energy at all: status 1
    cand = rng.uniform(-1.0, 1.0, (4, K))
    dw = _draws(rng, nrec, [])
    for norm in ("l1norm", "l2norm"):
        got = fbr.evaluate(nbr, sb, sR, lo, None, False, cand, norm, dw)
        assert list(got["status"]) == [1, 0]
        assert np.all(np.isnan(got["group_value"][0])) and np.all(got["group_cand"][0] == -1) and not np.any(got["group_shift"][0])
        has = np.array([True, False, False, True, True, True])
        assert np.all(got["best_group"][has] == 1) and np.all(got["best_group"][~has] == -1) and np.all(got["best_cand"][~has] == -1)
        assert np.all(np.isnan(got["best_value"][~has])) and not np.any(got["best_shift"][~has])


def test_a_receiver_whose_norm_is_zero_never_counts():
    """n_r = 0 (no reference energy at any shift): its draw weight changes nothing, and a draw that weights it alone is excluded"""
    rng = np.random.default_rng(24)
    K, nrec = 2, 4
    ns, lo = [2, 3, 2, 3], [0, -1, -1, 0]
    nbr, sb, sR = _sums(rng, 2, nrec, K, ns)
    sR[2][:] = 0.0
    cand = rng.uniform(-1.0, 1.0, (6, K))
    dw = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=8).astype(np.float64)
    dw[:, 0] += 1.0                                           # (no draw rests on receiver 3 alone)
    other = dw.copy()
    other[:, 2] = rng.uniform(0.0, 5.0, 8)
    alone = np.zeros((1, nrec))
    alone[0, 2] = 3.0
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            a = fbr.evaluate(nbr, sb, sR, lo, None, anarchy, cand, norm, dw)
            b = fbr.evaluate(nbr, sb, sR, lo, None, anarchy, cand, norm, other)
            for name in a:
                assert np.array_equal(a[name], b[name], equal_nan=True), name
            assert not np.any(a["best_shift"][:, 2]) and not np.any(a["group_shift"][:, :, 2]) and not np.any(np.isnan(a["best_value"]))
            c = fbr.evaluate(nbr, sb, sR, lo, None, anarchy, cand, norm, alone)
            assert np.isnan(c["best_value"][0]) and c["best_group"][0] == -1 and c["best_cand"][0] == -1 and not np.any(c["best_shift"])
