"""kiwi_hip_spectral_candidates_bootstrap without a device: the plumbing of the four entry points, the shape call, and the numpy
restatement (tests/spectral_candidates_bootstrap_restatement.py) on hand-made slot arrays -- that it IS tests/outer_restatement.py
on the flattened sources, the ties, a group of zero norms, the excluded draws.  The device is pinned to the host route and to the
restatement bit for bit in tests/test_spectral_candidates_bootstrap_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib
from tests import outer_restatement as orr
from tests import spectral_candidates_bootstrap_restatement as sbr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_spectral_candidates_bootstrap", "kiwi_hip_spectral_candidates_bootstrap_params",
           "kiwi_hip_get_spectral_candidates_bootstrap_ms", "kiwi_hip_spectral_candidates_bootstrap_shape"]
# seven slots on five receivers: receivers of 1, 2 and 3 slots, receiver 3 without slots (disabled), receiver 4 of one
SLOT_RECEIVER = np.array([0, 1, 1, 2, 2, 2, 4], np.int32)
NREC = 5


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
    # the waveform sibling's lists without k0, kstep, nk and without the two *_offset arrays
    assert len(L.kiwi_hip_spectral_candidates_bootstrap.argtypes) == len(L.kiwi_hip_waveform_candidates_bootstrap.argtypes) - 5 == 17
    assert len(L.kiwi_hip_spectral_candidates_bootstrap_params.argtypes) == len(L.kiwi_hip_waveform_candidates_bootstrap_params.argtypes) - 5 == 19
    assert L.kiwi_hip_get_spectral_candidates_bootstrap_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert L.kiwi_hip_spectral_candidates_bootstrap_shape.argtypes == [C.c_int, klib.c_int_p, klib.c_int_p, klib.c_int_p]
    assert "kiwi_hip_spectral_candidates_bootstrap_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    assert kmax == 8
    for K in range(1, kmax + 1):
        c, t, r = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_spectral_candidates_bootstrap_shape(K, C.byref(c), C.byref(t), C.byref(r)) == 0
        assert (c.value, t.value, r.value) == (256, 16, 70)
        # the bootstrap kernel is the waveform sibling's: its shape is that one's
        c2, t2, r2 = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_bootstrap_shape(K, C.byref(c2), C.byref(t2), C.byref(r2)) == 0
        assert (c.value, t.value, r.value) == (c2.value, t2.value, r2.value)
    c, t, r = C.c_int(), C.c_int(), C.c_int()
    for K in (0, 9):
        assert L.kiwi_hip_spectral_candidates_bootstrap_shape(K, C.byref(c), C.byref(t), C.byref(r)) != 0
    assert L.kiwi_hip_spectral_candidates_bootstrap_shape(6, None, C.byref(t), C.byref(r)) != 0
    assert L.kiwi_hip_spectral_candidates_bootstrap_shape(6, C.byref(c), None, C.byref(r)) != 0
    assert L.kiwi_hip_spectral_candidates_bootstrap_shape(6, C.byref(c), C.byref(t), None) != 0


# ------------------------------------------------------------------------------------------------ the restatement
def _slots(rng, ng, ncand):
    """(slot_misfit [ng, ncand, nmis], slot_norm [ng, nmis]) float32, positive"""
    nmis = len(SLOT_RECEIVER)
    return (rng.uniform(0.1, 2.0, (ng, ncand, nmis)).astype(np.float32), rng.uniform(0.5, 2.0, (ng, nmis)).astype(np.float32))


def _draws(rng, skipped):
    """ones, two resampled rows, all zeros, a row that is non-zero only on the skipped receivers"""
    dw = np.ones((5, NREC))
    dw[1:3] = rng.multinomial(NREC, np.full(NREC, 1.0 / NREC), size=2)
    dw[3] = 0.0
    dw[4] = 0.0
    dw[4, skipped] = 2.0
    return dw


def test_restatement_is_outer_restatement_on_the_flattened_sources():
    rng = np.random.default_rng(31)
    ng, ncand = 3, 7
    m, n = _slots(rng, ng, ncand)
    n[:, 0] = 0.0                                             # receiver 0: no reference energy
    m[:, :, 0] = 0.25
    w = np.array([1.0, 0.0, 2.0, 0.0, 1.5])                   # receiver 1: weight 0; receiver 3 has no slots
    dw = _draws(rng, [1, 3])
    dw[1:3] = [[2, 0, 1, 1, 1], [0, 1, 3, 0, 1]]               # (resampled rows in which a counted receiver is drawn)
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            got = sbr.from_slots(m, n, SLOT_RECEIVER, NREC, np.zeros(ng, np.int32), dw, norm, w, anarchy)
            flat_m = m.reshape(ng * ncand, -1)
            flat_n = np.repeat(n, ncand, axis=0)
            bv, bi, _ = orr.outer_misfits(flat_m, flat_n, SLOT_RECEIVER, NREC, norm, w, anarchy, dw)
            assert np.array_equal(got["best_value"], bv, equal_nan=True)
            has = ~np.isnan(bv)
            assert np.array_equal(has, [True, True, True, False, False])        # zeros; only skipped receivers: excluded
            assert np.array_equal((got["best_group"] * ncand + got["best_cand"])[has], bi[has])        # the index taken apart
            assert np.all((got["best_cand"][has] >= 0) & (got["best_cand"][has] < ncand))
            for name in ("best_group", "best_offset", "best_cand"):
                assert np.all(got[name][~has] == -1) and got[name].dtype == np.int32
            assert np.all(got["best_offset"][has] == 0)                         # there are no offsets
            assert np.all(np.isnan(got["group_value"][:, 3:])) and np.all(got["group_cand"][:, 3:] == -1)
            for g in range(ng):
                gv, gi, _ = orr.outer_misfits(flat_m[g * ncand:(g + 1) * ncand], flat_n[g * ncand:(g + 1) * ncand], SLOT_RECEIVER, NREC, norm, w,
                                              anarchy, dw)
                assert np.array_equal(got["group_value"][g], gv, equal_nan=True)
                assert np.array_equal(got["group_cand"][g][has], gi[has])
            # the call's best is the best of the groups' bests, the lower group among equals
            for d in np.nonzero(has)[0]:
                g = got["best_group"][d]
                assert got["group_value"][g, d] == got["best_value"][d] == np.nanmin(got["group_value"][:, d])
                assert got["group_cand"][g, d] == got["best_cand"][d]
            # a draw of ones under l1norm without anarchy, by hand: the slots of a receiver summed, the receivers weighted
            if norm == "l1norm" and not anarchy:
                M = np.stack([flat_m[:, SLOT_RECEIVER == r].astype(np.float64).sum(1) for r in range(NREC)], 1)
                N = np.stack([flat_n[:, SLOT_RECEIVER == r].astype(np.float64).sum(1) for r in range(NREC)], 1)
                assert np.allclose(got["best_value"][0], np.min((M * w).sum(1) / (N * w).sum(1)), rtol=1e-12)


def test_ties_go_to_the_lowest_group_and_candidate():
    rng = np.random.default_rng(32)
    ncand = 5
    m, n = _slots(rng, 1, ncand)
    m[0, 3] = m[0, 1]                                         # two identical candidates
    m = np.tile(m, (2, 1, 1))                                 # two groups with identical slot misfits
    n = np.tile(n, (2, 1))
    dw = np.concatenate([np.ones((1, NREC)), rng.multinomial(NREC, np.full(NREC, 1.0 / NREC), size=6)])
    for norm in ("l1norm", "l2norm"):
        got = sbr.from_slots(m, n, SLOT_RECEIVER, NREC, [0, 0], dw, norm, None, True)
        assert np.all(got["best_group"] == 0) and np.all(got["best_cand"] != 3)
        assert np.array_equal(got["group_value"][0], got["group_value"][1]) and np.array_equal(got["group_cand"][0], got["group_cand"][1])
        # the same candidates in the opposite order: the tie still goes to the lower index, now the other copy
        back = sbr.from_slots(m[:, ::-1], n, SLOT_RECEIVER, NREC, [0, 0], dw, norm, None, True)
        assert np.array_equal(back["best_value"], got["best_value"]) and np.all(back["best_cand"] != 3)
        assert np.array_equal(back["best_cand"], np.where(got["best_cand"] == 1, 1, 4 - got["best_cand"]))


def test_a_group_of_zero_norms_is_excluded_from_every_draw():
    """what the parent call leaves for a group with status 2: slot norms and slot misfits of zeros"""
    rng = np.random.default_rng(33)
    m, n = _slots(rng, 2, 4)
    n[0] = 0.0
    m[0] = 0.0
    dw = _draws(rng, [3])
    for norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            got = sbr.from_slots(m, n, SLOT_RECEIVER, NREC, [2, 0], dw, norm, None, anarchy)
            assert list(got["status"]) == [2, 0]
            assert np.all(np.isnan(got["group_value"][0])) and np.all(got["group_cand"][0] == -1)
            assert np.all(got["best_group"][:3] == 1) and np.all(got["best_group"][3:] == -1) and np.all(np.isnan(got["best_value"][3:]))


def test_a_draw_of_zeros_answers_nan_and_minus_one():
    rng = np.random.default_rng(34)
    m, n = _slots(rng, 2, 3)
    got = sbr.from_slots(m, n, SLOT_RECEIVER, NREC, [0, 0], np.zeros((1, NREC)), "l1norm")
    assert np.isnan(got["best_value"][0]) and np.all(np.isnan(got["group_value"][:, 0]))
    assert got["best_group"][0] == -1 and got["best_cand"][0] == -1 and np.all(got["group_cand"][:, 0] == -1)
    # the host route itself writes index 0 there: the one deliberate difference
    bv, bi, _ = orr.outer_misfits(m.reshape(6, -1), np.repeat(n, 3, axis=0), SLOT_RECEIVER, NREC, "l1norm", None, False, np.zeros((1, NREC)))
    assert np.isnan(bv[0]) and bi[0] == 0
