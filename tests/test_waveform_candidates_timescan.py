"""kiwi_hip_waveform_candidates_time_scan without a device: the plumbing of the new entry points; the numpy restatement of the
device arithmetic (tests/waveform_candidates_timescan_restatement.py) on hand-made rows -- the offset reads the combined trace k
samples earlier under the fixed taper, the fold over the offsets takes the first minimum and passes over NaN --; and the maths
against the CPU oracle: the restatement on the oracle's untapered rows against the oracle's own evaluation of the combined tensor
with references and tapers moved by -k samples (route B of the time scans), and the unit candidates against the oracle's misfits
of the basis sources at that offset.  Only the plumbing tests run the built library; the others validate the DEFINITION -- the
restatement against the oracle -- and need no kernel.  The device is pinned to the restatement bit for bit in
tests/test_waveform_candidates_timescan_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import lib as klib
from tests import waveform_candidates_restatement as wr
from tests import waveform_candidates_timescan_restatement as wtr
from tests.common import misfit_close
from tests.linfit_cases import UNIT, mt_row
from tests.test_linfit_timescan import LOCATION, _basis, _fresh, _raw_rows, _scenario
from tests.test_waveform_candidates_gpu import slot_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_waveform_candidates_time_scan", "kiwi_hip_waveform_candidates_time_scan_params",
           "kiwi_hip_get_waveform_candidates_time_scan_ms", "kiwi_hip_waveform_candidates_time_scan_shape",
           "kiwi_hip_waveform_candidates_time_scan_rows"]
F32 = np.float32
DT = 0.5
NAMES = {1: "l2norm", 2: "l1norm"}


# ------------------------------------------------------------------------------------------------ C1: the plumbing
def test_symbols_are_exported_mapped_declared_in_the_ctypes_table_and_bound_in_fortran():
    L = klib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", klib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in dyn.splitlines() if line.strip())
    text = open(os.path.join(ROOT, "kiwi_amd", "csrc", "kiwi_hip.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    globs = re.search(r"global:(.*?);\s*local:", text, re.S).group(1).replace(";", " ").split()
    declared = klib.declared_symbols()
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    header = open(os.path.join(ROOT, "include", "kiwi_hip.h")).read()
    for s in SYMBOLS:
        assert s in exported, s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        assert s in declared, s
        f = getattr(L, s)
        assert f.restype is C.c_int and f.argtypes is not None, s
        assert "name='%s'" % s in binding, s
        # the ctypes table has as many arguments as the header's prototype
        proto = re.search(r"\bint %s\((.*?)\);" % s, header, re.S).group(1)
        assert len(f.argtypes) == len(proto.split(",")), s
    assert len(L.kiwi_hip_waveform_candidates_time_scan.argtypes) == 22
    assert len(L.kiwi_hip_waveform_candidates_time_scan_params.argtypes) == 24
    assert L.kiwi_hip_get_waveform_candidates_time_scan_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_waveform_candidates_time_scan_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()
    makefile = open(os.path.join(ROOT, "kiwi_amd", "csrc", "Makefile")).read()
    assert "kiwi_waveform_candidates_timescan.hpp" in makefile


def test_shape_answers_without_a_device():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    for K in range(1, kmax + 1):
        c, s, j = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_time_scan_shape(K, C.byref(c), C.byref(s), C.byref(j)) == 0
        pc, ps = C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_shape(K, C.byref(pc), C.byref(ps)) == 0
        assert (c.value, s.value) == (pc.value, ps.value)                 # the parent's tile and stage
        # a staged sample -- K row values and J (taper, reference) pairs -- is whole 16-byte reads with less than one pair to spare
        assert j.value >= 8 and (K + 2 * j.value + 3) // 4 * 4 - (K + 2 * j.value) < 2 and K + 2 * (j.value - 1) < K + 16 + 3
    for K in (0, kmax + 1):
        assert L.kiwi_hip_waveform_candidates_time_scan_shape(K, C.byref(c), C.byref(s), C.byref(j)) != 0


# ------------------------------------------------------------------------------------------------ C2: hand-made rows
def test_an_offset_reads_the_combined_trace_k_samples_earlier_under_the_fixed_taper():
    S = 2
    raw = np.array([[[9., 8., 1., 2., 3., 4., 7., 6.], [5., 5., 1., 1., 1., 1., 5., 5.]]], F32)        # [1, K = 2, wlen 4 + 2 S]
    taper = np.array([1., 0.5, 0.5, 1.], F32)
    ref = np.array([2., 1., 1., 2.], F32)
    ks = [-2, 0, 1]
    sm = wtr.slot_misfits_of([raw], [taper], [ref], np.eye(2), 2, DT, S, ks)
    assert sm.shape == (1, 3, 2, 1)
    # e_0: k = 0: u = 1 2 3 4, vt = 1 1 1.5 4, d = 1 0 -.5 -2;  k = 1: u = 8 1 2 3, vt = 8 .5 1 3;  k = -2: u = 3 4 7 6, vt = 3 2 3.5 6
    assert list(sm[0, :, 0, 0]) == [F32(DT * (1 + 1 + 2.5 + 4)), F32(DT * 3.5), F32(DT * (6 + .5 + 0 + 1))]
    # the synthetics factor scales the synthetic side only: 1.f ref - 2 vt
    sm2 = wtr.slot_misfits_of([raw], [taper], [ref], np.eye(2), 2, DT, S, [0], syn_factor=2.0)
    assert sm2[0, 0, 0, 0] == F32(DT * (0 + 1 + 2 + 6))
    # l2norm: the root of dt times the sum of squares
    sm3 = wtr.slot_misfits_of([raw], [taper], [ref], np.eye(2), 1, DT, S, [0])
    assert sm3[0, 0, 0, 0] == F32(np.sqrt(DT * (1 + 0 + .25 + 4)))
    # a sample outside the window contributes nothing, also where the combined trace is not finite there
    bad = raw.copy()
    bad[0, 0, 0] = np.nan                                    # extended sample -2: read by k = 2 only
    bad[0, 0, 7] = np.inf                                    # extended sample 5: read by k = -2 only
    a = wtr.slot_misfits_of([bad], [taper], [ref], np.eye(2), 2, DT, S, [-1, 0, 1])
    b = wtr.slot_misfits_of([raw], [taper], [ref], np.eye(2), 2, DT, S, [-1, 0, 1])
    assert np.array_equal(a, b)
    # offset 0 of a unit candidate is the parent's restatement on the tapered row
    tapered = (raw[:, :, S:S + 4] * taper).astype(F32)
    for method in (1, 2):
        mine = wtr.slot_misfits_of([raw], [taper], [ref], np.eye(2), method, DT, S, [0])[:, 0]
        assert np.array_equal(mine, wr.slot_misfits_of([tapered], [ref], np.eye(2), method, DT))


def test_fold_over_the_offsets_first_minimum_nan_passed_over_and_statuses():
    # one slot per receiver, two receivers; norm factors 2 and 4: misfit = (m0 + m1) / 6 under l1norm
    smis = np.zeros((2, 4, 3, 2), F32)
    smis[0, :, :, 0] = [[3, 6, 9], [1.5, 6, 3], [1.5, 3, 3], [3, 3, 12]]
    smis[1] = 6.0
    norm = np.array([[2.0, 4.0], [2.0, 4.0]], F32)
    out = wtr.fold_offsets(smis, norm, [0, 1], [1.0, 1.0], False, "l1norm")
    assert out["misfit"].shape == (2, 4, 3) and list(out["status"]) == [0, 0]
    assert np.array_equal(out["misfit"][0], np.array([[.5, 1, 1.5], [.25, 1, .5], [.25, .5, .5], [.5, .5, 2]]))
    assert list(out["best_index"][0]) == [0, 0, 0, 0] and list(out["best_misfit"][0]) == [.5, .25, .25, .5]
    assert out["best_offset"][0] == 1                                     # the first of the two smallest
    assert list(out["cand_offset"][0]) == [1, 2, 1] and list(out["cand_misfit"][0]) == [.25, .5, .5]
    assert out["best_offset"][1] == 0 and list(out["cand_offset"][1]) == [0, 0, 0]       # all equal: the lowest index
    # a NaN is passed over, wherever it stands; an offset whose candidates are all NaN has no winner and never is the best offset
    smis[0, 1, 0, 0] = np.nan
    smis[0, 0, :, 0] = np.nan
    out = wtr.fold_offsets(smis, norm, [0, 1], [1.0, 1.0], False, "l1norm")
    assert out["best_index"][0, 0] == -1 and np.isnan(out["best_misfit"][0, 0])
    assert out["best_index"][0, 1] == 2 and out["best_misfit"][0, 1] == .5
    assert out["best_offset"][0] == 2 and list(out["cand_offset"][0]) == [2, 2, 1]
    assert out["status"][0] == 0                                          # (the denominator of the fold does not depend on the offset)
    # no receiver counts: status 1, NaN, no winner at any offset, no best offset
    out = wtr.fold_offsets(smis, norm, [0, 1], [0.0, 0.0], False, "l2norm")
    assert list(out["status"]) == [1, 1] and np.all(out["best_index"] == -1) and np.all(out["best_offset"] == -1)
    assert np.all(np.isnan(out["misfit"])) and np.all(out["cand_offset"] == -1) and np.all(np.isnan(out["cand_misfit"]))
    # (status 2, a basis source that failed to discretise, is set by the library's host code, which needs a device to be reached:
    # tests/test_waveform_candidates_timescan_gpu.py test_a_failed_basis_source_gives_its_group_status_two)


# ------------------------------------------------------------------------------------------------ C3: against the oracle
KS = (-3, 0, 5)
S = 5
NCAND = 6
_CASE = {}


def oracle_case():
    """the oracle's untapered rows of the six elementary tensors over the windows made S samples wider, its taper weights and
    tapered references; per offset k, method and synthetics factor its own slot misfits (and norm factors) of NCAND combined
    tensors and of the six elementary ones with references and tapers moved by -k samples.  Made once and shared"""
    if _CASE:
        return _CASE
    sc = _scenario(LOCATION[0] + 2 * DT)                     # the references: the planted tensor two samples later than the basis
    assert sc.gf["dt"] == DT
    raw, taper, ref, _ = _raw_rows(sc, _basis(), S)
    rng = np.random.default_rng(91)
    cand = rng.uniform(-2.0, 2.0, (NCAND, 6)).astype(F32)
    sources = [mt_row((x.astype(np.float64) * UNIT).astype(F32), location=LOCATION, risetime=0.5) for x in cand] + list(_basis())
    mis = {}
    for k in KS:
        e = _fresh(sc, ref_shift=-k, taper_shift=-k * DT)
        for method in (1, 2):
            e.set_misfit_method(method)
            for factor in (1.0, 0.75):
                e.set_synthetics_factor(factor)
                m, n = [], []
                for row in sources:
                    e.set_source_params(6, row)
                    mi, ni, _ = e.get_misfits()
                    m.append(np.array(mi, np.float64)), n.append(np.array(ni, np.float64))
                mis[(k, method, factor)] = (np.array(m), np.array(n))
        e.close()
    _CASE.update(dt=DT, raw=raw, taper=taper, ref=ref, cand=cand.astype(np.float64), mis=mis)
    for a in raw + taper + ref:
        a.setflags(write=False)
    return _CASE


@pytest.mark.parametrize("factor", [1.0, 0.75])
@pytest.mark.parametrize("method", [1, 2])
def test_restatement_on_the_oracles_rows_against_the_oracle_with_references_and_tapers_moved(method, factor):
    """Bound per (candidate, slot): tests/test_waveform_candidates_gpu.py slot_bound on the rows as the offset tapers them --
    MISFIT_RTOL max(m, n) for the comparison and SYN_RTOL T (sum_a |xf_a| max|s_a| + max|v|) for the two traces."""
    c = oracle_case()
    raw, taper, ref, cand = c["raw"], c["taper"], c["ref"], c["cand"]
    sm = wtr.slot_misfits_of(raw, taper, ref, cand, method, DT, S, list(KS), factor)          # [1, nk, ncand, nmis]
    worst = 0.0
    for j, k in enumerate(KS):
        m, n = c["mis"][(k, method, factor)]
        m, n = m[:NCAND], n[:NCAND]
        assert np.array_equal(n, np.tile(c["mis"][(0, method, factor)][1][:1], (NCAND, 1))), "the norm factors do not depend on the offset"
        rows_k = [(r[0][:, S - k:S - k + len(t)] * t).astype(F32) for r, t in zip(raw, taper)]
        bound = slot_bound(NAMES[method], DT, [F32(factor) * r for r in rows_k], ref, cand, m, n)
        dm = np.abs(sm[0, j].astype(np.float64) - m)
        worst = max(worst, float(np.max(dm / bound)))
        print("%s factor %g offset %+d: largest |dm| / max(m, n) %.3g, largest |dm| / bound %.3g" % (
            NAMES[method], factor, k, np.max(dm / np.maximum(m, n)), np.max(dm / bound)))
    print("%s factor %g: largest error / bound over the offsets %.3g" % (NAMES[method], factor, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("method", [1, 2])
def test_unit_candidates_against_the_oracles_misfits_of_the_basis_sources_at_that_offset(method):
    c = oracle_case()
    for factor in (1.0, 0.75):
        sm = wtr.slot_misfits_of(c["raw"], c["taper"], c["ref"], np.eye(6), method, DT, S, list(KS), factor)
        for j, k in enumerate(KS):
            m, n = c["mis"][(k, method, factor)]
            assert misfit_close(sm[0, j], m[NCAND:], norm=n[NCAND:]), (method, factor, k)
