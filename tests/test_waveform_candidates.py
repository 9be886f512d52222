"""kiwi_hip_waveform_candidates without a device: the numpy restatement of the device arithmetic
(tests/waveform_candidates_restatement.py) on hand-made traces -- a unit candidate, the synthetics factor, a zero-weight receiver,
a receiver without reference energy, anarchy, both outer norms, ties --, the maths against the CPU oracle's own l1norm and l2norm
evaluation of 40 double couples, the fold against tests/outer_restatement.py, method 1 against the Gram route's restatement, and
the plumbing of the new entry points.  The device is pinned to the restatement bit for bit in
tests/test_waveform_candidates_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import lib as klib, synthetic
from tests import linfit_candidates_restatement as lc
from tests import linfit_restatement as lr
from tests import outer_restatement as outer
from tests import waveform_candidates_restatement as wr
from tests.common import MISFIT_RTOL, SYN_RTOL, Scenario
from tests.linfit_cases import UNIT, basis_rows, mt_row, oracle_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_waveform_candidates", "kiwi_hip_waveform_candidates_params", "kiwi_hip_get_waveform_candidates_ms",
           "kiwi_hip_waveform_candidates_shape"]
COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # tests/test_linfit_gpu.py's receivers of 1 to 5 components
F32 = np.float32
DT = 0.5

ROWS = np.array([[1., 2., 3., 4.], [1., 1., 1., 1.]], F32)   # two basis rows of a slot; every operation below is exact


def _one(rows, ref, norm, x, method, outer_norm="l1norm", w=(1.0,), anarchy=False, syn_factor=1.0):
    """a group of one slot"""
    return wr.evaluate([np.asarray(rows, F32)[None]], [np.asarray(ref, F32)], [[norm]], [0], w, anarchy, x, method, outer_norm, DT, syn_factor)


# ------------------------------------------------------------------------------------------------ C1: hand-made traces
def test_unit_candidate_returns_the_rows_own_misfit():
    ref = np.array([2., 2., 2., 2.], F32)
    for a in range(2):
        d = ref.astype(np.float64) - ROWS[a]
        own = {1: F32(np.sqrt(DT * np.sum(d * d))), 2: F32(DT * np.sum(np.abs(d)))}
        for method in (1, 2):
            out = _one(ROWS, ref, 4.0, np.eye(2), method)
            assert out["slot_misfit"][0, a, 0] == own[method]
            assert out["misfit"][0, a] == float(own[method]) / 4.0             # one slot: m / n
    # e_0: d = 1, 0, -1, -2; e_1: d = 1, 1, 1, 1
    out = _one(ROWS, ref, 4.0, np.eye(2), 2)
    assert list(out["slot_misfit"][0, :, 0]) == [2.0, 2.0] and out["best_index"][0] == 0 and out["status"][0] == 0
    out = _one(ROWS, ref, 4.0, np.eye(2), 1)
    assert list(out["slot_misfit"][0, :, 0]) == [F32(np.sqrt(3.0)), F32(np.sqrt(2.0))] and out["best_index"][0] == 1
    assert out["best_misfit"][0] == out["misfit"][0, 1]
    # a combination, x = (2, -3): v = -1, 1, 3, 5; d = 3, 1, -1, -3
    out = _one(ROWS, ref, 4.0, [[2.0, -3.0]], 2)
    assert out["slot_misfit"][0, 0, 0] == 4.0
    out = _one(ROWS, ref, 4.0, [[2.0, -3.0]], 1)
    assert out["slot_misfit"][0, 0, 0] == F32(np.sqrt(10.0))
    # the candidate is rounded to fp32 before anything else
    x = 1.0 + 2.0 ** -30
    assert _one(ROWS, ROWS[0], 1.0, [[x, 0.0]], 2)["slot_misfit"][0, 0, 0] == 0.0


def test_synthetics_factor_scales_the_synthetic_side_only():
    for method in (1, 2):
        assert _one(ROWS, 2.0 * ROWS[0], 1.0, [[1.0, 0.0]], method, syn_factor=2.0)["slot_misfit"][0, 0, 0] == 0.0
        assert _one(ROWS, ROWS[0], 1.0, [[1.0, 0.0]], method, syn_factor=2.0)["slot_misfit"][0, 0, 0] > 0.0
    # d = 1.f a - 2 v = -1, -2, -3, -4 for a = v
    assert _one(ROWS, ROWS[0], 1.0, [[1.0, 0.0]], 2, syn_factor=2.0)["slot_misfit"][0, 0, 0] == 5.0


def test_outer_fold_weights_anarchy_and_receivers_that_do_not_count():
    # receiver 0: two slots, receiver 1: weight 0 or 3, receiver 2: no reference energy (norm factor 0).  Under l1norm inside, x = e_0
    # has the slot misfits 2, 1, 3, 0.5
    syn = [ROWS[None]] * 4
    ref = [np.array(r, F32) for r in ([2., 2., 2., 2.], [1., 2., 3., 2.], [2., 3., 4., 7.], [1., 2., 3., 3.])]
    norm, rec = [[4.0, 1.0, 5.0, 0.0]], [0, 0, 1, 2]
    x = [[1.0, 0.0]]
    for w1 in (0.0, 3.0):
        w = [2.0, w1, 1.0]
        out = wr.evaluate(syn, ref, norm, rec, w, False, x, 2, "l1norm", DT)
        assert list(out["slot_misfit"][0, 0]) == [2.0, 1.0, 3.0, 0.5]
        assert out["misfit"][0, 0] == (((2.0 + 1.0) * 2.0 + 3.0 * w1) + 0.5 * 1.0) / (((4.0 + 1.0) * 2.0 + 5.0 * w1) + 0.0)
        out = wr.evaluate(syn, ref, norm, rec, w, False, x, 2, "l2norm", DT)
        M0, N0 = np.sqrt(4.0 + 1.0), np.sqrt(16.0 + 1.0)
        want = np.sqrt((((M0 * 2.0) ** 2 + (3.0 * w1) ** 2) + (0.5 * 1.0) ** 2) / (((N0 * 2.0) ** 2 + (5.0 * w1) ** 2) + 0.0))
        assert out["misfit"][0, 0] == want
        # anarchy: rw = w / N; the receiver without reference energy gets the weight 0
        out = wr.evaluate(syn, ref, norm, rec, w, True, x, 2, "l1norm", DT)
        r0, r1 = 2.0 / 5.0, w1 / 5.0
        assert out["misfit"][0, 0] == ((3.0 * r0 + 3.0 * r1) + 0.5 * 0.0) / ((5.0 * r0 + 5.0 * r1) + 0.0)
    # no receiver counts: NaN, no winner, status 1
    out = wr.evaluate(syn, ref, norm, rec, [0.0, 0.0, 1.0], False, x, 2, "l2norm", DT)
    assert out["status"][0] == 1 and out["best_index"][0] == -1 and np.isnan(out["best_misfit"][0]) and np.isnan(out["misfit"][0, 0])
    # among equal misfits the lowest index wins
    out = wr.evaluate(syn, ref, norm, rec, [1.0, 1.0, 1.0], False, [[0.0, 3.0], [1.0, 0.0], [1.0, 0.0]], 2, "l1norm", DT)
    assert out["misfit"][0, 1] == out["misfit"][0, 2] < out["misfit"][0, 0] and out["best_index"][0] == 1


# ------------------------------------------------------------------------------------------------ C2: against the oracle
PLANTED_SDR = (40.0, 60.0, 100.0, 5e18)
NCAND = 40
_ORACLE = {}


def oracle_case(method):
    """the oracle's tapered traces of the six elementary tensors, its norm factors and its own slot misfits of the 40 combined
    sources and of the six elementary ones under `method`; made once per method and shared"""
    if method in _ORACLE:
        return _ORACLE[method]
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    sc.apply_setup(e, True)
    e.set_misfit_method(method)
    basis = basis_rows("moment_tensor", mt_row(np.zeros(6)))
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis, 6)
    own = []
    for row in basis:
        e.set_source_params(6, row)
        own.append(e.get_misfits()[0])
    rng = np.random.default_rng(77)
    sdr = np.stack([rng.uniform(0., 360., NCAND), rng.uniform(0., 90., NCAND), rng.uniform(-180., 180., NCAND)], 1)
    sdr[0] = PLANTED_SDR[:3]
    tensors = np.array([synthetic.mt_from_sdr(s, d, r, PLANTED_SDR[3]) for s, d, r in sdr]).astype(np.float32)
    m, n, g = [], [], []
    for t in tensors:
        e.set_source_params(6, mt_row(t))
        mi, ni, gi = e.get_misfits()
        m.append(mi), n.append(ni), g.append(gi)
    e.close()
    case = dict(dt=sc.gf["dt"], nrec=sc.nrec, syn=syn, ref=ref, receivers=receivers, slot_receiver=[r for r, sl in enumerate(receivers) for _ in sl],
                own=np.array(own), cand=tensors.astype(np.float64) / UNIT, m=np.array(m, np.float64), n=np.array(n, np.float64), g=np.array(g, np.float64))
    for a in (case["syn"], case["ref"], case["own"], case["cand"], case["m"], case["n"], case["g"]):
        for b in (a if isinstance(a, list) else [a]):
            b.setflags(write=False)
    _ORACLE[method] = case
    return case


@pytest.mark.parametrize("method", [1, 2])
def test_predicted_slot_misfits_against_the_oracle(method):
    """Tapered synthetics of the six elementary tensors from the CPU oracle; 40 random double couples, the planted one first,
    through the restatement; every slot misfit against the oracle's own evaluation of the combined `moment_tensor` source.

    Bound per slot: MISFIT_RTOL max(m, n) + SYN_RTOL T (sum_a |xf_a| max|s_a| + max|v|), T = dt wlen under l1norm and
    sqrt(dt wlen) under l2norm: the comparison itself within the suite's rule, and the two traces -- the synthesis of the combined
    source and the combination of the six -- each within SYN_RTOL of their scale at every sample."""
    name = {1: "l2norm", 2: "l1norm"}[method]
    c = oracle_case(method)
    dt, syn, ref = c["dt"], c["syn"], c["ref"]
    assert len(ref) == 18 and set(len(r) for r in ref) <= {259, 260}
    out = wr.evaluate(syn, ref, c["n"][:1], c["slot_receiver"], np.ones(c["nrec"]), False, c["cand"], method, "l2norm", dt)
    xf = c["cand"].astype(F32).astype(np.float64)
    m, n = c["m"], c["n"]
    bound = MISFIT_RTOL * np.maximum(m, n)
    for j in range(len(ref)):
        wlen = len(ref[j])
        T = dt * wlen if method == 2 else np.sqrt(dt * wlen)
        top = np.abs(xf) @ np.max(np.abs(syn[j][0].astype(np.float64)), axis=1)
        v = np.max(np.abs(wr.combine(syn[j][0], xf).astype(np.float64)), axis=1)
        bound[:, j] += SYN_RTOL * T * (top + v)
    dm = np.abs(out["slot_misfit"][0].astype(np.float64) - m)
    print("%s: %d slots, windows of %s samples, largest |dm| / max(m, n) %.3g, largest |dm| / bound %.3g" % (
        name, len(ref), sorted(set(len(r) for r in ref)), np.max(dm / np.maximum(m, n)), np.max(dm / bound)))
    assert np.all(dm <= bound)
    # the global misfit of the fold is the oracle's
    assert np.all(np.abs(out["misfit"][0] - c["g"]) <= 4 * MISFIT_RTOL * np.sqrt(c["g"] ** 2 + 1.0))
    assert out["best_index"][0] == 0 or out["misfit"][0, out["best_index"][0]] <= out["misfit"][0, 0]
    # the unit candidates: v = s_a exactly, and the oracle's own slot misfits of the six elementary sources bit for bit
    unit = wr.slot_misfits_of(syn, ref, np.eye(6), method, dt)
    assert unit.shape == (1, 6, 18) and np.array_equal(unit[0], c["own"].astype(F32))


# ------------------------------------------------------------------------------------------------ C3: the fold
def test_fold_equals_the_outer_restatement_on_its_own_slots():
    rng = np.random.default_rng(3)
    rec = [0, 1, 1, 2, 2, 2, 3, 4, 4]                        # receiver 5 of six has no slots
    nrec, nc = 6, 50
    smis = rng.uniform(0.0, 3.0, (nc, len(rec))).astype(F32)
    norm = rng.uniform(0.5, 2.0, len(rec)).astype(F32)
    norm[6] = 0.0                                             # receiver 3 without reference energy
    smis[7, :] = 0.0
    w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
    for outer_norm in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            for weights in (w, np.zeros(6)):
                mine, status = wr.fold(smis, norm, rec, weights, anarchy, outer_norm)
                bv, bi, theirs = outer.outer_misfits(smis, np.tile(norm, (nc, 1)), rec, nrec, outer_norm, weights, anarchy, which_draw=0)
                assert np.array_equal(mine, theirs, equal_nan=True), (outer_norm, anarchy)
                i, v = wr.best_of(mine[None])
                if status == 0:
                    assert i[0] == bi[0] and v[0] == bv[0]
                else:
                    assert i[0] == -1 and np.isnan(bv[0]) and np.all(np.isnan(mine))


# ------------------------------------------------------------------------------------------------ C4: against the Gram route
def test_l2norm_from_the_residual_against_the_gram_route():
    """Under the outer l2norm the per-slot fold and the Gram route's receiver-level fold are the same quantity,
    g = sqrt(sum_r w_r^2 |d_r - v_r|^2 / sum_r w_r^2 |d_r|^2).  With candidates that are exact in fp32 both restatements evaluate
    the same coefficients on the same traces; each lies within the suite's rule for global misfits of g, MISFIT_RTOL sqrt(g^2 + 1)."""
    c = oracle_case(1)
    dt, syn, ref = c["dt"], c["syn"], c["ref"]
    rng = np.random.default_rng(5)
    cand = np.concatenate([c["cand"], rng.uniform(-5.0, 5.0, (60, 6))]).astype(F32).astype(np.float64)
    w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
    fit = lr.fit(syn, ref, c["receivers"], dt, w)
    worst = 0.0
    for anarchy in (False, True):
        gram = lc.evaluate(fit["by_receiver"], lr.fit(syn, ref, c["receivers"], dt, w, anarchy)["normal"], w, anarchy, cand, "l2norm")
        wave = wr.evaluate(syn, ref, c["n"][:1], c["slot_receiver"], w, anarchy, cand, 1, "l2norm", dt)
        ratio = np.abs(wave["misfit"][0] - gram["misfit"][0]) / (MISFIT_RTOL * np.sqrt(gram["misfit"][0] ** 2 + 1.0))
        worst = max(worst, float(np.max(ratio)))
        assert np.all(ratio <= 1.0), (anarchy, np.max(ratio))
    print("l2norm from the residual against the Gram route: largest |dg| / (MISFIT_RTOL sqrt(g^2 + 1)) %.3g" % worst)


# ------------------------------------------------------------------------------------------------ C5: plumbing
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
    assert len(L.kiwi_hip_waveform_candidates.argtypes) == 15
    assert len(L.kiwi_hip_waveform_candidates_params.argtypes) == 17
    assert L.kiwi_hip_get_waveform_candidates_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_waveform_candidates_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device_and_a_stage_fits_the_lds():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    shapes = set()
    for K in range(1, kmax + 1):
        c, s = C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_shape(K, C.byref(c), C.byref(s)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and s.value >= 64
        # a stage: per sample the K rows and the reference side, padded to whole 16-byte reads; well inside 64 KiB
        assert s.value * 4 * ((K + 1 + 3) // 4 * 4) <= 16 * 1024
        shapes.add((c.value, s.value))
    assert len(shapes) == 1
    c, s = C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_waveform_candidates_shape(K, C.byref(c), C.byref(s)) != 0
    assert L.kiwi_hip_waveform_candidates_shape(6, None, C.byref(s)) != 0
    assert L.kiwi_hip_waveform_candidates_shape(6, C.byref(c), None) != 0
