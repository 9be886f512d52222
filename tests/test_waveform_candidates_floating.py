"""kiwi_hip_waveform_candidates_floating without a device: the numpy restatement of the device arithmetic
(tests/waveform_candidates_floating_restatement.py) on hand-made traces -- every range (0, 0) against the plain restatement, a
planted delay, the first of equal minima, the receiver's sum deciding the shift --, the maths against the CPU oracle's own
floating_l1norm and floating_l2norm evaluation of the six unit candidates and 40 double couples, and the plumbing of the new entry
points.  The device is pinned to the restatement bit for bit in tests/test_waveform_candidates_floating_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import lib as klib, synthetic
from tests import waveform_candidates_floating_restatement as fr
from tests import waveform_candidates_restatement as wr
from tests.common import MISFIT_RTOL, SYN_RTOL, Scenario
from tests.linfit_cases import UNIT, basis_rows, mt_row, oracle_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_waveform_candidates_floating", "kiwi_hip_waveform_candidates_floating_params",
           "kiwi_hip_get_waveform_candidates_floating_ms", "kiwi_hip_waveform_candidates_floating_shape"]
COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # tests/test_linfit_gpu.py's receivers of 1 to 5 components
F32 = np.float32
DT = 0.5


# ------------------------------------------------------------------------------------------------ C1: hand-made traces
def test_every_range_of_one_shift_is_the_plain_restatement_bit_for_bit():
    rng = np.random.default_rng(1)
    rec, wlens, K, ngroup = [0, 0, 1, 2, 2, 2], [7, 7, 300, 40, 40, 40], 3, 2
    syn = [rng.standard_normal((ngroup, K, n)).astype(F32) for n in wlens]
    refx = [rng.standard_normal(n).astype(F32) for n in wlens]
    tw = [rng.uniform(0.0, 1.0, n).astype(F32) for n in wlens]
    aq = [fr.shifted_references(a, t, 1) for a, t in zip(refx, tw)]
    ref = [(a * t).astype(F32) for a, t in zip(refx, tw)]
    norm = rng.uniform(0.5, 2.0, (ngroup, len(rec))).astype(F32)
    cand = rng.uniform(-2.0, 2.0, (30, K))
    w = np.array([1.0, 0.0, 2.5])
    for method in (1, 2):
        for outer in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                for factor in (1.0, 0.75):
                    a = fr.evaluate(syn, aq, [0, 0, 0], norm, rec, w, anarchy, cand, method, outer, DT, factor)
                    b = wr.evaluate(syn, ref, norm, rec, w, anarchy, cand, method, outer, DT, factor)
                    for name in b:
                        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name], equal_nan=True), (name, method, outer, anarchy)
                    assert not np.any(a["cand_shift"]) and not np.any(a["best_shift"])


def test_a_planted_delay_per_receiver_is_returned_exactly_with_slot_misfit_zero():
    rng = np.random.default_rng(2)
    K, x0 = 3, np.array([[2.0, -1.0, 0.5]])
    rec, wlen = [0, 1, 1], 50
    ranges, planted = [(-3, 2), (1, 9)], [-1, 6]              # 6 and 9 shifts
    syn = [rng.integers(-8, 9, (1, K, wlen)).astype(F32) for _ in rec]      # (small integers: the combination is exact)
    aq = []
    for m, r in enumerate(rec):
        lo, hi = ranges[r]
        ns = hi - lo + 1
        refx = rng.integers(-8, 9, wlen + ns - 1).astype(F32)
        q0 = planted[r] - lo
        refx[ns - 1 - q0:ns - 1 - q0 + wlen] = wr.combine(syn[m][0], x0.astype(F32))[0]
        aq.append(fr.shifted_references(refx, np.ones(wlen, F32), ns))
    cand = np.concatenate([x0, rng.uniform(-2.0, 2.0, (5, K))])
    for method in (1, 2):
        out = fr.evaluate(syn, aq, [lo for lo, _ in ranges], np.ones((1, 3), F32), rec, np.ones(2), False, cand, method, "l1norm", DT)
        assert list(out["cand_shift"][0, 0]) == planted and list(out["best_shift"][0]) == planted
        assert np.all(out["slot_misfit"][0, 0] == 0.0) and out["best_index"][0] == 0 and out["best_misfit"][0] == 0.0
        assert np.all(out["slot_misfit"][0, 1:] > 0.0)
        for r, (lo, hi) in enumerate(ranges):
            assert np.all((out["cand_shift"][0, :, r] >= lo) & (out["cand_shift"][0, :, r] <= hi))


def test_the_first_of_equal_minima_wins_and_the_receivers_sum_decides():
    for method in (1, 2):
        q, mk = fr.select([np.array([[3., 1., 1., 2.]], F32)], method)
        assert q[0] == 1 and mk[0, 0] == 1.0
        # components that alone prefer shifts 0 and 1; their sum (6, 6, 4; of squares 26, 26, 8) prefers shift 2
        q, mk = fr.select([np.array([[1., 5., 2.]], F32), np.array([[5., 1., 2.]], F32)], method)
        assert q[0] == 2 and list(mk[0]) == [2.0, 2.0]
    # l1 and l2 inside can disagree: sums 4, 4.5; of squares 10, 10.25 against 3 + 1 = 4, 10 -- and 2.2 + 2.2 = 4.4, 9.68
    m = [np.array([[3., 2.2]], F32), np.array([[1., 2.2]], F32)]
    assert fr.select(m, 2)[0][0] == 0 and fr.select(m, 1)[0][0] == 1
    # a NaN sum at the first shift stays (q == 0 || sum < best, as floating_select_kernel has it)
    assert fr.select([np.array([[np.nan, 1.]], F32)], 2)[0][0] == 0
    # a constant reference: every shift has the same misfit, the range's first shift is returned
    rows = np.arange(12, dtype=F32).reshape(1, 2, 6)
    aq = [fr.shifted_references(np.full(6 + 4, 3.0, F32), np.ones(6, F32), 5)]
    out = fr.evaluate([rows], aq, [-2], np.ones((1, 1), F32), [0], np.ones(1), False, [[1.0, 0.0]], 2, "l1norm", DT)
    assert out["cand_shift"][0, 0, 0] == -2


# ------------------------------------------------------------------------------------------------ C2: against the oracle
PLANTED_SDR = (40.0, 60.0, 100.0, 5e18)
DELAYS = [2, -1, 0, 3, -2, 1]                                # whole samples by which each station's data are late
RANGES = [(-4, 2), (-1, 3), (-2, 2), (-6, 2), (-1, 4), (-3, 3)]      # 7, 5, 5, 9, 6, 7 shifts; each holds the shift -delay
NCAND = 40
PAD = 8


def _setup(noise):
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    rng = np.random.default_rng(77)
    for (ir, k), (lo, d) in list(sc.refs.items()):         # (padded: the data cover the taper at every shift of the ranges)
        padded = np.zeros(len(d) + 2 * PAD)
        padded[PAD + DELAYS[ir - 1]:PAD + DELAYS[ir - 1] + len(d)] = d
        sc.refs[(ir, k)] = (lo - PAD, (padded + noise * np.std(d) * rng.standard_normal(len(padded))).astype(np.float32))
    sc.apply_setup(e, True)
    return sc, e, rng


def _oracle_shifted_references(sc, e):
    """aq[m] [ns, wlen] from the oracle's own tapered references, its data moved by every shift of the range"""
    ns = [hi - lo + 1 for lo, hi in RANGES]
    aq = [np.zeros((ns[r], 0), F32) for r in range(sc.nrec) for _ in sc.comps[r]]
    for j in range(max(ns)):
        m = 0
        for r in range(sc.nrec):
            sh = RANGES[r][0] + min(j, ns[r] - 1)
            e.shift_ref_seismogram(r + 1, sh)
            for k in range(len(sc.comps[r])):
                a = e.reference(r + 1, k + 1, 2)[1]
                if aq[m].shape[1] == 0:
                    aq[m] = np.zeros((ns[r], len(a)), F32)
                if j < ns[r]:
                    aq[m][j] = a
                m += 1
            e.shift_ref_seismogram(r + 1, -sh)
    return aq


@pytest.mark.parametrize("method", [1, 2])
def test_receiver_minima_against_the_oracles_floating_norms(method):
    """Tapered synthetics of the six elementary tensors and the moved, tapered references from the CPU oracle; the six unit
    candidates and 40 random double couples, the planted one first, through the restatement; per receiver the minimum over the
    shifts, F = min_q f_q with f_q = sum_k m_kq under floating_l1norm and sqrt(sum_k m_kq^2) under floating_l2norm, against the
    same figure of the oracle's own evaluation of the combined `moment_tensor` source under its floating norm.

    F is 1-Lipschitz in the per-shift values: |F - F'| <= max_q |f_q - f'_q| <= sum_k max_q |m_kq - m'_kq|, so a near tie between
    two shifts cannot fail this and no case is left out.  Per slot the bound is tests/test_waveform_candidates.py's,
    MISFIT_RTOL max(m, n) + SYN_RTOL T (sum_a |xf_a| max|s_a| + max|v|), T = dt wlen (l1) or sqrt(dt wlen) (l2), with m the LARGEST
    restated m_kq over the shifts (the oracle returns only the winner's).  The shifts themselves are asserted on noise-free data
    only (test_planted_delays_on_noise_free_oracle_data)."""
    sc, e, rng = _setup(0.02)
    e.set_misfit_method(method)                                # (the plain norm: tapered traces at a given shift)
    K, dt, nrec = 6, sc.gf["dt"], sc.nrec
    syn, _, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(np.zeros(6))), K)
    aq = _oracle_shifted_references(sc, e)
    slot_r = [r for r, sl in enumerate(receivers) for _ in sl]
    sdr = np.stack([rng.uniform(0., 360., NCAND), rng.uniform(0., 90., NCAND), rng.uniform(-180., 180., NCAND)], 1)
    sdr[0] = PLANTED_SDR[:3]
    tensors = np.concatenate([np.eye(6) * UNIT, [synthetic.mt_from_sdr(s, d, r, PLANTED_SDR[3]) for s, d, r in sdr]]).astype(np.float32)
    cand = tensors.astype(np.float64) / UNIT
    xf = cand.astype(F32).astype(np.float64)
    mkq = [fr.slot_misfits_per_shift(syn[m][0], aq[m], cand, method, dt) for m in range(len(syn))]
    e.set_misfit_method({1: 7, 2: 8}[method])
    for r in range(nrec):
        e.set_floating_shiftrange(r + 1, *RANGES[r])
    worst = 0.0
    for c in range(len(cand)):
        e.set_source_params(6, mt_row(tensors[c]))
        m, n, _ = e.get_misfits()
        m, n = m.astype(np.float64), n.astype(np.float64)
        for r in range(nrec):
            sl = receivers[r]
            theirs = sum(m[k] for k in sl) if method == 2 else np.sqrt(sum(m[k] ** 2 for k in sl))
            mine = fr.receiver_minimum([mkq[k][c:c + 1] for k in sl], method)[0]
            bound = 0.0
            for k in sl:
                wlen = syn[k].shape[2]
                T = dt * wlen if method == 2 else np.sqrt(dt * wlen)
                top = np.abs(xf[c]) @ np.max(np.abs(syn[k][0].astype(np.float64)), axis=1)
                v = np.max(np.abs(wr.combine(syn[k][0], xf[c:c + 1]).astype(np.float64)))
                bound += MISFIT_RTOL * max(float(np.max(mkq[k][c])), n[k]) + SYN_RTOL * T * (top + v)
            worst = max(worst, abs(mine - theirs) / bound)
            assert abs(mine - theirs) <= bound, (c, r, mine, theirs, bound)
    e.close()
    print("%d candidates x %d receivers against the oracle's %s: largest |dF| / bound %.3g" % (
        len(cand), nrec, {1: "floating_l2norm", 2: "floating_l1norm"}[method], worst))
    assert slot_r == sorted(slot_r)


def test_planted_delays_on_noise_free_oracle_data():
    """Noise-free data late by DELAYS: the planted mechanism returns the shifts -DELAYS under both methods, where every other shift
    of a range leaves a residual"""
    sc, e, _ = _setup(0.0)
    K, dt = 6, sc.gf["dt"]
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32).astype(np.float64)[None] / UNIT
    for method in (1, 2):
        e.set_misfit_method(method)
        syn, _, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(np.zeros(6))), K)
        aq = _oracle_shifted_references(sc, e)
        slot_r = [r for r, sl in enumerate(receivers) for _ in sl]
        norm = np.ones((1, len(syn)), F32)
        out = fr.evaluate(syn, aq, [lo for lo, _ in RANGES], norm, slot_r, np.ones(sc.nrec), False, planted, method, "l1norm", dt)
        assert list(out["cand_shift"][0, 0]) == [-d for d in DELAYS] and list(out["best_shift"][0]) == [-d for d in DELAYS]
    e.close()


# ------------------------------------------------------------------------------------------------ C3: plumbing
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
    assert len(L.kiwi_hip_waveform_candidates_floating.argtypes) == 17
    assert len(L.kiwi_hip_waveform_candidates_floating_params.argtypes) == 19
    assert L.kiwi_hip_get_waveform_candidates_floating_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_waveform_candidates_floating_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device_and_a_stage_fits_the_lds():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    for K in range(1, kmax + 1):
        c, s, j = C.c_int(), C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_floating_shape(K, C.byref(c), C.byref(s), C.byref(j)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and s.value >= 64 and j.value >= 4
        # a stage: per sample the K rows and the J shifted references in whole 16-byte reads; well inside 64 KiB
        assert (K + j.value) % 4 == 0 and s.value * 4 * (K + j.value) <= 16 * 1024
        c2, s2 = C.c_int(), C.c_int()
        assert L.kiwi_hip_waveform_candidates_shape(K, C.byref(c2), C.byref(s2)) == 0 and (c2.value, s2.value) == (c.value, s.value)
    c, s, j = C.c_int(), C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_waveform_candidates_floating_shape(K, C.byref(c), C.byref(s), C.byref(j)) != 0
    assert L.kiwi_hip_waveform_candidates_floating_shape(6, None, C.byref(s), C.byref(j)) != 0
    assert L.kiwi_hip_waveform_candidates_floating_shape(6, C.byref(c), None, C.byref(j)) != 0
    assert L.kiwi_hip_waveform_candidates_floating_shape(6, C.byref(c), C.byref(s), None) != 0
