"""kiwi_hip_spectral_candidates without a device: the numpy restatement of the device arithmetic
(tests/spectral_candidates_restatement.py) on hand-made spectra -- a unit candidate, skipped bins, a zero-weight receiver, a
receiver without reference energy, anarchy, both outer norms, the free scale --, the maths against the CPU oracle's own
ampspec evaluation of 40 double couples, and the plumbing of the new entry points.  The device is pinned to the restatement bit
for bit in tests/test_spectral_candidates_gpu.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import lib as klib, synthetic
from tests import spectral_candidates_restatement as sr
from tests.common import FFT_ROUNDOFF_C, MISFIT_RTOL, Scenario, fft_roundoff_bound, slot_scales
from tests.linfit_cases import UNIT, basis_rows, mt_row, oracle_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_spectral_candidates", "kiwi_hip_spectral_candidates_params", "kiwi_hip_get_spectral_candidates_ms",
           "kiwi_hip_spectral_candidates_shape"]
COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # tests/test_linfit_gpu.py's receivers of 1 to 5 components
F32 = np.float32
DT, NT = 0.5, 64                                            # df = 1 / 32 exactly


def _slot(pairs, refamp, filtw=None, norm=1.0, K=2):
    """a slot whose first basis row holds the (re, im) `pairs`, the second one (1, 0) in every bin"""
    spec = np.zeros((len(pairs), K, 2), F32)
    spec[:, 0] = pairs
    spec[:, 1] = (1.0, 0.0)
    fw = np.ones(len(pairs), F32) if filtw is None else np.asarray(filtw, F32)
    return dict(spectra=spec, refamp=np.asarray(refamp, F32), filtw=fw, ntrans=NT, norm=F32(norm), has_filter=filtw is not None)


PYTH = [(3.0, 4.0), (-6.0, 8.0), (5.0, -12.0)]              # amplitudes 5, 10, 13: every operation below is exact


# ------------------------------------------------------------------------------------------------ 1: hand-made spectra
def test_amplitude_is_the_scaled_correctly_rounded_root():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(4000) * 10.0 ** rng.uniform(-30, 30, 4000)).astype(F32)
    y = (rng.standard_normal(4000) * 10.0 ** rng.uniform(-30, 30, 4000)).astype(F32)
    got = sr.amp_rn(x, y)
    want = np.hypot(x.astype(np.float64), y.astype(np.float64))
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * want)             # two roundings in front of the root, one behind it
    assert list(sr.amp_rn([3, 0, 0, -5], [4, 0, 2, 12])) == [5, 0, 2, 13]
    assert np.isinf(sr.amp_rn([np.inf], [1.0])[0]) and np.isnan(sr.amp_rn([np.nan], [np.nan])[0])


def test_unit_candidate_returns_the_rows_own_amplitude_misfit():
    slots = [_slot(PYTH, [6.0, 10.0, 12.0], norm=2.0)]
    for method, want in ((3, np.sqrt(2.0 / 32.0)), (4, 2.0 / 32.0)):
        out = sr.evaluate([slots], [0], [1.0], False, [[1.0, 0.0], [0.0, 1.0]], method, "l1norm", DT)
        assert out["slot_misfit"][0, 0, 0] == F32(want)                 # d = 1, 0, -1
        assert out["misfit"][0, 0] == float(F32(want)) / 2.0            # one slot: m / n
        # the second basis row has the amplitude 1 in every bin: d = 5, 9, 11
        want2 = np.sqrt((25.0 + 81.0 + 121.0) / 32.0) if method == 3 else 25.0 / 32.0
        assert out["slot_misfit"][0, 1, 0] == F32(want2)
        assert out["best_index"][0] == 0 and out["best_misfit"][0] == out["misfit"][0, 0] and out["status"][0] == 0
    # a combination, x = (2, -3): the bins (6 - 3, 8), (-12 - 3, 16), (10 - 3, -24) have the amplitudes sqrt(73), sqrt(481), 25
    out = sr.evaluate([slots], [0], [1.0], False, [[2.0, -3.0]], 4, "l1norm", DT)
    b = [F32(np.sqrt(73.0)), F32(np.sqrt(481.0)), F32(25.0)]           # (the scaled squares are exact here: one rounding, the root's)
    d = [float(abs(F32(a) - v)) for a, v in zip([6.0, 10.0, 12.0], b)]
    assert out["slot_misfit"][0, 0, 0] == F32(((d[0] + d[1]) + d[2]) / 32.0)


def test_synthetics_factor_scales_the_synthetic_side():
    slots = [_slot(PYTH, [10.0, 20.0, 26.0])]
    out = sr.evaluate([slots], [0], [1.0], False, [[1.0, 0.0]], 3, "l1norm", DT, syn_factor=2.0)
    assert out["slot_misfit"][0, 0, 0] == 0.0


def test_skipped_bins_and_the_kept_range():
    fw = np.array([0, 0, 1, 0.5, 0, 0], F32)
    ra = np.array([0, 0, 3, 4, 0, 0], F32)
    assert sr.kept_range(fw, ra, True) == (2, 3)
    assert sr.kept_range(fw, ra, False) == (0, 5)
    assert sr.kept_range(np.zeros(6, F32), np.zeros(6, F32), True) == (0, -1)
    ra[5] = 1e-30
    with pytest.raises(ValueError):
        sr.kept_range(fw, ra, True)
    # the filter weight multiplies the synthetic amplitude only (the reference amplitude holds it already): bins 5 x 1, 10 x 0.5
    slots = [_slot(PYTH[:2], [5.0, 5.0], filtw=[1.0, 0.5])]
    out = sr.evaluate([slots], [0], [1.0], False, [[1.0, 0.0]], 4, "l1norm", DT)
    assert out["slot_misfit"][0, 0, 0] == 0.0
    # a slot that keeps no bin has the misfit 0 and still counts with its norm factor
    empty = dict(spectra=np.zeros((0, 2, 2), F32), refamp=np.zeros(0, F32), filtw=np.zeros(0, F32), ntrans=NT, norm=F32(3.0), has_filter=True)
    out = sr.evaluate([[_slot(PYTH, [6.0, 10.0, 12.0], norm=4.0), empty]], [0, 1], [1.0, 1.0], False, [[1.0, 0.0]], 4, "l1norm", DT)
    assert out["slot_misfit"][0, 0, 1] == 0.0 and out["misfit"][0, 0] == (2.0 / 32.0) / 7.0


def test_outer_fold_weights_anarchy_and_receivers_that_do_not_count():
    # receiver 0: two slots (misfits 0.25 and 0.5 under method 3), receiver 1: weight 0, receiver 2: no reference energy
    s00 = _slot(PYTH, [6.0, 10.0, 12.0], norm=2.0)                    # sqrt(2 / 32) = 0.25
    s01 = _slot(PYTH, [7.0, 8.0, 13.0], norm=1.0)                     # sqrt(8 / 32) = 0.5
    s1 = _slot(PYTH, [9.0, 10.0, 13.0], norm=5.0)                     # 16 / 32 -> sqrt = 0.70710677
    s2 = _slot(PYTH, [5.0, 14.0, 13.0], norm=0.0)                     # sqrt(16 / 32)
    slots, rec = [s00, s01, s1, s2], [0, 0, 1, 2]
    m2 = float(F32(np.sqrt(0.5)))
    x = [[1.0, 0.0]]
    for w1 in (0.0, 3.0):
        w = [2.0, w1, 1.0]
        out = sr.evaluate([slots], rec, w, False, x, 3, "l1norm", DT)
        assert list(out["slot_misfit"][0, 0]) == [0.25, 0.5, F32(m2), F32(m2)]
        want = ((0.0 + (0.25 + 0.5) * 2.0) + m2 * w1 + m2 * 1.0) / ((0.0 + 3.0 * 2.0) + 5.0 * w1 + 0.0)
        assert out["misfit"][0, 0] == want
        out = sr.evaluate([slots], rec, w, False, x, 3, "l2norm", DT)
        M0, N0 = np.sqrt(0.25 * 0.25 + 0.5 * 0.5), np.sqrt(4.0 + 1.0)
        M1, N1, M2 = np.sqrt(m2 * m2), np.sqrt(25.0), np.sqrt(m2 * m2)
        want = np.sqrt((((M0 * 2.0) ** 2 + (M1 * w1) ** 2) + (M2 * 1.0) ** 2) / (((N0 * 2.0) ** 2 + (N1 * w1) ** 2) + 0.0))
        assert out["misfit"][0, 0] == want
        # anarchy: rw = w / N; the receiver without reference energy gets the weight 0
        out = sr.evaluate([slots], rec, w, True, x, 3, "l1norm", DT)
        r0, r1 = 2.0 / 3.0, w1 / 5.0
        want = ((0.75 * r0) + m2 * r1 + m2 * 0.0) / ((3.0 * r0) + 5.0 * r1 + 0.0)
        assert out["misfit"][0, 0] == want
    # no receiver counts: NaN, no winner, status 1
    out = sr.evaluate([slots], rec, [0.0, 0.0, 1.0], False, x, 3, "l2norm", DT)
    assert out["status"][0] == 1 and out["best_index"][0] == -1 and np.isnan(out["best_misfit"][0]) and np.isnan(out["misfit"][0, 0])
    # among equal misfits the lowest index wins; a candidate and its opposite are equal (amplitude spectra leave the polarity open)
    out = sr.evaluate([slots], rec, [1.0, 1.0, 1.0], False, [[0.0, 1.0], [1.0, 0.0], [-1.0, 0.0]], 4, "l1norm", DT)
    assert out["misfit"][0, 1] == out["misfit"][0, 2] and out["best_index"][0] == 1


def test_free_scale_recovers_a_planted_scale_exactly():
    rng = np.random.default_rng(11)
    K, nb = 6, 40
    x = rng.uniform(-1.0, 1.0, (3, K))
    xf = x.astype(F32)
    slots, rec = [], [0, 0, 1]
    for m in range(3):
        spec = rng.standard_normal((nb, K, 2)).astype(F32)
        fw = rng.uniform(0.1, 1.0, nb).astype(F32)
        re, im = sr.combine(spec, xf[1:2])
        b = (sr.amp_rn(re, im)[0] * fw).astype(F32)
        slots.append(dict(spectra=spec, refamp=(F32(4.0) * b).astype(F32), filtw=fw, ntrans=NT, norm=F32(1.0 + m), has_filter=True))
    for anarchy in (False, True):
        out = sr.evaluate([slots], rec, [1.5, 0.5], anarchy, x, 3, "l2norm", DT, free_scale=True)
        assert out["scale"][0, 1] == 4.0 and out["misfit"][0, 1] == 0.0 and out["best_index"][0] == 1
        assert np.all(out["misfit"][0, [0, 2]] > 0.0)
    # a direction with no amplitude anywhere has no scale
    out = sr.evaluate([slots], rec, [1.0, 1.0], False, np.zeros((1, K)), 3, "l2norm", DT, free_scale=True)
    assert np.isnan(out["scale"][0, 0]) and np.isnan(out["misfit"][0, 0]) and out["best_index"][0] == -1 and out["status"][0] == 0


# ------------------------------------------------------------------------------------------------ 2: against the oracle
PLANTED_SDR = (40.0, 60.0, 100.0, 5e18)
NCAND = 40
CORNERS = (0.05, 0.1, 0.3, 0.4)                              # of Nyquist


@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("filtered", [False, True])
def test_predicted_slot_misfits_against_the_oracle(method, filtered):
    """Tapered synthetics of the six elementary tensors from oracle/libko.so, transformed in numpy; 40 random double couples
    through the restatement; every slot misfit against the oracle's own evaluation of the combined `moment_tensor` source.

    Bound per slot: MISFIT_RTOL max(m, n) + FFT_ROUNDOFF_C fft_roundoff_bound(c = 1), where the synthetic's norm is replaced by
    sum_a |x_a| n2(s_a) and log2 N by log2 N + K + 1: each of the K spectra carries its own transform error and the combination
    adds K + 1 roundings; the bound scales with the basis rows, not with the possibly cancelling sum."""
    name = {3: "ampspec_l2norm", 4: "ampspec_l1norm"}[method]
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    sc.apply_setup(e, True)
    dt, K = sc.gf["dt"], 6
    fx = [c * 0.5 / dt for c in CORNERS]
    if filtered:
        for ir in range(1, sc.nrec + 1):
            e.set_filter(ir, fx, [0., 1., 1., 0.])
    e.set_misfit_method(method)
    syn, ref, receivers = oracle_traces(e, sc.comps, 6, basis_rows("moment_tensor", mt_row(np.zeros(6))), K)
    slot_receiver = [r for r, sl in enumerate(receivers) for _ in sl]
    # reference side and transform lengths as the oracle has them
    e.set_source_params(6, mt_row(planted))
    m0, n0, _ = e.get_misfits()
    nt = slot_scales(e, sc.comps, dt)[0]
    slots, nkept, nbins = [], 0, 0
    j = 0
    for ir, cs in enumerate(sc.comps):
        for k in range(len(cs)):
            ntr, nb = int(nt[j]), int(nt[j]) // 2 + 1
            refamp = e.amp_spectrum(ir + 1, k + 1, False, filtered)[1]
            assert len(refamp) == nb
            fw = sr.filter_weights(fx, [0., 1., 1., 0.], nb, sr.df_of(ntr, dt)) if filtered else np.ones(nb, F32)
            klo, khi = sr.kept_range(fw, refamp, filtered)         # (raises where a skipped bin has reference amplitude)
            nkept += khi - klo + 1
            nbins += nb
            spec = sr.spectra_of(syn[j][0], ntr)
            slots.append(dict(spectra=spec[klo:khi + 1], refamp=refamp[klo:khi + 1], filtw=fw[klo:khi + 1], ntrans=ntr, norm=n0[j],
                              has_filter=filtered))
            j += 1
    n2_basis = np.array([[np.sqrt(dt * np.sum(syn[j][0, a].astype(np.float64) ** 2)) for a in range(K)] for j in range(len(slots))])
    rng = np.random.default_rng(77)
    sdr = np.stack([rng.uniform(0., 360., NCAND), rng.uniform(0., 90., NCAND), rng.uniform(-180., 180., NCAND)], 1)
    sdr[0] = PLANTED_SDR[:3]
    tensors = np.array([synthetic.mt_from_sdr(s, d, r, PLANTED_SDR[3]) for s, d, r in sdr]).astype(np.float32)
    cand = tensors.astype(np.float64) / UNIT
    out = sr.evaluate([slots], slot_receiver, np.ones(sc.nrec), False, cand, method, "l2norm", dt)
    worst, worst_cancel = -np.inf, 0.0
    for c in range(NCAND):
        e.set_source_params(6, mt_row(tensors[c]))
        m, n, g = e.get_misfits()
        ntc, wl, na, nb2 = slot_scales(e, sc.comps, dt)
        assert np.array_equal(ntc, nt)
        n2x = n2_basis @ np.abs(cand[c])
        worst_cancel = max(worst_cancel, float(np.max(n2x / np.maximum(nb2, 1e-300))))
        b1 = fft_roundoff_bound(name, dt, nt * 2.0 ** (K + 1), wl, na, n2x, c=1.0)
        scale = np.maximum(np.abs(n.astype(np.float64)), np.abs(m.astype(np.float64)))
        excess = np.abs(out["slot_misfit"][0, c].astype(np.float64) - m) - MISFIT_RTOL * scale
        worst = max(worst, float(np.max(excess / b1)))
        assert np.all(excess <= FFT_ROUNDOFF_C * b1), (c, np.max(excess / b1))
        # the global misfit of the fold is the oracle's
        assert abs(out["misfit"][0, c] - g) <= 4 * MISFIT_RTOL * np.sqrt(g * g + 1.0) + FFT_ROUNDOFF_C * np.max(b1 / np.maximum(scale, 1e-300))
    e.close()
    print("%s, filter %s: %d of %d bins kept, largest excess over bound(c = 1) %.3g (limit %.2f), sum |x_a| n2(s_a) up to %.0f x the "
          "norm of the combined trace" % (name, filtered, nkept, nbins, max(worst, 0.0), FFT_ROUNDOFF_C, worst_cancel))
    assert out["best_index"][0] == 0 or out["misfit"][0, out["best_index"][0]] <= out["misfit"][0, 0]


# ------------------------------------------------------------------------------------------------ 3: plumbing
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
    assert len(L.kiwi_hip_spectral_candidates.argtypes) == 21
    assert len(L.kiwi_hip_spectral_candidates_params.argtypes) == 23
    assert L.kiwi_hip_get_spectral_candidates_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_spectral_candidates_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_shape_answers_without_a_device_and_a_stage_fits_the_lds():
    L = klib.load()
    kmax = L.kiwi_hip_linear_fit_max_basis()
    shapes = set()
    for K in range(1, kmax + 1):
        c, b, n = C.c_int(), C.c_int(), C.c_int(-1)
        assert L.kiwi_hip_spectral_candidates_shape(None, K, C.byref(c), C.byref(b), C.byref(n)) == 0
        assert c.value >= 64 and c.value % 64 == 0 and b.value >= 1 and n.value == 0
        # a stage: K complex spectra, a reference amplitude and a filter weight per bin, next to the tile's bests; the spectra
        # kernel may hold a transform of 32768 samples (128 KiB) in the 160 KiB of a workgroup
        assert b.value * (8 * K + 8) + (c.value // 64) * 12 <= 64 * 1024
        shapes.add((c.value, b.value))
    assert len(shapes) == 1
    c, b = C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_spectral_candidates_shape(None, K, C.byref(c), C.byref(b), None) != 0
    assert L.kiwi_hip_spectral_candidates_shape(None, 6, None, C.byref(b), None) != 0
    assert L.kiwi_hip_spectral_candidates_shape(None, 6, C.byref(c), None, None) != 0
    assert L.kiwi_hip_spectral_candidates_shape(None, 6, C.byref(c), C.byref(b), None) == 0
