"""kiwi_hip_linear_fit_time_scan without a device: the entry points exist in the library, the symbol map, the header, the ctypes
table and the Fortran binding; the limits and the kernel's shape answer; the yardstick of the GPU tests on the CPU oracle -- the fit
of basis sources moved by k samples (route A) gives the bits of the fit with references and tapers moved by -k samples (route
B) --; and a planted tensor at a planted offset through tests/linfit_timescan_restatement.py."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import lib as klib, synthetic
from tests import linfit_restatement as lr
from tests import linfit_timescan_restatement as ltr
from tests.common import Scenario
from tests.linfit_cases import PLANTED, UNIT, basis_rows, mt_row, oracle_traces, receivers_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_linear_fit_time_scan", "kiwi_hip_linear_fit_time_scan_params", "kiwi_hip_get_linear_fit_time_scan_ms",
           "kiwi_hip_linear_fit_time_scan_shape"]
COMPS = ["d", "ne", "ned", "ned", "ne", "d"]
WINDOW = 150
KS = (-7, 3, 8)
# (a `moment_tensor` row's own rise-time parameter is discretised into centroids, never folded: 0.5 s gives two centroids at
# t0 -+ 0.125 s, dyadic like t0 itself, so every centroid's time / dt is exact in fp32, and so is every time + k dt)
LOCATION = [1.25, 500., -800., 10000.]


def test_symbols_are_exported_mapped_declared_in_the_ctypes_table_and_bound_in_fortran():
    L = klib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", klib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in dyn.splitlines() if line.strip())
    text = open(os.path.join(ROOT, "kiwi_amd", "csrc", "kiwi_hip.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    globs = re.search(r"global:(.*?);\s*local:", text, re.S).group(1).replace(";", " ").split()
    declared = klib.declared_symbols()
    binding = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for s in SYMBOLS:
        assert s in exported, s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        assert s in declared, s
        f = getattr(L, s)
        assert f.restype is C.c_int and f.argtypes is not None, s
        assert "name='%s'" % s in binding, s
    assert len(L.kiwi_hip_linear_fit_time_scan.argtypes) == 15 and len(L.kiwi_hip_linear_fit_time_scan_params.argtypes) == 17
    assert L.kiwi_hip_get_linear_fit_time_scan_ms.argtypes == [C.c_void_p, klib.c_float_p]
    assert "kiwi_hip_linear_fit_time_scan_shape" in open(os.path.join(ROOT, "kiwi_amd", "fortran", "binding_smoke.f90")).read()


def test_limits_and_shape_answer_without_a_device():
    L = klib.load()
    assert L.kiwi_hip_time_scan_max_shift() == 1024 and L.kiwi_hip_time_scan_max_offsets() == 256
    kmax = L.kiwi_hip_linear_fit_max_basis()
    tiles = set()
    for K in range(1, kmax + 1):
        j, t = C.c_int(), C.c_int()
        assert L.kiwi_hip_linear_fit_time_scan_shape(K, C.byref(j), C.byref(t)) == 0
        nn = K * (K + 1) // 2 + K + 1
        assert 1 <= j.value <= 256 and 2 * (j.value * (nn - 1) + 1) <= 256       # the accumulators of a thread are registers
        assert t.value >= 256 and t.value % 256 == 0                              # a thread's samples do not depend on the tiling
        tiles.add(t.value)
    assert len(tiles) == 1
    j, t = C.c_int(), C.c_int()
    for K in (0, kmax + 1):
        assert L.kiwi_hip_linear_fit_time_scan_shape(K, C.byref(j), C.byref(t)) != 0


# ---------------------------------------------------------------------------------------------- the yardstick, on the oracle
def _scenario(true_time):
    sc = Scenario(comps_list=COMPS, true_type=6, true_params=mt_row(PLANTED, location=[true_time] + LOCATION[1:], risetime=0.5))
    e = sc.oracle()
    sc.make_references(e)
    e.close()
    dt = sc.gf["dt"]
    for ir in range(1, sc.nrec + 1):
        sc.tapers[ir] = synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, WINDOW, dt, 10.0)
    return sc


def _fresh(sc, ref_shift=0, taper_shift=0.0):
    """an oracle engine with the references moved by ref_shift samples and the tapers by taper_shift seconds"""
    e = sc.oracle()
    sc.apply_setup(e, True)
    if ref_shift:
        for ir in range(1, sc.nrec + 1):
            e.shift_ref_seismogram(ir, ref_shift)
    if taper_shift:
        for ir, (x, y) in sc.tapers.items():
            e.set_taper(ir, np.asarray(x, np.float32) + np.float32(taper_shift), y)
    return e


def _basis(seconds=0.0):
    rows = basis_rows("moment_tensor", mt_row(np.zeros(6), location=LOCATION, risetime=0.5))
    rows[:, 0] += np.float32(seconds)
    return rows


def test_route_a_equals_route_b_on_the_oracle():
    sc = _scenario(LOCATION[0] + 2 * 0.5)
    dt = sc.gf["dt"]
    assert dt == 0.5
    fits = []
    for k in (0,) + KS:
        e = _fresh(sc)
        syn_a, ref_a, receivers = oracle_traces(e, sc.comps, 6, _basis(k * dt), 6)                 # route A: the basis k dt later
        e.close()
        a = lr.fit(syn_a, ref_a, receivers, dt)
        if k:
            e = _fresh(sc, ref_shift=-k, taper_shift=-k * dt)
            syn_b, ref_b, _ = oracle_traces(e, sc.comps, 6, _basis(), 6)                          # route B: references and tapers k dt earlier
            e.close()
            for x, y in zip(syn_a + ref_a, syn_b + ref_b):
                assert np.array_equal(x, y), k
            b = lr.fit(syn_b, ref_b, receivers, dt)
            for name in a:
                assert np.array_equal(a[name], b[name], equal_nan=True), (k, name)
        assert a["status"][0] == 0 and len(ref_a) == 12 and len(ref_a[0]) == WINDOW
        fits.append(a)
    assert all(np.any(f["coef"] != fits[0]["coef"]) for f in fits[1:]), "the offsets change the coefficients"


def _raw_rows(sc, rows, S):
    """(raw[slot] [1, K, wlen + 2 S], taper[slot] [wlen], ref[slot] [wlen], tapered oracle traces syn[slot] [1, K, wlen]) of the basis
    `rows` on the oracle: the untapered synthetics (ko.Engine.synthetic(..., 1)) laid over the windows made S samples wider, and the
    taper weights read as the tapered reference of an engine whose references are ones"""
    e = _fresh(sc)
    syn, ref, _ = oracle_traces(e, sc.comps, 6, rows, len(rows))
    slots = [(ir + 1, k + 1) for ir, c in enumerate(sc.comps) for k in range(len(c))]
    w0 = [e.reference(ir, k, 2)[0] for ir, k in slots]
    raw = [np.zeros((1, len(rows), len(r) + 2 * S), np.float32) for r in ref]
    for i, p in enumerate(rows):
        e.set_source_params(6, p)
        e.get_misfits()
        for m, (ir, k) in enumerate(slots):
            lo, d = e.synthetic(ir, k, 1)
            for x in range(raw[m].shape[2]):
                t = w0[m] - S + x - lo
                if 0 <= t < len(d):
                    raw[m][0, i, x] = d[t]
    e.close()
    ones = sc.oracle()
    for m, (ir, k) in enumerate(slots):
        ones.set_reference(ir, k, w0[m] - 50, np.ones(len(ref[m]) + 100, np.float32))
    for ir, (x, y) in sc.tapers.items():
        ones.set_taper(ir, x, y)
    ones.set_source_params(6, rows[0])
    ones.get_misfits()
    taper = []
    for m, (ir, k) in enumerate(slots):
        lo, w = ones.reference(ir, k, 2)
        assert lo == w0[m] and len(w) == len(ref[m])
        taper.append(w)
    ones.close()
    return raw, taper, ref, syn


def test_planted_tensor_at_a_planted_offset_through_the_restatement():
    dt, S = 0.5, 4
    sc = _scenario(LOCATION[0] + 2 * dt)                      # the references: the planted tensor two samples later than the basis
    raw, taper, ref, syn = _raw_rows(sc, _basis(), S)
    receivers = receivers_of(sc.comps)
    # offset 0 of the restatement is the oracle's own tapered trace, bit for bit
    for a, b in zip(ltr.shifted_traces(raw, taper, S, 0), syn):
        assert np.array_equal(a, b)
    out = ltr.fit(raw, taper, ref, receivers, dt, S, -3, 1, 8)
    assert out["coef"].shape == (1, 8, 6) and out["misfit"].shape == out["status"].shape == out["pivot_min"].shape == (1, 8)
    assert np.all(out["status"] == 0) and out["best"][0] == 5                         # offsets -3 .. 4: +2 is index 5
    tensor = out["coef"][0, 5] * UNIT
    rel = np.abs(tensor - PLANTED.astype(np.float64)) / np.abs(PLANTED.astype(np.float64))
    print("planted tensor at offset +2: relative error", rel, "misfits over the offsets", out["misfit"][0])
    assert np.all(rel <= 1e-5) and out["misfit"][0, 5] <= 1e-5
    assert np.all(np.delete(out["misfit"][0], 5) > 100 * out["misfit"][0, 5])
    # offset 0 of the restatement is linfit_restatement on the oracle's traces
    plain = lr.fit(syn, ref, receivers, dt)
    for name in ("coef", "misfit", "status", "pivot_min", "normal"):
        assert np.array_equal(out[name][:, 3], plain[name], equal_nan=True), name
    # first minimum: the lowest index among equal values, only solved offsets, -1 where there is none
    m = np.array([[3.0, 1.0, 1.0, 0.5], [2.0, 2.0, 2.0, 2.0], [np.nan, np.nan, np.nan, np.nan]])
    st = np.array([[0, 0, 0, 1], [1, 0, 0, 0], [1, 2, 1, 1]])
    assert list(ltr.first_minimum(m, st)) == [1, 1, -1]
