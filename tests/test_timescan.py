"""The time scan without a device: the entry points exist in the library, the symbol map, the ctypes table and the header; the
two limits answer; split_time_axis; and the yardstick of the GPU tests itself, on the CPU oracle -- a source moved by k samples
(route A) gives the bits of the references and tapers moved by -k samples (route B) for the unfiltered time-domain methods."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import gridsearch, lib as klib, synthetic
from kiwi_amd.engine import NORMS
from oracle import ko
from tests.common import Scenario
from tests.timescan_cases import TIME_DOMAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_time_scan_max_shift", "kiwi_hip_time_scan_max_offsets", "kiwi_hip_time_scan", "kiwi_hip_time_scan_for_params",
           "kiwi_hip_get_time_scan_ms"]


def test_limits_answer_without_a_device():
    L = klib.load()
    assert L.kiwi_hip_time_scan_max_shift() == 1024
    assert L.kiwi_hip_time_scan_max_offsets() == 256


def test_symbols_are_exported_mapped_declared_and_in_the_ctypes_table():
    L = klib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", klib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in dyn.splitlines() if line.strip())
    text = open(os.path.join(ROOT, "kiwi_amd", "csrc", "kiwi_hip.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    globs = re.search(r"global:(.*?);\s*local:", text, re.S).group(1).replace(";", " ").split()
    declared = klib.declared_symbols()
    for s in SYMBOLS:
        assert s in exported, s
        assert any(fnmatch.fnmatchcase(s, g) for g in globs), (s, globs)
        assert s in declared, s
        f = getattr(L, s)
        assert f.restype is C.c_int and f.argtypes is not None, s
    assert L.kiwi_hip_time_scan.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, klib.c_float_p, klib.c_float_p,
                                             klib.c_float_p, klib.c_int_p]
    assert len(L.kiwi_hip_time_scan_for_params.argtypes) == 13 and len(L.kiwi_hip_get_time_scan_ms.argtypes) == 2
    assert len(L.kiwi_hip_time_scan_max_shift.argtypes) == 0 and len(L.kiwi_hip_time_scan_max_offsets.argtypes) == 0


def test_split_time_axis():
    f = gridsearch.split_time_axis
    assert f([0.0, 0.5, 1.0, 1.5], 0.5) == (0, 1, 4)
    assert f([-3.25, -1.75, -0.25, 1.25], 0.5) == (0, 3, 4)                 # a negative start off the sample grid, a step of three samples
    assert f(np.arange(21) * 2.0 - 20.0, 0.5) == (0, 4, 21)
    assert f([1.25], 0.5) == (0, 1, 1)
    assert f([7.0], 0.1) == (0, 1, 1)
    one_ulp = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert f([0.0, 0.5, one_ulp], 0.5) is None                              # off by one fp32 ulp
    assert f([0.0, 0.5, np.nextafter(np.float32(1.0), np.float32(0.0))], 0.5) is None
    assert f([0.0, 0.5, 1.5], 0.5) is None                                  # whole samples, uneven steps
    assert f([1.0, 0.5, 0.0], 0.5) is None                                  # descending
    assert f([0.0, 0.0], 0.5) is None
    assert f([0.0, 0.25, 0.5], 0.5) is None                                 # half a sample
    assert f([], 0.5) is None


# ---------------------------------------------------------------------------------------------- the yardstick, on the oracle
COMPS = ["d", "ne", "ned", "ned", "ne", "d"]
WINDOW = 150
KS = (-7, 3, 8)


def _scenario():
    sc = Scenario(comps_list=COMPS)
    e = sc.oracle()
    sc.make_references(e)
    e.close()
    dt = sc.gf["dt"]
    for ir in range(1, sc.nrec + 1):
        sc.tapers[ir] = synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, WINDOW, dt, 10.0)
    return sc


def _fresh(sc, method, ref_shift=0, taper_shift=0.0):
    """a fresh oracle engine (a probe's span keeps history): references moved by ref_shift samples, tapers by taper_shift s"""
    e = sc.oracle()
    sc.apply_setup(e, True)
    e.switch_receiver(6, False)
    e.set_misfit_method(NORMS[method])
    if ref_shift:
        for ir in range(1, sc.nrec + 1):
            e.shift_ref_seismogram(ir, ref_shift)
    if taper_shift:
        for ir, (x, y) in sc.tapers.items():
            e.set_taper(ir, np.asarray(x, np.float32) + np.float32(taper_shift), y)
    return e


def _sources():
    # (a `moment_tensor` row's own rise-time parameter is discretised into centroids, never folded: 0.5 s gives two centroids at
    # t0 -+ 0.125 s, dyadic like t0 itself, so every centroid's time / dt is exact in fp32; 0 would be a source without moment)
    mt = np.array([1.25, 500., -800., 10000., 4.1e18, -2.3e18, 7.7e18, 3.5e18, -2.9e18, 5.2e18, 0.5], np.float32)
    cent, _, rise, _ = ko.discretize(6, mt, 0.5)
    assert rise == 0.0 and np.all(cent[:, 3] * 8 == np.rint(cent[:, 3] * 8)) and np.any(cent[:, 4:] != 0)
    rng = np.random.default_rng(5)
    tab = np.zeros((4, 10), np.float32)
    tab[:, 0:2] = rng.uniform(-3000., 3000., (4, 2))
    tab[:, 2] = rng.uniform(8000., 12000., 4)
    tab[:, 3] = np.array([-1.375, 0.25, 0.625, 2.0], np.float32)          # dyadic: time / dt is exact in fp32
    tab[:, 4:10] = rng.standard_normal((4, 6)) * 1e18
    return mt, tab


def _evaluate(e, kind, src, seconds):
    if kind == "moment_tensor":
        p = src.copy()
        p[0] += np.float32(seconds)
        e.set_source_params(6, p)
    else:
        t = src.copy()
        t[:, 3] += np.float32(seconds)
        e.set_centroids(t, 1.0, 2.0)                                        # rise time 2 s: five taps
    m, n, g = e.get_misfits()
    e.close()
    return m.copy(), n.copy(), np.float32(g)


@pytest.mark.parametrize("kind", ["moment_tensor", "centroid_table"])
def test_route_a_equals_route_b_on_the_oracle(kind):
    sc = _scenario()
    dt = sc.gf["dt"]
    mt, tab = _sources()
    src = mt if kind == "moment_tensor" else tab
    for method in TIME_DOMAIN:
        m0, n0, g0 = _evaluate(_fresh(sc, method), kind, src, 0.0)
        assert np.all(np.isfinite(m0)) and np.all(m0 != 0) and len(m0) == 11
        moved = 0
        for k in KS:
            a = _evaluate(_fresh(sc, method), kind, src, k * dt)                                  # route A: the source k dt later
            b = _evaluate(_fresh(sc, method, ref_shift=-k, taper_shift=-k * dt), kind, src, 0.0)  # route B: references and tapers k dt earlier
            for x, y, what in zip(a, b, ("misfit", "norm", "global")):
                assert np.array_equal(x, y), (kind, method, k, what, x, y)
            moved += int(not np.array_equal(a[0], m0))
        assert moved == len(KS), "the offsets change the misfits"
