"""Misfit bands without a device: the entry points exist in the library, the symbol map, the ctypes table and the header;
kiwi_hip_misfit_bands_max answers; the host helper that folds band misfits into one outer misfit per source."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

from kiwi_amd import gridsearch, lib as klib
from kiwi_amd.engine import make_global_misfits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kiwi_hip_misfit_bands_max", "kiwi_hip_set_misfit_bands", "kiwi_hip_get_misfit_bands", "kiwi_hip_band_misfits",
           "kiwi_hip_band_misfits_for_params", "kiwi_hip_get_band_misfits_ms"]


def test_bands_max_answers_without_a_device():
    L = klib.load()
    assert L.kiwi_hip_misfit_bands_max() == 16


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
    assert L.kiwi_hip_band_misfits.argtypes == [C.c_void_p, C.c_int, C.c_int, klib.c_float_p, klib.c_float_p, klib.c_float_p]
    assert len(L.kiwi_hip_band_misfits_for_params.argtypes) == 9 and len(L.kiwi_hip_set_misfit_bands.argtypes) == 6


def test_one_band_of_unit_weight_is_make_global_misfits():
    rng = np.random.default_rng(3)
    m = rng.uniform(0.1, 2.0, (4, 1, 3, 2))
    n = rng.uniform(1.0, 3.0, (4, 1, 3, 2))
    m[:, :, 1, 1] = 0.0
    n[:, :, 1, 1] = 0.0                                       # a receiver of one component
    w = np.array([1.0, 0.5, 2.0])
    for outer in ("l1norm", "l2norm"):
        for anarchy in (False, True):
            g, by_rec = gridsearch.make_band_global_misfits(m, n, None, outer, w, anarchy)
            g0, by_rec0 = make_global_misfits(m[:, 0], n[:, 0], outer, w, anarchy=anarchy)
            assert np.array_equal(g, g0) and np.array_equal(by_rec, by_rec0)


def test_two_bands_by_hand():
    # one source, two receivers; receiver 1 has two components, receiver 2 one
    m = np.zeros((1, 2, 2, 2))
    n = np.zeros((1, 2, 2, 2))
    m[0, 0] = [[3.0, 4.0], [1.0, 0.0]]
    n[0, 0] = [[6.0, 8.0], [2.0, 0.0]]
    m[0, 1] = [[1.0, 2.0], [2.0, 0.0]]
    n[0, 1] = [[2.0, 2.0], [4.0, 0.0]]
    bw = np.array([1.0, 0.5])
    # l2norm: per receiver the root of the sum of squares over (band, component) of weight x value, then over the receivers
    m1 = np.sqrt(3.0 ** 2 + 4.0 ** 2 + 0.5 ** 2 + 1.0 ** 2)
    m2 = np.sqrt(1.0 ** 2 + 1.0 ** 2)
    n1 = np.sqrt(6.0 ** 2 + 8.0 ** 2 + 1.0 ** 2 + 1.0 ** 2)
    n2 = np.sqrt(2.0 ** 2 + 2.0 ** 2)
    g, by_rec = gridsearch.make_band_global_misfits(m, n, bw, "l2norm")
    assert np.allclose(by_rec[0], [m1, m2], rtol=1e-15)
    assert np.isclose(g[0], np.sqrt((m1 ** 2 + m2 ** 2) / (n1 ** 2 + n2 ** 2)), rtol=1e-15)
    # l1norm: plain sums
    g, by_rec = gridsearch.make_band_global_misfits(m, n, bw, "l1norm")
    assert np.allclose(by_rec[0], [3.0 + 4.0 + 0.5 + 1.0, 1.0 + 1.0], rtol=1e-15)
    assert np.isclose(g[0], (8.5 + 2.0) / (6.0 + 8.0 + 1.0 + 1.0 + 2.0 + 2.0), rtol=1e-15)


def test_band_slots_to_receivers_layout():
    comps = ["d", "ne", "ned"]
    m = np.arange(2 * 2 * 4, dtype=np.float32).reshape(2, 2, 4)          # receiver 2 disabled: slots d | n e d
    mis, nor = gridsearch.band_slots_to_receivers(m, m + 100, comps, enabled=[True, False, True])
    assert mis.shape == (2, 2, 3, 3)
    assert np.array_equal(mis[1, 1, 0], [12.0, 0, 0]) and np.all(mis[:, :, 1] == 0) and np.array_equal(mis[1, 1, 2], [13.0, 14.0, 15.0])
    assert np.array_equal(nor[0, 0, 2], [101.0, 102.0, 103.0])
