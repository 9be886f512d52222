"""The kernels of `Engine.linear_fit`'s path executed on the HOST from their own source text (tests/host_kernels: a
<hip/hip_runtime.h> for a plain C++ compiler, an executor that runs a workgroup's lanes as threads, and the stand-alone program
linfit_path_host.cpp with every device buffer a heap allocation of exactly the library's size) under AddressSanitizer + UBSan:
geometry_kernel, cellgroup_kernel, misfit_kernel with the kept traces, global_kernel, linfit_gram_kernel, linfit_solve_kernel,
and between them an audit of every global address accumulate_grouped_kernel forms from the tables the first two wrote (that
kernel's own text, kiwi_accum.inc, is assembly-bound and is not executed anywhere but on the device).

Why: the device half of the randomised sweep (tests/family_fuzz.py) ended in "an illegal memory access was encountered" at one
set-up (family_fuzz.recorded_fault_case) and nothing on that path is run on the device at new set-ups until the cause is found
without one.  What the run here means is fixed first: on the default scenario the host-run kernels give the oracle's geometry
records, the restatement's bits and the oracle's misfits, and the same program with one buffer an element short ends in a
sanitizer report.  Then the recorded set-up and the sweep's layouts.

What it found (CHANGELOG): misfit_kernel read the sample in FRONT of a synthetic's slot -- for the first slot of the first source in
front of the allocation -- whenever a rise time rounded to a fold of one tap (cases 4, 6 and 16 of the linear_fit_candidates slice:
`mt_eikonal`, rise time 0.4); fixed in kiwi_misfit.hpp folded_scaled_sample, the three cases are the regression.  The recorded
set-up itself runs clean through every kernel here and through the audit.

The program is built and run as tests/test_host_sanitizers.py runs its own; it is never loaded into Python."""
import copy

import numpy as np
import pytest

from oracle import ko
from tests import family_fuzz as ff
from tests import host_kernel_cases as hk
from tests import linfit_restatement as lr
from tests.common import Scenario, misfit_close
from tests.linfit_cases import PLANTED, mt_row, receivers_of

COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # tests/test_linfit_gpu.py: receivers of 1 to 5 components
ENABLED = [True] * 5 + [False]
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
K = 6
SHORT = ("recs", "reft", "tw", "nbr")      # buffers of the geometry, misfit, Gram and solve kernels whose last element is in use at this set-up
SLICES = [(f, s, i) for f in ("linear_fit", "linear_fit_candidates") for s, i in ff.slice_of(f)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return hk.build(tmp_path_factory.mktemp("host_kernels"))


def scattered_groups(rng, ngroup, K):
    """tests/test_linfit_gpu.py scattered_groups: basis sources that share nothing"""
    n = ngroup * K
    rows = np.zeros((n, 11), np.float32)
    rows[:, 0] = rng.uniform(-10., 10., n)
    rows[:, 1:3] = rng.uniform(-3000., 3000., (n, 2))
    rows[:, 3] = rng.uniform(8000., 12000., n)
    rows[:, 4:10] = rng.standard_normal((n, 6)) * 1e18
    rows[:, 10] = 1.0
    return rows


def default_set_up(ngroup, seed):
    """the default Scenario() as tests/test_linfit_gpu.py build(COMPS) sets it up: (scenario, oracle engine, rows)"""
    sc = Scenario(comps_list=COMPS, true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    sc.apply_setup(e, True)
    return sc, e, scattered_groups(np.random.default_rng(seed), ngroup, K)


@pytest.fixture(scope="module")
def default_case(exe, tmp_path_factory):
    """the default scenario's case file, the program's results on it, and the oracle's side: computed once, read by the tests"""
    where = tmp_path_factory.mktemp("default_case")
    sc, e, rows = default_set_up(2, 5)
    a = hk.case_arrays(sc, e, rows, K, lambda eng, row: eng.set_source_params(6, row), enabled=ENABLED, weights=WEIGHTS, anarchy=True)
    hk.write_arrays(where / "case.bin", a)
    r = hk.run(exe, where / "case.bin", where / "out.bin")
    assert hk.is_clean(r), (r.stdout + r.stderr)[-4000:]
    from kiwi_amd.engine import GEOREC
    res = hk.read_arrays(where / "out.bin")
    geo, mis = [], []
    for s, row in enumerate(rows):
        e.set_source_params(6, row)
        mis.append(e.get_misfits())
        geo.append([e.centroid_geometry(ir + 1, int(res["cent_ofs"][s + 1] - res["cent_ofs"][s]), GEOREC) for ir in range(sc.nrec)])
    e.close()
    sc.odb.close()
    return dict(sc=sc, rows=rows, path=where / "case.bin", res=res, geo=geo, mis=mis, stdout=r.stdout)


# ------------------------------------------------------------------------------------------------ what a clean run means
def test_host_run_geometry_kernel_gives_the_oracles_records(default_case):
    """the comparison of tests/test_gpu_parity.py test_geometry_records_match_oracle: integer fields identical, float fields within
    1e-5 and different in at most 0.2 % of their bits' places (here the host's libm is the oracle's: none differ)"""
    from kiwi_amd.engine import GEOREC
    res, sc = default_case["res"], default_case["sc"]
    recs = res["recs"].view(GEOREC)
    ofs = res["cent_ofs"]
    nf = nbad = 0
    for s in range(len(default_case["rows"])):
        nc = ofs[s + 1] - ofs[s]
        assert nc >= 2
        for ir in range(sc.nrec):
            g = recs[ofs[s] * sc.nrec + ir * nc:ofs[s] * sc.nrec + (ir + 1) * nc]
            o = default_case["geo"][s][ir][:nc]
            for name in ("row", "ishift"):
                assert np.array_equal(g[name], o[name]), (s, ir, name)
            assert np.array_equal(g["flags"] & 3, o["flags"]), (s, ir)
            for name in ("w", "wfrac", "f", "cl", "sl"):
                d = g[name].view(np.int32).astype(np.int64) - o[name].view(np.int32).astype(np.int64)
                nf += d.size
                nbad += np.count_nonzero(d)
                assert np.allclose(g[name], o[name], rtol=1e-5, atol=1e-12), (s, ir, name)
    print("geometry records: %d of %d float fields differ from the oracle's" % (nbad, nf))
    assert nf > 1000 and nbad <= 0.002 * nf, (nbad, nf)


def test_host_run_gram_and_solve_kernels_give_the_restatements_bits(default_case):
    res, sc, nsrc = default_case["res"], default_case["sc"], len(default_case["rows"])
    syn, ref = hk.traces_of(res, nsrc, K)
    fit = lr.fit(syn, ref, receivers_of(COMPS, ENABLED), sc.gf["dt"], WEIGHTS, True)
    for name, mine in (("by_receiver", res["by_receiver"]), ("normal", res["normal"]), ("coef", res["coef"]), ("misfit", res["fit_misfit"]),
                       ("status", res["status"]), ("pivot_min", res["pivot_min"])):
        assert np.array_equal(mine.reshape(fit[name].shape), fit[name], equal_nan=mine.dtype != np.int32), name
    assert np.all(res["status"] == 0) and np.all(res["by_receiver"].reshape(nsrc // K, sc.nrec, -1)[:, 5] == 0.0)


def test_host_run_misfit_kernel_gives_the_oracles_misfits(default_case):
    res, nsrc = default_case["res"], len(default_case["rows"])
    nmis = int(res["layout"][7])
    mine = res["misfit"].reshape(nsrc, nmis)
    for s, (m, n, g) in enumerate(default_case["mis"]):
        assert np.array_equal(res["norm"], n[:nmis])                                 # (the oracle has every receiver enabled: the sixth's slots follow)
        assert misfit_close(mine[s], m[:nmis], norm=n[:nmis]), s
        mo, no = np.asarray(m[:nmis], np.float64), np.asarray(n[:nmis], np.float64)
        assert misfit_close(res["global"][s], np.sqrt(np.sum(mo * mo)) / np.sqrt(np.sum(no * no)), glob=True), s


@pytest.mark.parametrize("short", SHORT)
def test_the_detector_detects(exe, default_case, tmp_path, short):
    """the same program on the same case with ONE of its own buffers an element short: a sanitizer report, not a clean run"""
    r = hk.run(exe, default_case["path"], tmp_path / "out.bin", short=short)
    assert r.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in r.stderr and "run: clean" not in r.stdout, (short, r.returncode, (r.stdout + r.stderr)[-2000:])


# ------------------------------------------------------------------------------------------------ the sweep's set-ups
def eikonal_tables(case):
    cent, ofs, moment, rise = [], [0], [], []
    for row in case.rows:
        c, m, r, _ = ko.discretize_eikonal(5, np.asarray(row, np.float32), case.sc.effective_dt, case.oprof, case.cp, case.cn)
        cent.append(np.asarray(c, np.float32).reshape(-1, 10))
        ofs.append(ofs[-1] + len(cent[-1]))
        moment.append(m)
        rise.append(r)
    return np.concatenate(cent), ofs, moment, rise


def first_receiver_only(case):
    """the case with its first enabled receiver alone: nrec = 1 puts every per-receiver table at the end of its allocation"""
    ir = case.enabled.index(True)
    c = copy.copy(case)
    sc = copy.copy(case.sc)
    sc.nrec, sc.lat, sc.lon, sc.depth, sc.comps = 1, case.sc.lat[ir:ir + 1], case.sc.lon[ir:ir + 1], case.sc.depth[ir:ir + 1], case.sc.comps[ir:ir + 1]
    sc.refs = {(1, k): v for (r, k), v in case.sc.refs.items() if r == ir + 1}
    sc.tapers = {1: case.sc.tapers[ir + 1]}
    c.sc, c.enabled, c.weights = sc, [True], np.asarray(case.weights)[ir:ir + 1]
    return c


def run_case(exe, case, where, expect_window=None):
    """(CompletedProcess, results or None).  A misfit filter is left out: the transforms behind it are not this program's"""
    c = copy.copy(case)
    c.filter = None
    e = c.oracle()
    e.set_synthetics_factor(1.0)
    try:
        a = hk.case_arrays(c.sc, e, c.rows, ff.K, c.set_source, sourcetype=c.sourcetype, tables=eikonal_tables(c) if c.sourcetype == "mt_eikonal" else None,
                           enabled=c.enabled, weights=c.weights, anarchy=c.anarchy, factor=c.factor, undersampling=c.undersampling, expect_window=expect_window)
    finally:
        e.close()
        c.sc.odb.close()
    hk.write_arrays(where / "case.bin", a)
    r = hk.run(exe, where / "case.bin", where / "out.bin")
    return r, (hk.read_arrays(where / "out.bin") if r.returncode == 0 else None)


def test_the_recorded_set_up_runs_clean(exe, tmp_path):
    """family_fuzz.recorded_fault_case(): the window's numbers are asserted by the program (span (56, 306), halo 5, wbeg 51, wlen
    261), the layout here: cell mode, 64-thread workgroups, two tiles, three slots of 264 samples.  Every kernel and the audit:
    clean -- the cause of the device's fault is not in what runs here (CHANGELOG)."""
    r, res = run_case(exe, ff.recorded_fault_case(), tmp_path, expect_window=[56, 306, 5, 51, 261])
    print(r.stdout)
    assert hk.is_clean(r), (r.stdout + r.stderr)[-4000:]
    halo, max_wlen, T, ntiles, syn_stride, cell, compact, nmis = (int(v) for v in res["layout"][:8])
    assert (halo, max_wlen, T, ntiles, syn_stride, cell, compact, nmis) == (5, 261, 64, 2, 3 * 264, 1, 0, 3)
    assert res["audit"][1] > 0 and res["audit"][2] > 0 and np.all(np.isfinite(res["misfit"]))


@pytest.mark.parametrize("reduced", [False, True], ids=["as_drawn", "first_receiver_only"])
@pytest.mark.parametrize("family,seed,index", SLICES, ids=["%s-%d" % (f, i) for f, _, i in SLICES])
def test_the_sweeps_layouts_run_clean(exe, tmp_path, family, seed, index, reduced):
    case = ff.case_of(family, seed, index)
    if reduced:
        case = first_receiver_only(case)
    r, res = run_case(exe, case, tmp_path)
    assert hk.is_clean(r), (case.describe(), (r.stdout + r.stderr)[-4000:])
    assert res["audit"][0] > 0                                   # (some (source, receiver, tile) was walked)


# ------------------------------------------------------------------------------------------------ the device against the host run
@pytest.mark.gpu
@pytest.mark.exact_only
def test_device_gram_and_solve_equal_the_host_run_kernels_bits(tmp_path):
    """The default scenario with the calls of tests/test_linfit_gpu.py test_device_equals_restatement_bit_for_bit (K = 6, one
    group): the device's by_receiver and coef against the SAME kernel text run on the host on the device's own kept traces.
    Built without the sanitizers (they are for the host tests above); skips where the machine has no host compiler."""
    from tests.linfit_cases import device_traces
    from tests.test_linfit_gpu import build
    exe = hk.build(tmp_path, sanitize=False)
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)
        rows = scattered_groups(np.random.default_rng(100 * K + 1), 1, K)
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit(0, 1, K, receiver_weights=WEIGHTS, anarchy=False, normal=True, by_receiver=True)
        syn, _, _ = device_traces(p, sc.comps, ENABLED, 0, 1, K)
    finally:
        p.close()
    e = sc.oracle()
    sc.apply_setup(e, True)
    a = hk.case_arrays(sc, e, rows, K, lambda eng, row: eng.set_source_params(6, row), enabled=ENABLED, weights=WEIGHTS, anarchy=False)
    e.close()
    sc.odb.close()
    a["proc_rows"] = np.concatenate([s.reshape(-1) for s in syn]).astype(np.float32)      # [slot][source][wlen]
    hk.write_arrays(tmp_path / "case.bin", a)
    r = hk.run(exe, tmp_path / "case.bin", tmp_path / "out.bin")
    assert r.returncode == 0 and "run: clean" in r.stdout, (r.stdout + r.stderr)[-3000:]
    res = hk.read_arrays(tmp_path / "out.bin")
    assert np.array_equal(res["by_receiver"].reshape(fit.by_receiver.shape), fit.by_receiver)
    assert np.array_equal(res["coef"].reshape(fit.coef.shape), fit.coef) and np.all(fit.status == 0)
