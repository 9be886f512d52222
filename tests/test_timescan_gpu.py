"""kiwi_hip_time_scan on the device: the scan at offset k is bit for bit the separate evaluation of the sources moved by k dt
(the parent commit's path: set_source_params + eval + get_misfits) where every centroid's time / dt is exact in fp32, and bit
for bit the evaluation with references and tapers moved by -k samples for any source under the unfiltered time-domain methods;
whatever the method, the filters, the rise-time fold, the window, the number of offsets, the first source, the pieces, the
chunking and the kind of context; what the call leaves behind; the refusals; the grid search.  Under the `fused` arithmetic
contract the two calls may be served by different instantiations of the accumulate kernel: where their synthetics differ,
tests/timescan_cases.py assert_scan_equal applies the tolerance of include/kiwi_hip.h and says so."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd.lib import KiwiHipError
from tests import common
from tests import timescan_cases as tc
from tests.bands_cases import ALL_BANDS, assert_bands_equal, separate, trial_list
from tests.linfit_cases import eikonal_list_with_a_failed_piece
from tests.test_linfit_gpu import build, multi_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_children = {}


def child(arith, cases, env_extra):
    """named cases of tests/timescan_cases.py in a process of its own, run once per arithmetic contract and shared"""
    key = (arith, tuple(cases), tuple(sorted(env_extra.items())))
    if key not in _children:
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_timescan_child_%d.npz" % os.getpid())
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "timescan_cases.py"), out] + list(cases), capture_output=True, text=True,
                           env=dict(os.environ, **env_extra), timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        _children[key] = dict(np.load(out))
        os.remove(out)
    return _children[key]


def unfused(arith):
    """KIWI_HIP_FUSE=0: the plain evaluation of a batch without rise-time fold compares in misfit_kernel, the order the scan uses"""
    return child(arith, ["methods", "fold", "grid"], dict(KIWI_HIP_FUSE="0"))


@pytest.mark.parametrize("filt", tc.FILTERS)
@pytest.mark.parametrize("method", tc.METHODS)
def test_every_method_with_and_without_filter_equals_the_moved_sources(_arith, method, filt):
    z = unfused(_arith)
    key = "methods_%s_%s_" % (method, filt)
    got = (z[key + "m"], z[key + "n"], z[key + "g"])
    want = (z[key + "sm"], z[key + "sn"], z[key + "sg"])
    assert got[0].shape == (8, 6, 11) and got[1].shape == (8, 11) and got[2].shape == (8, 6)
    assert np.all(np.isfinite(got[0])) and np.all(got[0] != 0) and np.all(got[1] > 0)
    assert np.any(got[0][:, 0] != got[0][:, 1]), "the offsets change the misfits"
    tc.assert_scan_equal(got, want, "%s, filter %s" % (method, filt))
    assert np.array_equal(z[key + "b"], tc.first_argmin(got[2]))


@pytest.mark.parametrize("method", ["l2norm", "ampspec_l1norm"])
def test_rise_time_fold_on_the_scan_path(_arith, method):
    z = unfused(_arith)
    key = "fold_%s_" % method
    got = (z[key + "m"], z[key + "n"], z[key + "g"])
    assert np.all(np.isfinite(got[0])) and np.all(got[0] != 0)
    tc.assert_scan_equal(got, (z[key + "sm"], z[key + "sn"], z[key + "sg"]), "rise times 0, 1, 2 s, %s" % method)
    assert np.array_equal(z[key + "b"], tc.first_argmin(got[2]))


def test_a_rejected_source_reads_as_zeros_with_best_minus_one():
    """Only the eikonal source types keep a source the discretiser rejects in the batch (a rejected `moment_tensor` row fails the
    whole upload), so the rejected source sits in an `mt_eikonal` batch: zeros and best = -1 for it, and its neighbours as
    without it; offset 0 of every good source is its plain evaluation."""
    sc, p = build(None, planted=False)
    try:
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (5, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((5, 6)) * 1e18
        eik[2, 3] = 500.0                                     # "Empty rupture area": above the constraining planes
        m, n, g, b, failings = p.time_scan_for_params("mt_eikonal", eik, *tc.OFFSETS)
        assert failings == [2] and b[2] == -1
        assert np.all(m[2] == 0) and np.all(n[2] == 0) and np.all(g[2] == 0)
        good = [0, 1, 3, 4]
        assert np.array_equal(b[good], tc.first_argmin(g[good]))
        try:
            p.set_source_params("mt_eikonal", eik)            # the failing inside an uploaded batch
        except KiwiHipError:
            pass
        assert list(np.nonzero(p.get_source_status())[0]) == [2]
        tc.assert_scan_equal(p.time_scan(0, None, *tc.OFFSETS), (m, n, g), "uploaded batch with a failing")
        assert np.array_equal(p.time_scan(0, None, *tc.OFFSETS)[3], b)
        p.set_source_params("mt_eikonal", eik[good])
        m1, n1, g1, b1 = p.time_scan(0, None, *tc.OFFSETS)
        tc.assert_scan_equal((m1, n1, g1), (m[good], n[good], g[good]), "sources beside a failing")
        p.eval()
        pm, pn, pg = p.get_misfits()
        m0, n0, g0, _ = p.time_scan(0, None, 0, 1, 1)
        tc.assert_scan_equal((m0, n0, g0), (pm[:, None], pn, pg[:, None]), "offset 0 is the plain evaluation")
    finally:
        p.close()


@pytest.mark.parametrize("method", tc.TIME_DOMAIN)
def test_references_and_tapers_moved_the_other_way(method):
    """route B: any source -- fractional centroid times, a rise time of 2 s -- under an unfiltered time-domain method"""
    sc, p = tc.standard()
    try:
        dt = sc.gf["dt"]
        p.set_misfit_method(method)
        p.set_source_params("bilateral", trial_list(8))
        m, n, g, b = p.time_scan(0, None, *tc.OFFSETS)
        ms, gs = [], []
        for k in tc.offsets(*tc.OFFSETS):
            for ir in range(1, sc.nrec + 1):
                p.shift_ref_seismogram(ir, -k * dt)
                x, y = sc.tapers[ir]
                p.set_misfit_taper(ir, np.asarray(x, np.float32) - np.float32(k * dt), y)
            p.eval()
            pm, pn, pg = p.get_misfits()
            assert np.array_equal(pn, n), "norm factors of the moved references under the moved tapers"
            ms.append(pm); gs.append(pg)
            for ir in range(1, sc.nrec + 1):
                p.shift_ref_seismogram(ir, k * dt)
        want = (np.stack(ms, 1), n, np.stack(gs, 1))
        assert np.any(want[0][:, 0] != want[0][:, -1])
        tc.assert_scan_equal((m, n, g), want, "route B, %s" % method)
        assert np.array_equal(b, tc.first_argmin(g))
    finally:
        p.close()


SHAPE_SCANS = [(0, 1, 1), (-30, 30, 3), (-30, 20, 4), (-30, 15, 5), (-28, 7, 9)]      # nk = 1 and 3, 4, 5 around the kernel's four per pass, 9


@pytest.mark.parametrize("window", [100, 257, 600])
def test_window_shapes_and_offsets_per_pass(window):
    """explicit centroid tables with dyadic times and rise times (so that the plain evaluation compares in misfit_kernel, like
    the scan), |k| up to 30: the onset of the synthetic crosses the window's edge, 20 samples behind the reference's first"""
    assert tc.PER_PASS == 4 and {s[2] for s in SHAPE_SCANS} >= {1, tc.PER_PASS - 1, tc.PER_PASS, tc.PER_PASS + 1, 9}
    sc, p = tc.standard(window)
    try:
        dt = sc.gf["dt"]
        tabs, moments, rises = tc.fold_batch()
        rises = np.maximum(rises, 1.0).astype(np.float32)
        p.set_synthetics_factor(0.5)
        p.set_sources(tabs, moments, rises)
        p.eval()
        plain = p.get_misfits()
        ks = sorted(set(k for s in SHAPE_SCANS for k in tc.offsets(*s)))
        sm, sn, sg = tc.separate_tables(p, tabs, moments, rises, ks, dt)
        assert np.array_equal(sm[:, ks.index(0)], plain[0])
        p.set_sources(tabs, moments, rises)
        for scan in SHAPE_SCANS:
            idx = [ks.index(k) for k in tc.offsets(*scan)]
            m, n, g, b = p.time_scan(0, None, *scan)
            tc.assert_scan_equal((m, n, g), (sm[:, idx], sn, sg[:, idx]), "window %d, scan %s" % (window, scan))
            assert np.array_equal(b, tc.first_argmin(g))
        m, n, g, b = p.time_scan(0, None, 0, 1, 1)
        tc.assert_scan_equal((m[:, 0], n, g[:, 0]), plain, "nk = 1, k0 = 0 is eval + get_misfits")
        assert np.any(sm[:, 0] != sm[:, -1])
    finally:
        p.close()


def test_independence_of_routing(_arith, monkeypatch):
    tr, dup = tc.routing_sources()
    n = len(tr)
    sc, p = tc.standard()
    try:
        p.set_source_params("bilateral", tr)
        got = p.time_scan(0, None, *tc.OFFSETS)
        sub = p.time_scan(5, 7, *tc.OFFSETS)
        tc.assert_scan_equal(sub, tuple(x[5:12] for x in got), "isrc0 = 5")
        assert np.array_equal(sub[3], got[3][5:12])
        for piece in (3, n):
            m, nn, g, b, failings = p.time_scan_for_params("bilateral", tr, *tc.OFFSETS, piece=piece)
            assert failings == [] and p.nsrc == min(piece, n)
            tc.assert_scan_equal((m, nn, g), got, "piece %d" % piece)
            assert np.array_equal(b, got[3])
        p.set_source_params("bilateral", dup)
        got_dup = p.time_scan(0, None, *tc.OFFSETS)
        assert np.any(got_dup[0][0] != got_dup[0][1])          # one table, different moments
    finally:
        p.close()
    # several chunks, and shared synthetics forced on: read when a context is made -- a process of its own
    z = child(_arith, ["routing"], dict(KIWI_HIP_CHUNK_MB="1", KIWI_HIP_DEDUPE="2"))
    assert z["routing_list_launches"][1] >= 3, z["routing_list_launches"]
    for name, want in (("list", got), ("dup", got_dup)):
        tc.assert_scan_equal(tuple(z["routing_%s_%s" % (name, q)] for q in "mng"), want, "chunks and KIWI_HIP_DEDUPE=2, %s" % name)
        assert np.array_equal(z["routing_%s_b" % name], want[3])
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = build(tc.COMPS, planted=False, window=tc.WINDOW, engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        m2.switch_receiver(6, False)
        m, nn, g, b, failings = m2.time_scan_for_params("bilateral", tr, *tc.OFFSETS, piece=3)
        assert failings == []
        tc.assert_scan_equal((m, nn, g), got, "two devices")
        assert np.array_equal(b, got[3])
    finally:
        m2.close()


def test_state_afterwards():
    """after a scan the context evaluates as one that never scanned, and the band call still matches its separate evaluations"""
    tr = trial_list(6)
    sc, fresh = tc.standard()
    try:
        fresh.set_source_params("bilateral", tr)
        fresh.eval()
        want = fresh.get_misfits()
    finally:
        fresh.close()
    sc, p = tc.standard()
    try:
        p.set_source_params("bilateral", tr)
        p.time_scan(0, None, -30, 12, 6)
        after_scan = p.get_misfits()                          # what the scan leaves: the plain evaluation of the range
        p.eval()
        again = p.get_misfits()
        for a, b, c in zip(after_scan, again, want):
            assert np.array_equal(b, c)                       # the bits of a context that never scanned
            assert common.same_bits(a, c) if common.arith() == "exact" else common.misfit_close(a, c, norm=want[1] if a.ndim == 2 else None, glob=a.ndim == 1)
        p.set_keep_synthetics(2)
        p.eval()
        kept = p.get_synthetics(1, 2, 1, 2)
        p.time_scan(0, None, 0, 5, 3)
        lo, d = p.get_synthetics(1, 2, 1, 2)
        assert lo == kept[0] and np.array_equal(d, kept[1])   # kept synthetics are where they were
        p.set_keep_synthetics(0)
        bands = [ALL_BANDS[i] for i in (0, 5, 8, 11)]
        p.set_misfit_bands(bands)
        got = p.band_misfits()
        assert_bands_equal(got, separate(p, bands), "bands after a scan")
    finally:
        p.close()


def test_refusals_name_the_reason():
    sc, p = tc.standard()
    try:
        tr = trial_list(5)
        p.set_source_params("bilateral", tr)
        assert p.L.kiwi_hip_time_scan_max_shift() == 1024 and p.L.kiwi_hip_time_scan_max_offsets() == 256
        with pytest.raises(KiwiHipError, match="need at least one offset"):
            p.time_scan(0, None, 0, 1, 0)
        with pytest.raises(KiwiHipError, match="257 offsets; at most 256"):
            p.time_scan(0, None, -128, 1, 257)
        with pytest.raises(KiwiHipError, match="kstep = 0"):
            p.time_scan(0, None, 0, 0, 3)
        with pytest.raises(KiwiHipError, match=r"offsets 1000 \.\. 1030 samples; the largest shift is 1024"):
            p.time_scan(0, None, 1000, 10, 4)
        with pytest.raises(KiwiHipError, match="the largest shift is 1024"):
            p.time_scan(0, None, -1025, 1, 2)
        with pytest.raises(KiwiHipError, match="not inside the uploaded batch"):
            p.time_scan(2, 4, 0, 1, 2)
        p.set_misfit_method("floating_l1norm")
        with pytest.raises(KiwiHipError, match="floating norm"):
            p.time_scan(0, None, 0, 1, 2)
        with pytest.raises(KiwiHipError, match="floating norm"):
            p.time_scan_for_params("bilateral", tr, 0, 1, 2)
        p.set_misfit_method("l2norm")
        p.set_misfit_taper(2, [], [])
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.time_scan(0, None, 0, 1, 2)
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.time_scan_for_params("bilateral", tr, 0, 1, 2)
        p.set_misfit_taper(2, *sc.tapers[2])
        # a transform length the in-LDS transforms do not take: a reference of 20000 samples asks for 65536
        lo, d = sc.refs[(1, 1)]
        p.set_ref_seismogram(1, 1, lo, np.concatenate([d, np.zeros(20000 - len(d), np.float32)]))
        p.set_misfit_method("ampspec_l2norm")
        p.set_source_params("bilateral", tr)
        with pytest.raises(KiwiHipError, match="needs a transform of 65536 samples"):
            p.time_scan(0, None, 0, 1, 2)
        # the context is usable afterwards: the largest shift either way
        p.set_ref_seismogram(1, 1, lo, d)
        p.set_misfit_method("l1norm")
        p.set_source_params("bilateral", tr)
        m, n, g, b = p.time_scan(0, None, -1024, 2048, 2)
        assert m.shape == (5, 2, 11) and np.all(np.isfinite(m)) and np.all(n > 0)
    finally:
        p.close()
    # an enabled receiver component without a reference
    sc, q = tc.standard()
    q.close()
    q = sc.product()
    try:
        for (ir, k), (lo, d) in sc.refs.items():
            if (ir, k) != (3, 2):
                q.set_ref_seismogram(ir, k, lo, d)
        for ir, (x, y) in sc.tapers.items():
            q.set_misfit_taper(ir, x, y)
        q.set_source_params("bilateral", trial_list(3))
        with pytest.raises(KiwiHipError, match="needs a reference seismogram"):
            q.time_scan(0, None, 0, 1, 2)
    finally:
        q.close()
    # a row too long for LDS: the message names the length
    sc, r = build(tc.COMPS, planted=False, window=38000)
    try:
        r.set_source_params("bilateral", trial_list(3))
        with pytest.raises(KiwiHipError, match=r"a row of 38\d\d\d samples .* does not fit in LDS; the limit is 37888"):
            r.time_scan(0, None, -8, 4, 5)
    finally:
        r.close()


def test_library_transforms_only_is_refused_in_a_process_of_its_own(_arith):
    z = child(_arith, ["nofused"], dict(KIWI_HIP_FUSED_FFT="0"))
    assert "KIWI_HIP_FUSED_FFT=0 switches off" in str(z["nofused_error"])
    tc.assert_scan_equal(tuple(z["nofused_" + q] for q in "mng"), tuple(z["nofused_s" + q] for q in "mng"), "unfiltered l2norm, KIWI_HIP_FUSED_FFT=0")


def test_grid_search_with_a_scanned_time_axis(_arith):
    from kiwi_amd import gridsearch
    sc, p = tc.standard()
    try:
        a, b = tc.grid(sc), tc.grid(sc)
        a.compute(p)
        b.compute(p, time_scan=True)
        assert b.syntheses_saved == 12 and len(b.sources) == 15
        assert a.misfits_by_src.shape == b.misfits_by_src.shape == (15, 6, 3) and a.failings == b.failings == []
        assert np.array_equal(a.norms_by_src, b.norms_by_src)
        scale = np.maximum(np.abs(a.misfits_by_src), a.norms_by_src)
        assert np.all(np.abs(a.misfits_by_src - b.misfits_by_src) <= 1e-6 * scale)       # the header's bound
        a.postprocess(bootstrap_iterations=3, rng=np.random.default_rng(1))
        b.postprocess(bootstrap_iterations=3, rng=np.random.default_rng(1))
        assert a.ibest == b.ibest and np.array_equal(a.best_source, b.best_source)
        with pytest.raises(ValueError, match="linear_mt"):
            b.compute(p, time_scan=True, linear_mt=True)
        c = gridsearch.MisfitGrid("moment_tensor", a.base_params, param_values=[("depth", [9000., 10000.]), ("time", [0.0, 0.3, 0.6])])
        with pytest.raises(ValueError, match="not evenly spaced by a whole number of samples"):
            c.compute(p, time_scan=True)
        p.time_scan_for_params("moment_tensor", a.sources[:3], 0, 1, 2)
        ms = p.time_scan_ms()
        print("scan call: evaluation %.3f ms, scan kernels %.3f ms, downloads %.3f ms" % ms)
        assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0 and ms[2] >= 0
    finally:
        p.close()
    z = unfused(_arith)
    if _arith == "exact":                                     # KIWI_HIP_FUSE=0: the two routes compare in the same order
        assert np.array_equal(z["grid_m"], z["grid_sm"]) and np.array_equal(z["grid_n"], z["grid_sn"])
    else:
        assert np.all(np.abs(z["grid_m"] - z["grid_sm"]) <= 1e-6 * np.maximum(np.abs(z["grid_m"]), z["grid_n"]))


def test_example_script_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_timescan.py")], capture_output=True, text=True,
                         env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "planted time found" in out.stdout and "syntheses saved" in out.stdout, out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
def test_a_piece_in_which_every_source_fails_to_discretise():
    """three `mt_eikonal` sources in pieces of one, the middle one failing to discretise: nothing is uploaded for that piece.  It reads
    as zeros with best = -1, its neighbours as the call without it gives them"""
    sc, p = build(None, planted=False)
    try:
        eik, good = eikonal_list_with_a_failed_piece(p, 1)
        m, n, g, b, failings = p.time_scan_for_params("mt_eikonal", eik, *tc.OFFSETS, piece=1)
        assert failings == [1] and b[1] == -1
        assert not np.any(m[1]) and not np.any(n[1]) and not np.any(g[1])
        m2, n2, g2, b2, none = p.time_scan_for_params("mt_eikonal", good, *tc.OFFSETS, piece=1)
        assert none == []
        tc.assert_scan_equal((m[[0, 2]], n[[0, 2]], g[[0, 2]]), (m2, n2, g2), "sources beside a piece of which nothing is uploaded")
        assert np.array_equal(b[[0, 2]], b2)
    finally:
        p.close()
