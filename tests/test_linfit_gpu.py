"""kiwi_hip_linear_fit on the device: the same BITS as the numpy restatement (tests/linfit_restatement.py) fed with the
device's own kept traces, whatever K, the number of groups, the receivers' components, the weights, the window length, the
first source, the chunking, the pieces and the kind of context; the evaluation it leaves behind; the moment-tensor helper on
planted and on bilateral data, for `moment_tensor` and `mt_eikonal`, with and without a misfit filter; the refusals; the
grid search with a free tensor per node and the example.  Every group of every case is solvable with the reference traces
alone or is one of the named degenerate ones: nothing is skipped."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import gridsearch, mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_int_p
from tests import common
from tests import linfit_restatement as lr
from tests.common import SYN_RTOL, Scenario, misfit_close, same_bits
from tests.linfit_cases import (PLANTED, UNIT, assert_beside_a_failed_piece, device_traces, eikonal_list_with_a_failed_piece, mt_row,
                                slots_as_receivers)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPS = ["d", "ne", "ned", "ardn", "ardne", "ned"]          # receivers of 1 to 5 components
FILTER = ([0.01, 0.03, 0.25, 0.4], [0., 1., 1., 0.])


def build(comps=None, planted=True, window=None, engine=None):
    """(scenario, product engine) with references of the planted tensor (or of the default bilateral rupture) and tapers over
    the whole reference traces, or over `window` samples from 20 samples behind their first one"""
    kw = dict(true_type=6, true_params=mt_row(PLANTED)) if planted else {}
    sc = Scenario(comps_list=comps, **kw)
    e = sc.oracle()
    sc.make_references(e)
    if window:
        for ir in range(1, sc.nrec + 1):
            sc.tapers[ir] = synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, window, sc.gf["dt"], 10.0)
    p = sc.product() if engine is None else engine(sc)
    sc.apply_setup(p, False)
    return sc, p


def multi_engine(ndev):
    def make(sc):
        from kiwi_amd import Engine
        g = sc.gf
        first, nsamp, data = sc.odb.dense_tables()
        p = Engine(0, ndev=ndev)
        p.set_database(g["dt"], g["dx"], g["dz"], g["firstx"], g["firstz"], data, first, nsamp)
        p.set_receivers(sc.lat, sc.lon, sc.depth, sc.comps)
        p.set_source_location(40.0, 30.0, 0.0)
        p.set_effective_dt(sc.effective_dt)
        p.set_local_interpolation("bilinear")
        return p
    return make


def scattered_groups(rng, ngroup, K):
    """basis sources that share nothing: every one its own time, place and tensor"""
    n = ngroup * K
    rows = np.zeros((n, 11), np.float32)
    rows[:, 0] = rng.uniform(-10., 10., n)
    rows[:, 1:3] = rng.uniform(-3000., 3000., (n, 2))
    rows[:, 3] = rng.uniform(8000., 12000., n)
    rows[:, 4:10] = rng.standard_normal((n, 6)) * 1e18
    rows[:, 10] = 1.0
    return rows


def colocated_groups(rng, ngroup, K=6):
    """K random tensors at the planted source's place per group: the planted data lie in their span (K = 6)"""
    rows = np.tile(mt_row(PLANTED), (ngroup * K, 1))
    rows[:, 4:10] = rng.standard_normal((ngroup * K, 6)) * 1e18
    return rows


def assert_bits(fit, rs, what=""):
    for name in ("coef", "misfit", "status", "pivot_min", "normal", "by_receiver"):
        a, b = getattr(fit, name), rs[name]
        assert a.shape == b.shape, (what, name)
        same = np.array_equal(a, b, equal_nan=(a.dtype != np.int32))
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a.ravel()[:4], b.ravel()[:4])
        assert same, (what, name)


def restate(p, sc, enabled, isrc0, ngroup, K, weights=None, anarchy=False, which=2):
    syn, ref, receivers = device_traces(p, sc.comps, enabled, isrc0, ngroup, K, which)
    return lr.fit(syn, ref, receivers, sc.gf["dt"], weights, anarchy)


def assert_same_fit(a, b, what=""):
    """two device fits of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.
    fused: a kernel instantiation contracts its multiply-adds on its own and the batch shape chooses the instantiation, so
    the kept traces agree within SYN_RTOL of their maximum (tests/common.py same_bits); for data inside the span of the basis
    (colocated_groups) a relative perturbation eps of the traces moves the solution by at most cond(A) eps <= cond(G) eps:
    |coef_a - coef_b| <= 64 cond(G) SYN_RTOL max|coef| (64: perturbation is relative to the trace MAXIMUM, not its norm)."""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("coef", "misfit", "pivot_min", "normal"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    for g in range(len(a.coef)):
        G, _, _ = lr.full_matrix(a.normal[g], a.coef.shape[1])
        s = 1.0 / np.sqrt(np.diag(G))
        cond = np.linalg.cond(G * s[:, None] * s[None, :])
        assert np.max(np.abs(a.coef[g] - b.coef[g])) <= 64 * cond * SYN_RTOL * np.max(np.abs(a.coef[g])), (what, g)


# ------------------------------------------------------------------------------------------------ 5: device == restatement
@pytest.mark.parametrize("K,ngroup,anarchy", [(1, 1, False), (1, 7, True), (2, 1, True), (2, 7, False), (6, 1, False),
                                              (6, 7, True), (8, 1, True), (8, 7, False), (6, 300, False), (8, 300, True)])
def test_device_equals_restatement_bit_for_bit(K, ngroup, anarchy):
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)                           # a disabled receiver
        enabled = [True] * 5 + [False]
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # a zero weight; the weight of the disabled receiver never counts
        rows = scattered_groups(np.random.default_rng(100 * K + ngroup), ngroup, K)
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit(0, ngroup, K, receiver_weights=w, anarchy=anarchy, normal=True, by_receiver=True)
        rs = restate(p, sc, enabled, 0, ngroup, K, w, anarchy)
        assert_bits(fit, rs, "K=%d ngroup=%d" % (K, ngroup))
        print("K=%d ngroup=%d: smallest pivot %.3g" % (K, ngroup, fit.pivot_min.min()))
        assert np.all(fit.status == 0) and np.all(np.isfinite(fit.coef)) and np.all(fit.pivot_min > 1e-9)
        assert np.all(fit.by_receiver[:, 5] == 0.0) and np.all(fit.by_receiver[:, 1, -1] > 0.0)
        ms = p.linear_fit_ms()
        assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0
        # without weights: ones
        if ngroup == 7:
            assert_bits(p.linear_fit(0, ngroup, K, anarchy=anarchy, normal=True, by_receiver=True),
                        restate(p, sc, enabled, 0, ngroup, K, None, anarchy), "no weights")
    finally:
        p.close()


@pytest.mark.parametrize("window", [100, 256, 4096])
def test_window_lengths(window):
    sc, p = build(COMPS, window=window)
    try:
        assert len(p.get_reference(3, 1, 2)[1]) == window
        rows = scattered_groups(np.random.default_rng(window), 3, 6)
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit(0, 3, 6, normal=True, by_receiver=True)
        assert_bits(fit, restate(p, sc, [True] * 6, 0, 3, 6), "window %d" % window)
        assert np.all(fit.status == 0)
    finally:
        p.close()


def test_degenerate_groups_on_the_device():
    """an all-zero basis source (zero diagonal: status 1, pivot 0), two identical ones (status 1 or a pivot of round-off size)
    and a solvable group in one call; NaNs where stated, the sums still returned; bit for bit like the restatement"""
    sc, p = build(COMPS)
    try:
        rows = scattered_groups(np.random.default_rng(3), 3, 2)
        rows[1, 4:10] = 0.0                                   # group 0: second basis source without moment
        rows[3] = rows[2]                                     # group 1: twice the same source
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit(0, 3, 2, normal=True, by_receiver=True)
        assert_bits(fit, restate(p, sc, [True] * 6, 0, 3, 2), "degenerate")
        print("degenerate groups: status", fit.status, "pivot_min", fit.pivot_min)
        assert fit.status[0] == 1 and fit.pivot_min[0] == 0.0 and np.all(np.isnan(fit.coef[0])) and np.isnan(fit.misfit[0])
        assert fit.normal[0][lr.tri(2, 1, 1)] == 0.0 and fit.normal[0][0] > 0.0
        assert fit.status[1] == 1 or fit.pivot_min[1] < 1e-9
        assert fit.status[2] == 0 and fit.pivot_min[2] > 1e-3 and np.all(np.isfinite(fit.coef[2]))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: the same bits however it is cut
def test_first_source_chunks_pieces_and_contexts(monkeypatch):
    from kiwi_amd import Engine
    ngroup, K = 40, 6
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    sc, p = build(COMPS)
    try:
        p.set_source_params("moment_tensor", rows)
        base = p.linear_fit(0, ngroup, K, normal=True)
        assert np.all(base.status == 0)
        tensors = (base.coef[:, :, None] * rows.reshape(ngroup, K, 11)[:, :, 4:10]).sum(1)      # sum_i x_i T_i: the planted tensor
        assert np.all(np.abs(tensors - PLANTED) <= 1e-5 * np.abs(PLANTED))
        # isrc0 > 0, not a multiple of K, and against the restatement there
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        shifted = p.linear_fit(5, ngroup, K, normal=True, by_receiver=True)
        assert_bits(shifted, restate(p, sc, [True] * 6, 5, ngroup, K), "isrc0 = 5")
        assert_same_fit(base, shifted, "isrc0 = 5")
        # pieces of one group and of the default
        for piece in (K, 0, 13 * K + 2):
            assert_same_fit(base, p.linear_fit_params("moment_tensor", rows, K, normal=True, piece=piece), "piece %d" % piece)
            assert p.nsrc == (K if piece == K else (len(rows) if piece == 0 else 13 * K))
            p.eval()                                          # the engine holds the head of the list and knows how long it is
    finally:
        p.close()
    # several chunks: KIWI_HIP_CHUNK_MB is read at kiwi_hip_init
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")
    sc, q = build(COMPS)
    try:
        q.set_source_params("moment_tensor", rows)
        chunked = q.linear_fit(0, ngroup, K, normal=True, by_receiver=True)
        assert_same_fit(base, chunked, "chunks")
        # against the restatement: traces of earlier chunks are evaluated again source by source, which gives the same bits
        # under the exact contract (a source's evaluation does not depend on its batch)
        if common.arith() == "exact":
            assert_bits(chunked, restate(q, sc, [True] * 6, 0, ngroup, K), "chunks")
        q.eval()
        assert len(q.kernel_ms()[1]) == 3
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    # a multi-device context of one device, and two contexts stacked on device 0
    import torch
    for ndev in (1, 2):
        if ndev == 2 and torch.cuda.device_count() < 2:
            monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
        sc, m = build(COMPS, engine=multi_engine(ndev))
        try:
            assert m.ndevices() == ndev
            assert_same_fit(base, m.linear_fit_params("moment_tensor", rows, K, normal=True), "ndev %d" % ndev)
            assert_same_fit(base, m.linear_fit_params("moment_tensor", rows, K, normal=True, piece=2 * K), "ndev %d pieces" % ndev)
        finally:
            m.close()


# ------------------------------------------------------------------------------------------------ 7: what the call leaves behind
def test_misfits_of_the_basis_sources_are_those_of_an_evaluation():
    rows = np.concatenate([colocated_groups(np.random.default_rng(1), 5), scattered_groups(np.random.default_rng(2), 5, 6)])
    sc, p = build(COMPS)
    sc2, q = build(COMPS)
    try:
        p.set_source_params("moment_tensor", rows)
        p.linear_fit(6, 9, 6)
        q.set_source_params("moment_tensor", rows)
        q.eval()
        a, b = p.get_misfits(6, 54), q.get_misfits(6, 54)
        for x, y in zip(a, b):
            assert same_bits(x, y)
        assert np.all(a[0] > 0)
        with pytest.raises(KiwiHipError):
            p.get_misfits(0, 6)                               # sources outside the range were not evaluated
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ 8: the moment-tensor helper
def _predicted(p, sc, coef, which=2):
    """per-slot misfits the quadratic form predicts for the combination `coef` of the six uploaded basis sources"""
    syn, ref, receivers = device_traces(p, sc.comps, [True] * sc.nrec, 0, 1, 6, which)
    per_slot = lr.gram_by_receiver(syn, ref, slots_as_receivers(receivers), sc.gf["dt"])[0]
    return lr.predicted_slot_misfits(per_slot, coef)


def test_planted_tensor_recovered_through_fit_moment_tensors():
    sc, p = build(COMPS)
    try:
        rows = np.stack([mt_row(np.zeros(6)), mt_row(np.ones(6), location=[0.2, 800., -500., 11000.])])
        tensors, misfit, status, pivot = mtfit.fit_moment_tensors(p, "moment_tensor", rows)
        rel = np.abs(tensors[0] - PLANTED) / np.abs(PLANTED)
        print("planted tensor through the device: relative error", rel, "misfit", misfit, "pivot_min", pivot)
        assert np.all(status == 0) and np.all(rel <= 1e-5)
        assert misfit[0] <= 1e-5 and misfit[1] > 10 * misfit[0] and np.all(pivot > 0.5)
        dev, dmis, dstatus, dpiv = mtfit.fit_moment_tensors(p, "moment_tensor", rows, deviatoric=True)
        assert np.all(dstatus == 0) and np.all(np.abs(dev[:, :3].sum(1)) <= 1e-12 * np.abs(dev).max(1))
        assert np.all(dmis >= misfit)
    finally:
        p.close()


@pytest.mark.parametrize("sourcetype", ["moment_tensor", "mt_eikonal"])
def test_bilateral_data_fitted_tensor_predicts_the_engines_misfits(sourcetype, monkeypatch):
    sc, p = build(None, planted=False)
    try:
        if sourcetype == "mt_eikonal":
            G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
            p.set_source_crust(G["rupture_profile"], G["origin_profile"])
            p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
            row = np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32)
            c0 = 13
        else:
            row = mt_row(np.zeros(6))
            c0 = 4
        tensors, misfit, status, pivot = mtfit.fit_moment_tensors(p, sourcetype, row)
        assert status[0] == 0 and pivot[0] > (0.5 if sourcetype == "moment_tensor" else 1e-3)
        assert p.nsrc == 6                                    # the engine holds the six basis sources
        fitted = row.copy()
        fitted[c0:c0 + 6] = tensors[0]
        pm_pred = _predicted(p, sc, fitted[c0:c0 + 6].astype(np.float64) / UNIT)
        p.set_source_params(sourcetype, fitted)
        p.eval()
        pm, pn, pg = p.get_misfits()
        print("%s: worst |predicted - evaluated| / max(misfit, norm) %.3g; global predicted %.9f evaluated %.9f" % (
            sourcetype, np.max(np.abs(pm_pred - pm[0]) / np.maximum(pm[0], pn[0])), misfit[0], pg[0]))
        contract = common.arith()
        monkeypatch.setenv("KIWI_HIP_ARITH", "fused")         # the rule on the scale of the norm factors, for both contracts
        assert misfit_close(pm[0], pm_pred, norm=pn[0])
        assert misfit_close(pg[0], misfit[0], glob=True)
        monkeypatch.setenv("KIWI_HIP_ARITH", contract)
        if sourcetype == "moment_tensor":                     # no double couple of the cfg2 grid at this place does better
            grid = synthetic.mt_sdr_grid(depth=float(row[3]), risetime=float(row[10]))
            _, _, g, _ = p.misfits_for_params("moment_tensor", grid)
            print("best double couple of %d: %.6f, fitted tensor %.6f" % (len(grid), g.min(), misfit[0]))
            assert misfit[0] <= g.min()
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 9: with a misfit filter
def test_with_a_misfit_filter(monkeypatch):
    for fused_fft in ("0", None):
        if fused_fft is not None:
            monkeypatch.setenv("KIWI_HIP_FUSED_FFT", fused_fft)     # library transforms throughout: get_reference(3) then is the
        else:                                                      # reference the fit compared with (it forces them for its call)
            monkeypatch.delenv("KIWI_HIP_FUSED_FFT", raising=False)
        sc, p = build(None, planted=False)
        try:
            for ir in range(1, sc.nrec + 1):
                p.set_misfit_filter(ir, *FILTER)
            basis = mtfit.elementary_params("moment_tensor", mt_row(np.zeros(6)), UNIT)
            p.set_source_params("moment_tensor", basis)
            fit = p.linear_fit(0, 1, 6, normal=True, by_receiver=True)
            assert fit.status[0] == 0 and fit.pivot_min[0] > 0.1
            if fused_fft == "0":
                assert_bits(fit, restate(p, sc, [True] * 6, 0, 1, 6, which=3), "filtered")
            fitted = mt_row((fit.coef[0] * UNIT).astype(np.float32))
            pm_pred = _predicted(p, sc, fitted[4:10].astype(np.float64) / UNIT, which=3)
            p.set_source_params("moment_tensor", fitted)
            p.eval()
            pm, pn, pg = p.get_misfits()
            dt = sc.gf["dt"]
            nt, wl, na, nb = [], [], [], []
            for ir in range(1, sc.nrec + 1):
                for k in range(1, 4):
                    a, b = p.get_reference(ir, k, 2)[1].astype(np.float64), p.get_synthetics(0, ir, k, 2)[1].astype(np.float64)
                    nt.append(2 * (len(p.get_amp_spectrum(ir, k)[1]) - 1)); wl.append(len(a))
                    na.append(np.sqrt(dt * np.sum(a * a))); nb.append(np.sqrt(dt * np.sum(b * b)))
            ok, ratio = common.spectral_close("l2norm", dt, pm[0], pm_pred, pn[0], (np.array(nt), np.array(wl), np.array(na), np.array(nb)))
            print("filtered (KIWI_HIP_FUSED_FFT=%s): excess over 1e-6 / round-off bound %.3g; global predicted %.9f evaluated %.9f" % (
                fused_fft, ratio, fit.misfit[0], pg[0]))
            assert ok
        finally:
            p.close()


# ------------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert same_bits(x, y)

        def refused(match, call=None):
            with pytest.raises(KiwiHipError, match=match):
                (call or (lambda: p.linear_fit(0, 2, 6)))()
            with pytest.raises(KiwiHipError, match=match):
                p.linear_fit_params("moment_tensor", rows, 6)
            p.set_source_params("moment_tensor", rows)        # (a failed list call leaves no batch the engine may index)

        for method in ("l1norm", "ampspec_l2norm", "scalar_product", "peak"):
            p.set_misfit_method(method)
            refused("l2norm")
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(1, -1.0, 1.0)
        refused("floating shift")
        p.set_misfit_method("l2norm")
        still_usable()
        # K and the range, through the C entry itself (the Python method checks K before it calls)
        out = dict(coef=np.zeros(64), misfit=np.zeros(8), status=np.zeros(8, np.int32))
        dp = lambda a: a.ctypes.data_as(c_double_p)           # noqa: E731
        for K in (0, 9, -1):
            rc = p.L.kiwi_hip_linear_fit(p.h, 0, 1, K, None, 0, dp(out["coef"]), dp(out["misfit"]), out["status"].ctypes.data_as(c_int_p),
                                         None, None, None)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="basis sources per group"):
                p._ck(rc, "linear_fit")
            with pytest.raises(KiwiHipError, match="basis sources per group"):
                p.linear_fit(0, 1, K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            with pytest.raises(KiwiHipError, match="not inside the uploaded batch"):
                p.linear_fit(isrc0, ngroup, 6)
        still_usable()
        assert np.all(p.linear_fit(0, 2, 6).status == 0)
    finally:
        p.close()
    # an enabled receiver without a taper
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[2]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.linear_fit(0, 2, 6)
        p.eval()
        assert np.all(p.get_misfits()[0] > 0)
        p.switch_receiver(2, False)                           # disabled: it does not matter any more
        assert np.all(p.linear_fit(0, 2, 6).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 11: grid search and example
def test_grid_search_with_a_free_tensor_per_node():
    true_row = mt_row(PLANTED, location=[0., 800., -400., 11000.])
    sc = Scenario(true_type=6, true_params=true_row)
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        grid = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)),
                                     param_values=[("north-shift", 800. + 400. * np.arange(-2, 3)), ("east-shift", -400. + 400. * np.arange(-2, 3)),
                                                   ("depth", [10000., 11000., 12000.])])
        assert len(grid.sources) == 75
        grid.compute(p, linear_mt=True)
        best = grid.best_source
        print("grid search: best node", best[:4], "misfit", grid.fit_misfits[grid.ibest], "second best", np.sort(grid.fit_misfits)[1])
        assert np.array_equal(best[1:4], true_row[1:4])
        assert np.all(np.abs(best[4:10] - PLANTED) <= 1e-5 * np.abs(PLANTED))
        assert np.all(grid.fit_status == 0) and grid.fit_misfits[grid.ibest] <= 1e-5
        assert np.sort(grid.fit_misfits)[1] > 100 * grid.fit_misfits[grid.ibest]
        grid.postprocess(bootstrap_iterations=20, rng=np.random.default_rng(0))
        assert grid.ibest == int(np.argmin(grid.fit_misfits)) and grid.stats["depth"].best == 11000.0
        # without the argument nothing changes
        plain = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("depth", [10000., 11000.])])
        plain.compute(p)
        assert np.array_equal(plain.sources[:, 4:10], np.full((2, 6), np.float32(1e18))) and not hasattr(plain, "fit_misfits")
        with pytest.raises(KiwiHipError):
            gridsearch.MisfitGrid("bilateral", synthetic.TRUE_BILAT, param_values=[("depth", [10000.])]).compute(p, linear_mt=True)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_moment_tensor.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "best grid point" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
def test_a_piece_in_which_every_basis_source_fails_to_discretise():
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(None, planted=False)
    try:
        eik, good = eikonal_list_with_a_failed_piece(p)
        kw = dict(normal=True, by_receiver=True, piece=2)
        got = p.linear_fit_params("mt_eikonal", eik, 2, **kw)
        assert list(got.status) == [0, 2, 0]
        assert np.all(np.isnan(got.coef[1])) and np.isnan(got.misfit[1])
        assert got.pivot_min[1] == 0.0 and not np.any(got.normal[1]) and not np.any(got.by_receiver[1])
        assert_beside_a_failed_piece(got, p.linear_fit_params("mt_eikonal", good, 2, **kw), common.arith())
    finally:
        p.close()
