"""kiwi_hip_linear_fit_robust on the device: the same BITS as the numpy restatement (tests/linfit_robust_restatement.py) fed
with the device's own kept traces, in both modes -- A: misfit method l1norm, B: l2norm, outer norm l1norm --, whatever K, the
number of groups, the iterations, the weights, the window length, the first source, the chunking, the pieces and the kind
of context; what the fitted tensor's evaluation gives; a corrupted receiver; the forwarding to kiwi_hip_linear_fit; the
refusals; degenerate groups; a misfit filter; the grid search and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import engine as kengine
from kiwi_amd import gridsearch, mtfit
from kiwi_amd.lib import KiwiHipError, c_double_p, c_int_p
from tests import common
from tests import linfit_restatement as lr
from tests import linfit_robust_restatement as rr
from tests.common import SYN_RTOL, Scenario, misfit_close
from tests.linfit_cases import PLANTED, UNIT, device_traces, mt_row
from tests.test_linfit_gpu import COMPS, FILTER, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHOD = {"A": "l1norm", "B": "l2norm"}
EPS = 1e-3


def assert_answers(fit, rs, n, what=""):
    """a device call with niter = n against a restatement of at least n iterations"""
    for name, b in (("coef", rs["coef_at"][:, n]), ("misfit", rs["misfit_at"][:, n]), ("status", rs["status_at"][:, n]),
                    ("trace", rs["trace"][:, :n + 1])):
        a = getattr(fit, name)
        assert a.shape == b.shape, (what, name)
        same = np.array_equal(a, b, equal_nan=(a.dtype != np.int32))
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a.ravel()[:4], b.ravel()[:4])
        assert same, (what, name)


def corrupt_receiver(p, sc, ir, rng, factor=20.0):
    """noise `factor` x its signal on every reference trace of receiver ir (1-based)"""
    for k in range(1, len(sc.comps[ir - 1]) + 1):
        lo, d = sc.refs[(ir, k)]
        sc.refs[(ir, k)] = (lo, (d + factor * np.std(d) * rng.standard_normal(len(d))).astype(np.float32))
        p.set_ref_seismogram(ir, k, *sc.refs[(ir, k)])


def tensors_of(coef, rows, K=6):
    """sum_i x_i T_i per group: the tensor a combination of K tensors at one place stands for"""
    return (coef[:, :, None] * rows.reshape(len(coef), K, 11)[:, :, 4:10].astype(np.float64)).sum(1)


# ------------------------------------------------------------------------------------------------ device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 7), (2, 1), (2, 7), (6, 1), (6, 7), (8, 1), (8, 7)])
def test_device_equals_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS)                                      # receivers of 1, 2, 3, 4, 5 and 3 components
    try:
        p.switch_receiver(6, False)                           # a disabled receiver
        enabled = [True] * 5 + [False]
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # a zero weight; the weight of the disabled receiver never counts
        rows = scattered_groups(np.random.default_rng(100 * K + ngroup), ngroup, K)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        syn, ref, receivers = device_traces(p, sc.comps, enabled, 0, ngroup, K)
        for mode in ("A", "B"):
            p.set_misfit_method(METHOD[mode])
            for anarchy in (False, True):
                rs = rr.fit(syn, ref, receivers, sc.gf["dt"], mode, w, anarchy, 8, EPS)
                for n in (0, 1, 8):
                    fit = p.linear_fit_robust(0, ngroup, K, receiver_weights=w, anarchy=anarchy, niter=n, eps=EPS)
                    assert_answers(fit, rs, n, "mode %s K=%d ngroup=%d anarchy=%s niter=%d" % (mode, K, ngroup, anarchy, n))
                    assert np.all(fit.status == 0) and np.all(np.isfinite(fit.coef)) and np.all(fit.misfit > 0)
                    ms = p.linear_fit_robust_ms()
                    assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
                obj = rs["trace"][:, :, 0]
                print("mode %s K=%d ngroup=%d anarchy=%s: objective %.6f -> %.6f, misfit %.6f -> %.6f" % (
                    mode, K, ngroup, anarchy, obj[0, 0], obj[0, -1], rs["trace"][0, 0, 1], rs["trace"][0, -1, 1]))
                slack = sum(s.shape[2] for s in syn) * (K + 2) * 2.0 ** -52      # the round-off of the objective's own sum
                assert np.all(obj[:, 1:] <= obj[:, :-1] * (1.0 + slack))
            if ngroup == 7:                                   # without weights: ones
                assert_answers(p.linear_fit_robust(0, ngroup, K, niter=2, eps=EPS),
                               rr.fit(syn, ref, receivers, sc.gf["dt"], mode, None, False, 2, EPS), 2, "no weights, mode " + mode)
    finally:
        p.close()


@pytest.mark.parametrize("window", [100, 600])
def test_window_lengths_clamped_samples_and_a_corrupted_receiver(window):
    """fewer samples than threads, and several strides; references that are an exact combination of the basis on every
    receiver but one, so that almost every sample takes the max(|e|, a_r) clamp; the corrupted receiver drags the l2 tensor
    and not the robust one"""
    sc, p = build(COMPS, window=window)
    try:
        assert len(p.get_reference(3, 1, 2)[1]) == window
        corrupt_receiver(p, sc, 4, np.random.default_rng(window))
        ngroup, K = 3, 6
        rows = colocated_groups(np.random.default_rng(window + 1), ngroup)
        p.set_source_params("moment_tensor", rows)
        l2 = p.linear_fit(0, ngroup, K)
        err_l2 = np.max(np.abs(tensors_of(l2.coef, rows) - PLANTED) / np.abs(PLANTED))
        syn, ref, receivers = device_traces(p, sc.comps, [True] * 6, 0, ngroup, K)
        for mode, anarchy in (("A", False), ("B", True), ("A", True), ("B", False)):
            p.set_misfit_method(METHOD[mode])
            fit = p.linear_fit_robust(0, ngroup, K, anarchy=anarchy, niter=8, eps=EPS)
            assert_answers(fit, rr.fit(syn, ref, receivers, sc.gf["dt"], mode, None, anarchy, 8, EPS), 8, "window %d mode %s" % (window, mode))
            err = np.max(np.abs(tensors_of(fit.coef, rows) - PLANTED) / np.abs(PLANTED))
            print("window %d mode %s anarchy %s: largest relative tensor error %.3g (l2 fit %.3g)" % (window, mode, anarchy, err, err_l2))
            assert np.all(fit.status == 0) and err < err_l2
    finally:
        p.close()


def test_forwarding_gives_the_bits_of_linear_fit():
    sc, p = build(COMPS)
    try:
        rows = scattered_groups(np.random.default_rng(5), 4, 6)
        p.set_source_params("moment_tensor", rows)
        w = np.array([1.0, 0.5, 2.0, 1.0, 0.0, 1.0])
        for anarchy in (False, True):
            a = p.linear_fit(0, 4, 6, receiver_weights=w, anarchy=anarchy)
            b = p.linear_fit_robust(0, 4, 6, outer_norm="l2norm", receiver_weights=w, anarchy=anarchy, niter=3, eps=EPS)
            c = p.linear_fit_robust_params("moment_tensor", rows, 6, outer_norm="l2norm", receiver_weights=w, anarchy=anarchy, niter=3)
            for f in (b, c):
                assert np.array_equal(a.coef, f.coef) and np.array_equal(a.misfit, f.misfit) and np.array_equal(a.status, f.status)
                assert f.trace.shape == (4, 4, 2) and np.array_equal(f.trace[:, 0, 0], a.misfit) and np.array_equal(f.trace[:, 0, 1], a.misfit)
                assert np.all(np.isnan(f.trace[:, 1:]))
        # niter = 0 of the robust modes: the l2 coefficients, their l1 misfit
        b0 = p.linear_fit_robust(0, 4, 6, receiver_weights=w, niter=0, eps=EPS)
        assert np.array_equal(b0.coef, p.linear_fit(0, 4, 6, receiver_weights=w).coef) and np.array_equal(b0.trace[:, 0, 1], b0.misfit)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ however it is cut
def _clamped_condition(nbr, receivers, ref, dt, mode, anarchy, eps):
    """cond of the unit-diagonal reweighted normal matrix where every sample (mode A) or receiver (mode B) takes the clamp:
    the weights are then constants of the data: v_r / a_r (A), v_r / (eps n_r) (B)"""
    K, dt64 = 6, np.float64(np.float32(dt))
    G = np.zeros((K, K))
    for r, slots in enumerate(receivers):
        Gr, _, Rr = lr.full_matrix(nbr[r], K)
        if not slots or not Rr > 0:
            continue
        Dr = dt64 * sum(np.abs(np.asarray(ref[m], np.float64)).sum() for m in slots)
        T = sum(len(ref[m]) for m in slots)
        if mode == "A":
            u = (1.0 / Dr if anarchy else 1.0) / (eps * np.sqrt(Rr / (dt64 * T)))
        else:
            u = (1.0 / np.sqrt(Rr) if anarchy else 1.0) / (eps * np.sqrt(Rr))
        G += u * Gr
    s = 1.0 / np.sqrt(np.diag(G))
    return np.linalg.cond(G * s[:, None] * s[None, :])


def assert_same_robust_fit(a, b, cond, what=""):
    """two device fits of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.
    fused: the kept traces agree within SYN_RTOL of their maximum (tests/common.py same_bits).  The data lie inside the span of
    the basis on every receiver (colocated_groups), so every residual stays under the clamp, the reweighted system is a
    least-squares problem with weights that are constants of the data, and a relative perturbation of the traces moves its
    solution by at most cond times it, as in tests/test_linfit_gpu.py assert_same_fit: 64 cond SYN_RTOL max|coef|."""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("coef", "misfit", "trace"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    for g in range(len(a.coef)):
        assert np.max(np.abs(a.coef[g] - b.coef[g])) <= 64 * cond[g] * SYN_RTOL * np.max(np.abs(a.coef[g])), (what, g)


@pytest.mark.parametrize("mode", ["A", "B"])
def test_first_source_chunks_pieces_and_contexts(mode, monkeypatch):
    ngroup, K, niter, anarchy = 40, 6, 3, True
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    kw = dict(anarchy=anarchy, niter=niter, eps=EPS)
    sc, p = build(COMPS)
    try:
        p.set_misfit_method(METHOD[mode])
        p.set_source_params("moment_tensor", rows)
        base = p.linear_fit_robust(0, ngroup, K, **kw)
        assert np.all(base.status == 0)
        assert np.all(np.abs(tensors_of(base.coef, rows) - PLANTED) <= 1e-5 * np.abs(PLANTED))
        syn, ref, receivers = device_traces(p, sc.comps, [True] * 6, 0, ngroup, K)
        assert_answers(base, rr.fit(syn, ref, receivers, sc.gf["dt"], mode, None, anarchy, niter, EPS), niter, "base")
        nbr = lr.gram_by_receiver(syn, ref, receivers, sc.gf["dt"])
        cond = [_clamped_condition(nbr[g], receivers, ref, sc.gf["dt"], mode, anarchy, EPS) for g in range(ngroup)]
        # isrc0 > 0, not a multiple of K, and against the restatement there
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        shifted = p.linear_fit_robust(5, ngroup, K, **kw)
        syn, ref, receivers = device_traces(p, sc.comps, [True] * 6, 5, ngroup, K)
        assert_answers(shifted, rr.fit(syn, ref, receivers, sc.gf["dt"], mode, None, anarchy, niter, EPS), niter, "isrc0 = 5")
        assert_same_robust_fit(base, shifted, cond, "isrc0 = 5")
        for piece in (K, 0, 13 * K + 2):
            assert_same_robust_fit(base, p.linear_fit_robust_params("moment_tensor", rows, K, piece=piece, **kw), cond, "piece %d" % piece)
            assert p.nsrc == (K if piece == K else (len(rows) if piece == 0 else 13 * K))
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks: read at kiwi_hip_init
    sc, q = build(COMPS)
    try:
        q.set_misfit_method(METHOD[mode])
        q.set_source_params("moment_tensor", rows)
        assert_same_robust_fit(base, q.linear_fit_robust(0, ngroup, K, **kw), cond, "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = build(COMPS, engine=multi_engine(2))              # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        m.set_misfit_method(METHOD[mode])
        assert_same_robust_fit(base, m.linear_fit_robust_params("moment_tensor", rows, K, **kw), cond, "two contexts")
        assert_same_robust_fit(base, m.linear_fit_robust_params("moment_tensor", rows, K, piece=2 * K, **kw), cond, "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("mode", ["A", "B"])
def test_fitted_tensor_evaluates_to_the_misfit_the_fit_reports(mode, monkeypatch):
    """the fitted tensor uploaded as an ordinary source, evaluated under the context's method, its per-slot results through
    make_global_misfits(outer_norm="l1norm").  Mode B takes a receiver's slots together (its l2 misfit over all components, as
    the Gram kernel sums them), so the per-slot results are combined per receiver first: make_global_misfits' l1 branch on the
    l2 per-receiver misfits."""
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        corrupt_receiver(p, sc, 2, np.random.default_rng(1), factor=3.0)
        p.set_misfit_method(METHOD[mode])
        row = mt_row(np.zeros(6))
        w = np.array([1.0, 1.0, 0.5, 2.0, 1.0, 1.5])
        for anarchy in (False, True):
            tensors, misfit, status, _ = mtfit.fit_moment_tensors(p, "moment_tensor", row, outer_norm="l1norm", receiver_weights=w,
                                                                  anarchy=anarchy, niter=8, eps=EPS)
            assert status[0] == 0 and p.nsrc == 6
            fitted = row.copy()
            fitted[4:10] = tensors[0]
            mis, nor, failings = p.make_misfits_for_sources("moment_tensor", fitted[None, :])
            assert not failings
            if mode == "B":
                mis, nor = np.sqrt((mis ** 2).sum(2, keepdims=True)), np.sqrt((nor ** 2).sum(2, keepdims=True))
            g, _ = kengine.make_global_misfits(mis, nor, outer_norm="l1norm", receiver_weights=w, anarchy=anarchy)
            print("mode %s anarchy %s: the fit reports %.9f, the evaluation of its tensor gives %.9f" % (mode, anarchy, misfit[0], g[0]))
            contract = common.arith()
            monkeypatch.setenv("KIWI_HIP_ARITH", "fused")     # the rule on the scale of the norm factors, for both contracts
            assert misfit_close(g[0], misfit[0], glob=True)
            monkeypatch.setenv("KIWI_HIP_ARITH", contract)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ degenerate groups, filter
def test_degenerate_groups_and_a_failed_basis_source():
    sc, p = build(COMPS)
    try:
        rows = scattered_groups(np.random.default_rng(3), 3, 2)
        rows[1, 4:10] = 0.0                                   # group 0: second basis source without moment: no l2 start
        rows[3] = rows[2]                                     # group 1: twice the same source: rank deficient
        # a basis source that fails to discretise ("Empty rupture area": above the constraining planes): mt_eikonal
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (4, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((4, 6)) * 1e18
        eik[3, 3] = 500.0
        for mode in ("A", "B"):
            p.set_misfit_method(METHOD[mode])
            fit = p.linear_fit_robust_params("moment_tensor", rows, 2, niter=4, eps=EPS)
            print("mode %s degenerate groups: status %s" % (mode, fit.status))
            assert fit.status[0] == 1 and np.all(np.isnan(fit.coef[0])) and np.isnan(fit.misfit[0]) and np.all(np.isnan(fit.trace[0]))
            assert fit.status[1] == 1 or (fit.status[1] == 3 and np.all(np.isfinite(fit.coef[1])) and np.isfinite(fit.misfit[1]))
            assert fit.status[2] == 0 and np.all(np.isfinite(fit.coef[2])) and np.all(np.isfinite(fit.trace[2]))
            fit = p.linear_fit_robust_params("mt_eikonal", eik, 2, niter=2, eps=EPS)
            assert fit.status[0] == 0 and np.all(np.isfinite(fit.coef[0])) and np.all(np.isfinite(fit.trace[0]))
            assert fit.status[1] == 2 and np.all(np.isnan(fit.coef[1])) and np.isnan(fit.misfit[1]) and np.all(np.isnan(fit.trace[1]))
    finally:
        p.close()


def test_with_a_misfit_filter(monkeypatch):
    monkeypatch.setenv("KIWI_HIP_FUSED_FFT", "0")             # library transforms throughout: get_reference(3) then is the
    sc, p = build(None, planted=False)                        # reference the fit compared with (it forces them for its call)
    try:
        for ir in range(1, sc.nrec + 1):
            p.set_misfit_filter(ir, *FILTER)
        basis = mtfit.elementary_params("moment_tensor", mt_row(np.zeros(6)), UNIT)
        for mode in ("A", "B"):
            p.set_misfit_method(METHOD[mode])
            p.set_source_params("moment_tensor", basis)
            fit = p.linear_fit_robust(0, 1, 6, niter=3, eps=EPS)
            assert fit.status[0] == 0
            syn, ref, receivers = device_traces(p, sc.comps, [True] * 6, 0, 1, 6, which=3)
            assert_answers(fit, rr.fit(syn, ref, receivers, sc.gf["dt"], mode, None, False, 3, EPS), 3, "filtered, mode " + mode)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.set_misfit_method("l2norm")
            p.set_source_params("moment_tensor", rows)
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)

        def refused(match, **kw):
            with pytest.raises(KiwiHipError, match=match):
                p.linear_fit_robust(0, 2, 6, **kw)
            with pytest.raises(KiwiHipError, match=match):
                p.linear_fit_robust_params("moment_tensor", rows, 6, **kw)
            p.set_source_params("moment_tensor", rows)        # (a failed list call leaves no batch the engine may index)

        for method in ("ampspec_l2norm", "ampspec_l1norm", "scalar_product", "peak"):
            p.set_misfit_method(method)
            refused("l2norm")
            refused("l2norm", outer_norm="l2norm")
        p.set_misfit_method("floating_l1norm")
        p.set_floating_shiftrange(1, -1.0, 1.0)
        refused("floating shift")
        p.set_misfit_method("l1norm")
        refused("no quadratic majoriser", outer_norm="l2norm")
        with pytest.raises(KiwiHipError, match="l2norm"):
            p.linear_fit(0, 2, 6)                             # the l2 fit still refuses l1norm
        for method in ("l1norm", "l2norm"):
            p.set_misfit_method(method)
            refused("niter", niter=-1)
            for eps in (0.0, -1e-3, float("nan"), float("inf")):
                refused("eps", eps=eps)
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_robust(0, 2, 6, outer_norm="l3norm")
        still_usable()
        out = dict(coef=np.zeros(64), misfit=np.zeros(8), status=np.zeros(8, np.int32))
        dp = lambda a: a.ctypes.data_as(c_double_p)           # noqa: E731
        for K in (0, 9, -1):
            rc = p.L.kiwi_hip_linear_fit_robust(p.h, 0, 1, K, 1, None, 0, 2, 1e-3, dp(out["coef"]), dp(out["misfit"]),
                                                out["status"].ctypes.data_as(c_int_p), None)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="basis sources per group"):
                p._ck(rc, "linear_fit_robust")
        rc = p.L.kiwi_hip_linear_fit_robust(p.h, 0, 1, 6, 3, None, 0, 2, 1e-3, dp(out["coef"]), dp(out["misfit"]),
                                            out["status"].ctypes.data_as(c_int_p), None)
        with pytest.raises(KiwiHipError, match="outer_norm"):
            p._ck(rc, "linear_fit_robust")
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            with pytest.raises(KiwiHipError, match="not inside the uploaded batch"):
                p.linear_fit_robust(isrc0, ngroup, 6)
        with pytest.raises(KiwiHipError, match="deviatoric"):
            mtfit.fit_moment_tensors(p, "moment_tensor", rows[:1], deviatoric=True, outer_norm="l1norm")
        still_usable()
        assert np.all(p.linear_fit_robust(0, 2, 6).status == 0)   # a trace may be left out at the C entry; here it is not
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
            p.linear_fit_robust(0, 2, 6)
        p.switch_receiver(2, False)
        assert np.all(p.linear_fit_robust(0, 2, 6).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ grid search and example
def test_grid_search_with_a_robust_tensor_per_node():
    true_row = mt_row(PLANTED, location=[0., 800., -400., 11000.])
    sc = Scenario(true_type=6, true_params=true_row)
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        corrupt_receiver(p, sc, 3, np.random.default_rng(2))
        values = [("north-shift", 800. + 400. * np.arange(-1, 2)), ("east-shift", -400. + 400. * np.arange(-1, 2)), ("depth", [10000., 11000., 12000.])]
        grid = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=values)
        grid.compute(p, linear_mt=True, outer_norm="l1norm", niter=8, eps=EPS)
        best = grid.best_source
        err = np.max(np.abs(best[4:10] - PLANTED) / np.abs(PLANTED))
        print("robust grid search: best node", best[:4], "misfit", grid.fit_misfits[grid.ibest], "largest relative tensor error %.3g" % err)
        assert np.array_equal(best[1:4], true_row[1:4]) and np.all(grid.fit_status == 0)
        plain = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=values)
        plain.compute(p, linear_mt=True)
        err_l2 = np.max(np.abs(plain.sources[grid.ibest, 4:10] - PLANTED) / np.abs(PLANTED))
        print("the l2 fit at that node: largest relative tensor error %.3g" % err_l2)
        assert err < err_l2
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_moment_tensor_robust.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "l1 fit" in out.stdout
