"""kiwi_hip_linear_fit_wide on the device: the same BITS as kiwi_hip_linear_fit for K <= 8, and as the numpy restatement
(tests/linfit_wide_restatement.py) fed with the device's own kept traces for every K up to 64 -- one tile, two tiles, ragged
tiles, the maximum --, with free and with non-negative coefficients, with and without a penalty, whatever the number of groups,
the receivers' components, the weights, the window length, the first source, the chunking, the pieces and the kind of context;
the evaluation it leaves behind; the degenerate groups; the refusals; the slip inversion helper and its example."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import slipfit
from kiwi_amd.lib import KiwiHipError, c_double_p, c_int_p
from tests import common
from tests import linfit_restatement as lr
from tests import linfit_wide_restatement as lw
from tests.common import Scenario, same_bits
from tests.linfit_cases import PLANTED, device_traces, mt_row
from tests.test_linfit_gpu import build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPS = ["d", "ne", "ned", "ned", "ne", "d"]                # receivers of 1, 2 and 3 components
ENABLED = [True] * 5 + [False]                              # the last one is disabled in every case below
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # a zero weight; the weight of the disabled receiver never counts
FIELDS = ("coef", "misfit", "status", "pivot_min", "normal", "by_receiver", "npositive", "nsolves")


def assert_bits(fit, rs, what="", fields=FIELDS):
    for name in fields:
        a, b = getattr(fit, name), rs[name]
        assert a.shape == b.shape, (what, name)
        same = np.array_equal(a, b, equal_nan=(a.dtype != np.int32))
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a.ravel()[:4], b.ravel()[:4])
        assert same, (what, name)


def restate(p, sc, isrc0, ngroup, K, weights=None, anarchy=False, enabled=ENABLED, **kw):
    syn, ref, receivers = device_traces(p, sc.comps, enabled, isrc0, ngroup, K, 2)
    return lw.fit(syn, ref, receivers, sc.gf["dt"], weights, anarchy, **kw)


def assert_same_fit(a, b, what=""):
    """two device fits of the same groups through different chunkings / pieces / contexts: the same bits under the exact
    contract.  fused: a kernel instantiation contracts its multiply-adds on its own and the batch shape chooses the
    instantiation, so the kept traces agree within SYN_RTOL of their maximum (tests/common.py same_bits); the normal matrix
    is a sum of products of two traces: within 3 SYN_RTOL of the geometric mean of its diagonal elements"""
    assert a.normal.shape == b.normal.shape, what
    if common.arith() == "exact":
        for name in ("coef", "misfit", "status", "pivot_min", "normal", "npositive", "nsolves"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    K = a.coef.shape[1]
    for g in range(len(a.coef)):
        Ga, ba, Ra = lr.full_matrix(a.normal[g], K)
        Gb, bb, Rb = lr.full_matrix(b.normal[g], K)
        scale = np.sqrt(np.outer(np.diag(Ga), np.diag(Ga)))
        assert np.all(np.abs(Ga - Gb) <= 3 * 64 * common.SYN_RTOL * scale), (what, g)
        assert np.all(np.abs(ba - bb) <= 3 * 64 * common.SYN_RTOL * np.sqrt(np.diag(Ga) * Ra)), (what, g)


# ------------------------------------------------------------------------------------------------ K <= 8: the narrow fit's bits
@pytest.mark.parametrize("K", [1, 6, 8])
def test_same_bits_as_the_narrow_fit(K):
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(K), 5, K))
        for anarchy in (False, True):
            a = p.linear_fit(0, 5, K, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True, by_receiver=True)
            b = p.linear_fit_wide(0, 5, K, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True, by_receiver=True)
            for name in ("coef", "misfit", "status", "pivot_min", "normal", "by_receiver"):
                assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (K, anarchy, name)
            assert np.all(b.status == 0) and np.all(b.nsolves == 1) and np.array_equal(b.npositive, (b.coef > 0).sum(1))
        ms, wide_ms = p.linear_fit_ms(), p.linear_fit_wide_ms()
        assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0
        assert len(wide_ms) == 2 and wide_ms[0] > 0 and wide_ms[1] > 0 and wide_ms[0] + wide_ms[1] <= ms[1] * 1.001 + 1e-3
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ device == restatement, free
@pytest.mark.parametrize("K,ngroup,anarchy,window", [(9, 1, False, 100), (9, 3, True, 600), (16, 3, False, 600), (16, 1, True, 100),
                                                     (17, 1, True, 600), (17, 3, False, 100), (33, 3, True, 100), (33, 1, False, 600),
                                                     (64, 1, True, 100), (64, 3, False, 600)])
def test_device_equals_restatement_bit_for_bit(K, ngroup, anarchy, window):
    sc, p = build(COMPS, window=window)
    try:
        p.switch_receiver(6, False)
        assert len(p.get_reference(3, 1, 2)[1]) == window
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(100 * K + ngroup), ngroup, K))
        fit = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True, by_receiver=True)
        rs = restate(p, sc, 0, ngroup, K, WEIGHTS, anarchy)
        print("K=%d ngroup=%d window=%d: status %s smallest pivot %.3g" % (K, ngroup, window, fit.status, fit.pivot_min.min()))
        assert_bits(fit, rs, "K=%d ngroup=%d" % (K, ngroup))
        assert np.all(fit.by_receiver[:, 5] == 0.0) and np.all(fit.by_receiver[:, 1, -1] > 0.0)
        assert np.all(fit.nsolves == 1)
        assert np.all(np.isfinite(fit.coef[fit.status == 0])) and np.all(np.isnan(fit.coef[fit.status != 0]))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ device == restatement, nonneg
def test_nonneg_planted_combination_with_zeros():
    """K = 6 tensors at the planted source's place; the data are the combination x0 >= 0 of them, with zeros"""
    rng = np.random.default_rng(21)
    rows = colocated_groups(rng, 2)
    x0 = np.array([1.5, 0.0, 0.7, 0.0, 0.0, 2.0])
    planted = (x0[:, None] * rows[:6, 4:10].astype(np.float64)).sum(0).astype(np.float32)
    sc = Scenario(comps_list=COMPS, true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit_wide(0, 2, 6, receiver_weights=WEIGHTS, nonneg=True, normal=True, by_receiver=True)
        assert_bits(fit, restate(p, sc, 0, 2, 6, WEIGHTS, False, nonneg=True), "planted")
        print("planted %s: coef %s misfit %.3g npositive %d nsolves %d" % (x0, fit.coef[0], fit.misfit[0], fit.npositive[0], fit.nsolves[0]))
        assert fit.status[0] == 0 and np.all(fit.coef >= 0.0)
        # the fp32 pipeline leaves 1e-7 of the data as residual (tests/test_linfit.py): the zeros come back as zeros or as that
        assert np.all(np.abs(fit.coef[0] - x0) <= 1e-4 * x0.max()) and fit.misfit[0] <= 1e-5
        assert fit.status[1] == 0 and fit.misfit[1] >= fit.misfit[0]
    finally:
        p.close()


@pytest.mark.parametrize("K,relative", [(6, True), (17, True), (17, False), (64, True), (64, False)])
def test_nonneg_with_negative_free_coefficients_and_a_penalty(K, relative):
    shape = {6: (6, 1, 1, 1), 17: (17, 1, 1, 1), 64: (4, 4, 2, 2)}[K]           # (nx, ny, nrake, nwin) of the penalty
    ngroup = 2
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(7 * K), ngroup, K))
        free = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, normal=True, by_receiver=True)
        assert_bits(free, restate(p, sc, 0, ngroup, K, WEIGHTS), "free K=%d" % K)
        assert np.all(free.status == 0) and np.any(free.coef.min(1) < 0.0)
        # without a penalty
        rs = restate(p, sc, 0, ngroup, K, WEIGHTS, nonneg=True)
        fit = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, nonneg=True, normal=True, by_receiver=True)
        assert_bits(fit, rs, "nonneg K=%d" % K)
        print("K=%d nonneg: status %s npositive %s nsolves %s misfit %s (free %s)" % (K, fit.status, fit.npositive, fit.nsolves, fit.misfit, free.misfit))
        assert np.all(fit.status == 0) and np.all(fit.coef >= 0.0) and np.all(fit.misfit >= free.misfit)
        assert np.array_equal(fit.npositive, (fit.coef > 0).sum(1))
        if K >= 17:
            assert np.any(rs["nsolves"] > rs["npositive"])    # the removal branch ran
        # with a penalty: relative to the mean diagonal, or absolute of the same size
        P = 0.05 * slipfit.laplacian_penalty(*shape)
        if not relative:
            G, _, _ = lr.full_matrix(free.normal[0], K)
            P = P * (np.trace(G) / K)
        rs = restate(p, sc, 0, ngroup, K, WEIGHTS, nonneg=True, penalty=P, penalty_relative=relative)
        fit = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, nonneg=True, penalty=P, penalty_relative=relative, normal=True,
                                by_receiver=True)
        assert_bits(fit, rs, "nonneg penalty K=%d" % K)
        assert np.array_equal(fit.normal, free.normal)        # the sums are returned without the penalty
        # ... and with free coefficients
        rs = restate(p, sc, 0, ngroup, K, WEIGHTS, penalty=P, penalty_relative=relative)
        pen = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, penalty=P, penalty_relative=relative, normal=True, by_receiver=True)
        assert_bits(pen, rs, "free penalty K=%d" % K)
        assert np.all(pen.status == 0) and np.all(pen.misfit >= free.misfit) and np.all(pen.pivot_min >= free.pivot_min)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ degenerate groups
def test_degenerate_groups_and_a_failed_basis_source():
    K = 10
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)
        rows = scattered_groups(np.random.default_rng(5), 3, K)
        rows[3] = rows[1]                                     # group 0: twice the same source
        rows[K + 7, 4:10] = rows[K + 2, 4:10] + rows[K + 4, 4:10]   # group 1: a tensor that is the sum of two others at ...
        rows[K + 2, :4] = rows[K + 4, :4] = rows[K + 7, :4]         # ... the same place and time
        p.set_source_params("moment_tensor", rows)
        free = p.linear_fit_wide(0, 3, K, normal=True, by_receiver=True)
        assert_bits(free, restate(p, sc, 0, 3, K), "degenerate, free")
        print("degenerate groups, free: status", free.status, "pivot_min", free.pivot_min)
        assert free.status[0] == 1 and free.pivot_min[0] <= K * 2.0 ** -52 and np.all(np.isnan(free.coef[0])) and np.isnan(free.misfit[0])
        assert free.pivot_min[1] < 1e-9                       # (the tensor sum goes through fp32: dependent to 1e-7, not to 2^-52)
        assert free.status[2] == 0 and np.all(np.isfinite(free.coef[2]))
        syn, ref, receivers = device_traces(p, sc.comps, ENABLED, 0, 3, K, 2)
        rs = lw.fit(syn, ref, receivers, sc.gf["dt"], None, False, nonneg=True)
        fit = p.linear_fit_wide(0, 3, K, nonneg=True, normal=True, by_receiver=True)
        assert_bits(fit, rs, "degenerate, nonneg")
        barred = [lw.solve_one(rs["normal"][g], K, nonneg=True)["barred"] for g in range(3)]
        print("degenerate groups, nonneg: status", fit.status, "npositive", fit.npositive, "nsolves", fit.nsolves, "barred", barred)
        assert np.all(fit.status == 0) and np.all(fit.coef >= 0.0) and np.all(np.isfinite(fit.misfit))
        assert not (fit.coef[0, 1] > 0 and fit.coef[0, 3] > 0)        # of two identical sources at most one carries moment
        for g in range(3):                                    # a barred index stays at zero
            assert np.all(fit.coef[g, barred[g]] == 0.0)
        # a basis source that fails to discretise ("Empty rupture area": above the constraining planes): mt_eikonal
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (4, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((4, 6)) * 1e18
        eik[3, 3] = 500.0
        for nonneg in (False, True):
            fit = p.linear_fit_wide_params("mt_eikonal", eik, 2, nonneg=nonneg)
            assert fit.status[0] == 0 and np.all(np.isfinite(fit.coef[0]))
            assert fit.status[1] == 2 and np.all(np.isnan(fit.coef[1])) and np.isnan(fit.misfit[1])
            assert fit.npositive[1] == 0 and fit.nsolves[1] == 0
    finally:
        p.close()


def near_copies(rows, K, ngroup, ncopy=8):
    """the last `ncopy` sources of every group become the first ones with ONE tensor component moved by one fp32 ulp"""
    for g in range(ngroup):
        for i in range(ncopy):
            j = g * K + K - 1 - i
            rows[j] = rows[g * K + i]
            c = 4 + i % 6
            rows[j, c] = np.nextafter(rows[j, c], np.float32(np.inf if i % 2 else -np.inf))
    return rows


@pytest.mark.exact_only                                       # (which index is barred hangs on the last bits of the traces)
@pytest.mark.parametrize("K,seed", [(17, 305), (33, 305)])
def test_near_copies_are_barred_on_the_device(K, seed):
    """A source that differs from another one in the last bit of one tensor component has traces 6e-8 apart: a pivot of about
    1e-15, under K 2^-52 for K >= 17.  Its gradient, once its twin is passive, is (difference . residual): far above the
    threshold, of either sign, and the largest one left when everything else has converged.  Where it is positive the source
    enters, its pivot fails, and the index is barred: the pivot-failure branch of the device's active-set loop (take i* out
    of P, bar it, x_i* = 0, back to step 1), pinned by bit identity with the restatement, which says which indices it barred.
    With 8 such sources in each of 2 groups the restatement bars 3 (K = 17) and 4 (K = 33) of them on the oracle's traces"""
    ngroup = 2
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("moment_tensor", near_copies(scattered_groups(np.random.default_rng(seed), ngroup, K), K, ngroup))
        free = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, normal=True, by_receiver=True)
        assert_bits(free, restate(p, sc, 0, ngroup, K, WEIGHTS), "near copies, free")
        assert np.all(free.status == 1) and np.all(free.pivot_min <= K * 2.0 ** -52) and np.all(np.isnan(free.coef))
        rs = restate(p, sc, 0, ngroup, K, WEIGHTS, nonneg=True)
        fit = p.linear_fit_wide(0, ngroup, K, receiver_weights=WEIGHTS, nonneg=True, normal=True, by_receiver=True)
        assert_bits(fit, rs, "near copies, nonneg")
        ones = [lw.solve_one(rs["normal"][g], K, nonneg=True) for g in range(ngroup)]
        barred = [o["barred"] for o in ones]
        print("K=%d near copies: barred %s npositive %s nsolves %s" % (K, barred, fit.npositive, fit.nsolves))
        assert any(len(b) for b in barred)                    # the branch ran ...
        assert np.all(fit.status == 0) and np.all(fit.coef >= 0.0) and np.all(np.isfinite(fit.misfit))
        for g in range(ngroup):
            assert np.all(fit.coef[g, barred[g]] == 0.0)      # ... a barred index stays at zero ...
            assert fit.nsolves[g] >= fit.npositive[g] + len(barred[g])      # ... and cost one failed solve
            for i in barred[g]:                               # it is one of a pair whose other half is passive
                twin = K - 1 - i
                assert min(i, twin) < 8 and twin in ones[g]["passive"]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ the same bits however it is cut
def test_first_source_chunks_pieces_and_contexts(monkeypatch):
    ngroup, K = 6, 17
    rows = scattered_groups(np.random.default_rng(8), ngroup, K)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    P = 0.05 * slipfit.laplacian_penalty(K, 1)
    kw = dict(nonneg=True, penalty=P, penalty_relative=True, normal=True)
    sc, p = build(COMPS)
    try:
        p.set_source_params("moment_tensor", rows)
        base = p.linear_fit_wide(0, ngroup, K, **kw)
        assert np.all(base.status == 0) and np.any(base.nsolves > base.npositive)
        # isrc0 > 0, not a multiple of K, and against the restatement there
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        shifted = p.linear_fit_wide(5, ngroup, K, by_receiver=True, **kw)
        assert_bits(shifted, restate(p, sc, 5, ngroup, K, enabled=[True] * 6, nonneg=True, penalty=P, penalty_relative=True), "isrc0 = 5")
        assert_same_fit(base, shifted, "isrc0 = 5")
        for piece in (K, 0, 2 * K + 3):
            assert_same_fit(base, p.linear_fit_wide_params("moment_tensor", rows, K, piece=piece, **kw), "piece %d" % piece)
            assert p.nsrc == (K if piece == K else (len(rows) if piece == 0 else 2 * K))
            p.eval()                                          # the engine holds the head of the list and knows how long it is
    finally:
        p.close()
    # several chunks: KIWI_HIP_CHUNK_MB is read at kiwi_hip_init
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")
    sc, q = build(COMPS)
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_fit(base, q.linear_fit_wide(0, ngroup, K, **kw), "chunks")
        q.eval()
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
            assert_same_fit(base, m.linear_fit_wide_params("moment_tensor", rows, K, **kw), "ndev %d" % ndev)
            assert_same_fit(base, m.linear_fit_wide_params("moment_tensor", rows, K, piece=2 * K, **kw), "ndev %d pieces" % ndev)
        finally:
            m.close()


# ------------------------------------------------------------------------------------------------ what the call leaves behind
def test_misfits_of_the_basis_sources_are_those_of_an_evaluation():
    K = 17
    rows = scattered_groups(np.random.default_rng(2), 4, K)
    sc, p = build(COMPS)
    sc2, q = build(COMPS)
    try:
        p.set_source_params("moment_tensor", rows)
        p.linear_fit_wide(K, 3, K, nonneg=True)
        q.set_source_params("moment_tensor", rows)
        q.eval()
        a, b = p.get_misfits(K, 3 * K), q.get_misfits(K, 3 * K)
        for x, y in zip(a, b):
            assert same_bits(x, y)
        assert np.all(a[0] > 0)
        with pytest.raises(KiwiHipError):
            p.get_misfits(0, K)                               # sources outside the range were not evaluated
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    K = 12
    sc, p = build(COMPS)
    try:
        rows = scattered_groups(np.random.default_rng(4), 2, K)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.set_source_params("moment_tensor", rows)
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert same_bits(x, y)

        out = dict(coef=np.zeros(2 * 65), misfit=np.zeros(2), status=np.zeros(2, np.int32), pivot=np.zeros(2), npos=np.zeros(2, np.int32),
                   nsol=np.zeros(2, np.int32))
        dp = lambda a: a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: a.ctypes.data_as(c_int_p)              # noqa: E731

        def raw(K, nonneg=0, penalty=None):
            return p.L.kiwi_hip_linear_fit_wide(p.h, 0, 1, K, None, 0, nonneg, None if penalty is None else dp(penalty), 0, dp(out["coef"]),
                                                dp(out["misfit"]), ip(out["status"]), dp(out["pivot"]), ip(out["npos"]), ip(out["nsol"]),
                                                None, None)

        for bad in (0, 65, -1):
            rc = raw(bad)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="basis sources per group; 1 to 64"):
                p._ck(rc, "linear_fit_wide")
            with pytest.raises(KiwiHipError, match="basis sources per group; 1 to 64"):
                p.linear_fit_wide(0, 1, bad)
        with pytest.raises(KiwiHipError, match="basis sources per group; 1 to 64"):
            p.linear_fit_wide_params("moment_tensor", np.tile(rows[:1], (65, 1)), 65)
        rc = raw(K, nonneg=2)
        assert rc != 0
        with pytest.raises(KiwiHipError, match="nonneg = 2 must be 0 or 1"):
            p._ck(rc, "linear_fit_wide")
        with pytest.raises(KiwiHipError, match="must be 0 or 1"):
            p.linear_fit_wide(0, 2, K, nonneg=2)
        P = slipfit.laplacian_penalty(K, 1)
        for value in (np.nan, np.inf):
            P[7] = value
            with pytest.raises(KiwiHipError, match="penalty entry 7 is not finite"):
                p.linear_fit_wide(0, 2, K, penalty=P)
            with pytest.raises(KiwiHipError, match="penalty entry 7 is not finite"):
                p.linear_fit_wide_params("moment_tensor", rows, K, penalty=P)
        with pytest.raises(KiwiHipError, match="penalty must be"):
            p.linear_fit_wide(0, 2, K, penalty=np.zeros(5))
        still_usable()
        p.set_misfit_method("l1norm")
        with pytest.raises(KiwiHipError, match="l2norm"):
            p.linear_fit_wide(0, 2, K)
        with pytest.raises(KiwiHipError, match="l2norm"):
            p.linear_fit_wide_params("moment_tensor", rows, K, nonneg=True)
        p.set_misfit_method("l2norm")
        for isrc0, ngroup in ((0, 3), (K + 1, 1), (-1, 1)):
            with pytest.raises(KiwiHipError, match="not inside the uploaded batch"):
                p.linear_fit_wide(isrc0, ngroup, K)
        still_usable()
        assert np.all(p.linear_fit_wide(0, 2, K, nonneg=True).status == 0)
        assert np.all(p.linear_fit(0, 3, 8).status == 0)      # the narrow fit keeps its limit of 8 ...
        with pytest.raises(KiwiHipError, match="1 to 8 are supported"):
            p.linear_fit(0, 2, 9)                             # ... and its refusal
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
            p.linear_fit_wide(0, 2, K)
        p.eval()
        assert np.all(p.get_misfits()[0] > 0)
        p.switch_receiver(2, False)                           # disabled: it does not matter any more
        assert np.all(p.linear_fit_wide(0, 2, K).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ slip inversion and example
def _example():
    spec = importlib.util.spec_from_file_location("invert_slip", os.path.join(ROOT, "examples", "invert_slip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fit_slip_finds_both_planted_asperities():
    ex = _example()
    res = ex.main(verbose=False)
    planted = [a[:2] for a in ex.ASPERITIES]
    print("asperities found %s planted %s; misfit %.4f (free %.4f), %d positive of 64, %d solves; free minimum %.3g" % (
        res["asperities"], planted, res["misfit"], res["free_misfit"], res["npositive"], res["nsolves"], res["free"].min()))
    assert res["status"] == 0 and res["free_status"] == 0
    assert res["smooth"].shape == (ex.NY, ex.NX, 2, ex.NWIN) and np.all(res["smooth"] >= 0.0)
    assert res["asperities"] == [tuple(a) for a in planted]
    assert res["free"].min() < 0.0                            # the free, unsmoothed fit oscillates
    assert res["nsolves"] <= 3 * 64 and res["npositive"] == np.sum(res["smooth"] > 0)


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_slip.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "asperities found at" in out.stdout and "non-negative coefficients" in out.stdout
