"""kiwi_hip_linear_fit_candidates on the device: the same BITS as the numpy restatement
(tests/linfit_candidates_restatement.py) fed with the sums `linear_fit` returns on the same context, whatever K, the number of
groups, the outer norm, anarchy, the number of candidates against the kernel's tile and the number of receivers against its LDS
stage; the parent's kernels as yardsticks; the whole 12 960-mechanism grid against its syntheses; the same bits however the call
is cut; the refusals; the example."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import lib as klib, mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_restatement as cr
from tests import linfit_restatement as lr
from tests.common import SYN_RTOL, Scenario, misfit_close
from tests.linfit_cases import PLANTED, assert_beside_a_failed_piece, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (range(0, 360, 10), range(0, 91, 10), range(-180, 180, 10))


def assert_scan_bits(scan, rs, fit, ncand, free_scale, what):
    """every output of the call against the restatement's first ncand candidates (a candidate's results do not depend on the
    others; the best one is found again among them) and the free fit against `linear_fit`'s"""
    pairs = [("misfit", scan.misfit, rs["misfit"][:, :ncand]), ("receiver_misfit", scan.receiver_misfit, rs["receiver_misfit"][:, :ncand]),
             ("receiver_norm", scan.receiver_norm, rs["receiver_norm"]), ("status", scan.status, rs["status"]),
             ("fit_coef", scan.fit_coef, fit.coef), ("fit_misfit", scan.fit_misfit, fit.misfit)]
    if free_scale:
        pairs.append(("scale", scan.scale, rs["scale"][:, :ncand]))
    else:
        assert scan.scale is None
    best = [cr.first_minimum(row[:ncand]) for row in rs["misfit"]]
    pairs += [("best_index", scan.best_index, np.array([b[0] for b in best], np.int32)), ("best_misfit", scan.best_misfit, np.array([b[1] for b in best]))]
    for name, a, b in pairs:
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b, equal_nan=a.dtype != np.int32):
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
        assert np.array_equal(a, b, equal_nan=a.dtype != np.int32), (what, name)


def zero_reference(p, sc, ir):
    """receiver ir (1-based) with references of zeros: R_r = 0, skipped under l1norm and under anarchy"""
    for k in range(len(sc.comps[ir - 1])):
        lo, d = sc.refs[(ir, k + 1)]
        p.set_ref_seismogram(ir, k + 1, lo, np.zeros_like(d))


# ------------------------------------------------------------------------------------------------ 1: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 7), (6, 1), (6, 7), (8, 1), (8, 7)])
def test_device_equals_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS)
    try:
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # and one of weight 0; the weight of the disabled receiver never counts
        C, S = p.linear_fit_candidates_shape(K)
        assert C == 256 and S >= sc.nrec
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (4 * C + 3, K))
        cand[C - 1] = cand[2]                                 # equal misfits across a tile boundary: the lower index wins
        directions = cand.copy()
        directions[0] = 0.0                                   # no direction at all: NaN, passed over
        for anarchy in (False, True):
            fit = p.linear_fit(0, ngroup, K, receiver_weights=w, anarchy=anarchy, normal=True, by_receiver=True)
            assert np.all(fit.status == 0) and np.all(fit.by_receiver[:, 3, -1] == 0.0) and np.all(fit.by_receiver[:, 5] == 0.0)
            wz = np.where([True] * 5 + [False], w, 0.0)
            for norm, free, x in (("l1norm", False, cand), ("l2norm", False, cand), ("l2norm", True, directions)):
                rs = cr.evaluate(fit.by_receiver, fit.normal, wz, anarchy, x, norm, free)
                for ncand in (1, C - 1, C, C + 1, 4 * C + 3):
                    scan = p.linear_fit_candidates(0, ngroup, K, x[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                   free_scale=free, receiver_misfit=True)
                    assert_scan_bits(scan, rs, fit, ncand, free, "K=%d ngroup=%d %s anarchy=%s free=%s ncand=%d" % (K, ngroup, norm, anarchy, free, ncand))
                assert np.all(scan.status == 0) and np.all(scan.best_index >= 0) and np.all(np.isfinite(scan.best_misfit))
                assert np.all(scan.receiver_misfit[:, :, [1, 3, 5]] == 0) and np.all(scan.receiver_norm[:, [1, 3, 5]] == 0)
                assert np.all(scan.receiver_norm[:, [0, 2, 4]] > 0)
                if free:
                    assert np.all(np.isnan(scan.misfit[:, 0])) and np.all(np.isnan(scan.scale[:, 0])) and np.all(np.isnan(scan.receiver_misfit[:, 0, 0]))
            ms = p.linear_fit_candidates_ms()
            assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        # the arrays that are not asked for are not made
        scan = p.linear_fit_candidates(0, ngroup, K, cand[:3], misfit=False)
        assert scan.misfit is None and scan.receiver_misfit is None and scan.receiver_norm is None and scan.scale is None
        assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3))
    finally:
        p.close()


def test_more_receivers_than_one_lds_stage():
    """S + 1 receivers of one component: the rows of the sums pass through the LDS in two stages, the second of one receiver"""
    c, s = ctypes.c_int(), ctypes.c_int()
    assert klib.load().kiwi_hip_linear_fit_candidates_shape(6, ctypes.byref(c), ctypes.byref(s)) == 0
    S = s.value
    sc = Scenario(nrec=S + 1, comps_list=["d"] * (S + 1), true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        assert p.linear_fit_candidates_shape(6)[1] == S
        rng = np.random.default_rng(65)
        p.set_source_params("moment_tensor", scattered_groups(rng, 2, 6))
        w = rng.uniform(0.5, 2.0, S + 1)
        w[S - 1] = 0.0
        cand = rng.uniform(-2.0, 2.0, (70, 6))
        fit = p.linear_fit(0, 2, 6, receiver_weights=w, anarchy=True, normal=True, by_receiver=True)
        for norm in ("l1norm", "l2norm"):
            rs = cr.evaluate(fit.by_receiver, fit.normal, w, True, cand, norm)
            scan = p.linear_fit_candidates(0, 2, 6, cand, outer_norm=norm, receiver_weights=w, anarchy=True, receiver_misfit=True)
            assert_scan_bits(scan, rs, fit, 70, False, "%d receivers, %s" % (S + 1, norm))
            assert np.all(scan.receiver_misfit[:, :, S] > 0) and np.all(scan.receiver_misfit[:, :, S - 1] == 0)
        # the last receiver alone decides: only the second stage counts
        only = np.zeros(S + 1)
        only[S] = 1.0
        fit = p.linear_fit(0, 2, 6, receiver_weights=only, normal=True, by_receiver=True)
        rs = cr.evaluate(fit.by_receiver, fit.normal, only, False, cand, "l1norm")
        assert_scan_bits(p.linear_fit_candidates(0, 2, 6, cand, receiver_weights=only, receiver_misfit=True), rs, fit, 70, False, "last receiver")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: the parent's kernels
@pytest.mark.parametrize("anarchy", [False, True])
def test_the_fits_own_coefficients_give_the_parents_bits(anarchy):
    sc, p = build(COMPS)
    try:
        ngroup, K = 7, 6
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(21), ngroup, K))
        fit = p.linear_fit(0, ngroup, K, receiver_weights=w, anarchy=anarchy)
        robust = p.linear_fit_robust(0, ngroup, K, outer_norm="l1norm", receiver_weights=w, anarchy=anarchy, niter=0)
        assert np.all(fit.status == 0) and np.all(robust.status == 0)
        l2 = p.linear_fit_candidates(0, ngroup, K, fit.coef, outer_norm="l2norm", receiver_weights=w, anarchy=anarchy)
        l1 = p.linear_fit_candidates(0, ngroup, K, fit.coef, outer_norm="l1norm", receiver_weights=w, anarchy=anarchy)
        for g in range(ngroup):
            assert l2.misfit[g, g] == fit.misfit[g], g                 # linfit_solve_kernel's misfit
            assert l1.misfit[g, g] == robust.misfit[g], g              # robust_receiver_kernel's iterate 0
        assert np.array_equal(l2.best_index, np.arange(ngroup))        # nobody else's coefficients fit a group better than its own
        for scan in (l1, l2):
            assert np.array_equal(scan.fit_coef, fit.coef) and np.array_equal(scan.fit_misfit, fit.misfit)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: against syntheses
def test_the_whole_mechanism_grid_against_its_syntheses(monkeypatch):
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        row = mt_row(np.zeros(6))
        res = mtfit.scan_double_couples(p, "moment_tensor", row, *GRID, moment=7e18, outer_norm="l2norm", cube=True)
        assert p.nsrc == 6 and res["status"][0] == 0 and res["cube"].shape == (1, 36, 10, 36)
        predicted = res["cube"].reshape(-1)
        grid = synthetic.mt_sdr_grid(depth=float(row[3]), risetime=float(row[10]))
        _, _, g, status = p.misfits_for_params("moment_tensor", grid)
        assert len(g) == 12960 and not np.any(status)
        ibest = int(res["index"][0])
        print("12 960 double couples: worst |predicted - evaluated| %.3g; best predicted %.9f at (%g, %g, %g), evaluated there %.9f, evaluated minimum %.9f" % (
            np.max(np.abs(predicted - g)), res["misfit"][0], res["strike"][0], res["dip"][0], res["rake"][0], g[ibest], g.min()))
        contract = common.arith()
        monkeypatch.setenv("KIWI_HIP_ARITH", "fused")         # the rule on the scale of the norm factors, for both contracts
        assert misfit_close(g, predicted, glob=True)
        assert misfit_close(g[ibest], g.min(), glob=True)
        monkeypatch.setenv("KIWI_HIP_ARITH", contract)
        assert [res["strike"][0], res["dip"][0], res["rake"][0]] == list(mtfit.double_couple_candidates(*GRID)[1][ibest])
        assert res["moment"][0] == 7e18 and res["tensor_misfit"][0] <= res["misfit"][0]
        # the best moment of every mechanism on the way: never worse than the fixed one, never better than the free tensor
        free = mtfit.scan_double_couples(p, "moment_tensor", row, *GRID, outer_norm="l2norm", cube=True)
        assert np.all(free["cube"] <= res["cube"] * (1 + 1e-12)) and free["misfit"][0] >= free["tensor_misfit"][0]
        assert free["moments"].shape == (1, 36, 10, 36) and np.isfinite(free["moment"][0])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: the same bits however it is cut
def assert_same_scan(a, b, slack, what):
    """two scans of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.  fused: the
    batch shape chooses the accumulate kernel instantiation, so the kept traces agree within SYN_RTOL of their maximum, 64
    SYN_RTOL of their norm (assert_same_fit of tests/test_linfit_gpu.py); a candidate's misfit |sum_i x_i s_i - d| / |d| then moves
    by at most slack[g, c] = 64 SYN_RTOL sum_i |x_i| |s_i| / |d|, the largest such figure over the receivers that count"""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("best_index", "best_misfit", "misfit", "receiver_misfit", "receiver_norm", "fit_coef", "fit_misfit"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    assert np.all(np.abs(a.misfit - b.misfit) <= slack), what
    assert np.all(np.abs(a.best_misfit - b.best_misfit) <= slack.max(1)), what


@pytest.mark.parametrize("norm", ["l1norm", "l2norm"])
def test_first_source_chunks_pieces_and_contexts(norm, monkeypatch):
    ngroup, K, anarchy = 40, 6, True
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    kw = dict(outer_norm=norm, anarchy=anarchy, receiver_misfit=True)
    sc, p = build(COMPS)
    try:
        p.set_source_params("moment_tensor", rows)
        fit = p.linear_fit(0, ngroup, K, anarchy=anarchy, normal=True, by_receiver=True)
        base = p.linear_fit_candidates(0, ngroup, K, cand, **kw)
        assert_scan_bits(base, cr.evaluate(fit.by_receiver, fit.normal, None, anarchy, cand, norm), fit, 300, False, "base")
        NG, NN = K * (K + 1) // 2, lr.nn_of(K)
        diag = np.stack([fit.by_receiver[:, :, lr.tri(K, i, i)] for i in range(K)], 2)                      # [g, r, i]
        ratio = np.sqrt(diag / fit.by_receiver[:, :, NN - 1:NN])                                            # |s_i| / |d| per receiver
        slack = 64 * SYN_RTOL * np.max(np.abs(cand)[None, None, :, :] * ratio[:, :, None, :], axis=1).sum(2)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_scan(base, p.linear_fit_candidates(5, ngroup, K, cand, **kw), slack, "isrc0 = 5")
        for piece in (1, 5):
            assert_same_scan(base, p.linear_fit_candidates_params("moment_tensor", rows, K, cand, piece=piece, **kw), slack, "piece %d" % piece)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups and of candidate outputs: read at kiwi_hip_init
    sc, q = build(COMPS)
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_scan(base, q.linear_fit_candidates(0, ngroup, K, cand, **kw), slack, "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = build(COMPS, engine=multi_engine(2))              # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        assert_same_scan(base, m.linear_fit_candidates_params("moment_tensor", rows, K, cand, **kw), slack, "two contexts")
        assert_same_scan(base, m.linear_fit_candidates_params("moment_tensor", rows, K, cand, piece=2 * K, **kw), slack, "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_source_params("moment_tensor", rows)
        before = p.linear_fit(0, 2, 6, normal=True)

        def still_usable():
            after = p.linear_fit(0, 2, 6, normal=True)
            for name in ("coef", "misfit", "status", "pivot_min", "normal"):
                assert np.array_equal(getattr(before, name), getattr(after, name)), name

        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: a.ctypes.data_as(c_int_p)                                       # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, free=0, scale=False, isrc0=0, ngroup=2, params_form=True):
            """both C entries with these arguments: refused, with the reason in the message"""
            bi, bm, st = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32)
            sca = np.zeros(64) if scale else None
            x = np.ascontiguousarray(x, np.float64)
            tail = (ncand, dp(x), outer, None, 0, free, ip(bi), dp(bm), ip(st), None, dp(sca), None, None, None, None)
            rc = p.L.kiwi_hip_linear_fit_candidates(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match=match):
                p._ck(rc, "linear_fit_candidates")
            if params_form:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_linear_fit_candidates_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match=match):
                    p._ck(rc, "linear_fit_candidates")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)
            still_usable()

        entry("at least one candidate", ncand=0)
        entry("at least one candidate", ncand=-3)
        for bad in (np.nan, np.inf):
            x = cand.copy()
            x[3, 2] = bad
            entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        entry("outer_norm must be 1", outer=0)
        entry("free_scale = 2 must be 0 or 1", free=2)
        entry("free_scale needs the outer l2norm", outer=1, free=1)
        entry("scale array without free_scale", scale=True)
        for K in (0, 9):
            entry("basis sources per group", K=K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, params_form=False)
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_candidates(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.linear_fit_candidates(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="needs outer_norm l2norm"):
            mtfit.scan_double_couples(p, "moment_tensor", rows[0], [0.], [45.], [90.], moment=None, outer_norm="l1norm")
        # what linear_fit refuses about the set-up
        for method in ("l1norm", "ampspec_l2norm"):
            p.set_misfit_method(method)
            with pytest.raises(KiwiHipError, match="l2norm"):
                p.linear_fit_candidates(0, 2, 6, cand)
            with pytest.raises(KiwiHipError, match="l2norm"):
                p.linear_fit_candidates_params("moment_tensor", rows, 6, cand)
            p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(1, -1.0, 1.0)
        with pytest.raises(KiwiHipError, match="floating shift"):
            p.linear_fit_candidates(0, 2, 6, cand)
        p.set_misfit_method("l2norm")
        still_usable()
        assert np.all(p.linear_fit_candidates(0, 2, 6, cand).status == 0)
        # a basis source that fails to discretise ("Empty rupture area": above the constraining planes): status 2
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (4, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((4, 6)) * 1e18
        eik[3, 3] = 500.0
        for norm in ("l1norm", "l2norm"):
            scan = p.linear_fit_candidates_params("mt_eikonal", eik, 2, cand[:, :2], outer_norm=norm, receiver_misfit=True)
            assert scan.status[0] == 0 and scan.best_index[0] >= 0 and np.all(np.isfinite(scan.misfit[0]))
            assert scan.status[1] == 2 and scan.best_index[1] == -1 and np.isnan(scan.best_misfit[1]) and np.all(np.isnan(scan.misfit[1]))
            assert np.all(np.isnan(scan.fit_coef[1])) and np.all(scan.receiver_misfit[1] == 0) and np.all(scan.receiver_norm[1] == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: the example
def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism found" in out.stdout and "syntheses saved" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
@pytest.mark.parametrize("norm", ["l1norm", "l2norm"])
def test_a_piece_in_which_every_basis_source_fails_to_discretise(norm):
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(COMPS)
    try:
        eik, good = eikonal_list_with_a_failed_piece(p)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        kw = dict(outer_norm=norm, receiver_misfit=True, piece=2)
        got = p.linear_fit_candidates_params("mt_eikonal", eik, 2, cand, **kw)
        assert list(got.status) == [0, 2, 0]
        assert got.best_index[1] == -1 and np.isnan(got.best_misfit[1]) and np.all(np.isnan(got.misfit[1]))
        assert np.all(np.isnan(got.fit_coef[1])) and not np.any(got.receiver_misfit[1]) and not np.any(got.receiver_norm[1])
        assert_beside_a_failed_piece(got, p.linear_fit_candidates_params("mt_eikonal", good, 2, cand, **kw), common.arith(), norm)
    finally:
        p.close()
