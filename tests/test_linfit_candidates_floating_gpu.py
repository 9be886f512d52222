"""kiwi_hip_linear_fit_candidates_floating on the device: the same BITS as the numpy restatement
(tests/linfit_candidates_floating_restatement.py) fed with sums the device gives by the brute route -- the references moved by every
shift of the range, `linear_fit(..., by_receiver=True)` each time --, which also pins the cross-correlation kernel to the Gram
kernel's bits; ranges (0, 0) against kiwi_hip_linear_fit_candidates; a mechanism grid against its syntheses under floating_l2norm;
the same bits however the call is cut; the refusals; the helper, the bootstrap and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.engine import bootstrap_draw_weights
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_floating_restatement as fr
from tests import linfit_restatement as lr
from tests.common import MISFIT_RTOL, misfit_close
from tests.linfit_candidates_floating_cases import RANGES_A, RANGES_B, assert_floating_bits, brute_sums, set_ranges, slack_of
from tests.linfit_cases import PLANTED, assert_beside_a_failed_piece, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_candidates_gpu import zero_reference
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ 1: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 7), (6, 1), (6, 7), (8, 1), (8, 7)])
def test_device_equals_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy at any shift
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # and one of weight 0; the weight of the disabled receiver never counts
        wz = np.where([True] * 5 + [False], w, 0.0)
        C, J, S = p.linear_fit_candidates_floating_shape(K)
        assert C == 256 and J == 4 and S == 32
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (4 * C + 3, K))
        cand[C - 1] = cand[2]                                 # equal misfits across a tile boundary: the lower index wins
        # the receivers that count are 1, 3, 5: ranges of 1, J and 33 shifts (longer than a stage) with anarchy off, of 2 (negative
        # only), J + 1 and 1 with anarchy on
        for anarchy, ranges in ((False, RANGES_A), (True, RANGES_B)):
            assert [hi - lo + 1 for lo, hi in RANGES_A] == [1, 2, J, J + 1, S + 1, 3]
            nbr, sb, sR = brute_sums(p, dt, ranges, ngroup, K)
            assert np.all(sR[3] == 0.0) and np.all(nbr[:, 5] == 0.0)
            p.set_misfit_method("floating_l2norm")
            set_ranges(p, dt, ranges)
            for norm in ("l1norm", "l2norm"):
                rs = fr.evaluate(nbr, sb, sR, [lo for lo, _ in ranges], wz, anarchy, cand, norm)
                for ncand in (1, C - 1, C, C + 1, 4 * C + 3):
                    scan = p.linear_fit_candidates_floating(0, ngroup, K, cand[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                            cand_shift=True, receiver_misfit=True)
                    assert_floating_bits(scan, rs, ncand, "K=%d ngroup=%d %s anarchy=%s ncand=%d" % (K, ngroup, norm, anarchy, ncand))
                assert np.all(scan.status == 0) and np.all(scan.best_index >= 0) and np.all(np.isfinite(scan.best_misfit))
                assert np.all(scan.receiver_misfit[:, :, [1, 3, 5]] == 0) and np.all(scan.receiver_norm[:, [1, 3, 5]] == 0)
                assert np.all(scan.cand_shift[:, :, [1, 3, 5]] == 0) and np.all(scan.best_shift[:, [1, 3, 5]] == 0)
                assert np.all(scan.receiver_norm[:, [0, 2, 4]] > 0)
                for r in (0, 2, 4):
                    assert np.all((scan.cand_shift[:, :, r] >= ranges[r][0]) & (scan.cand_shift[:, :, r] <= ranges[r][1]))
            ms = p.linear_fit_candidates_floating_ms()
            assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
            # the arrays that are not asked for are not made
            scan = p.linear_fit_candidates_floating(0, ngroup, K, cand[:3], misfit=False)
            assert scan.misfit is None and scan.cand_shift is None and scan.receiver_misfit is None and scan.receiver_norm is None
            assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3))
            p.set_floating_shiftrange(0, 0.0, 0.0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: every range (0, 0)
@pytest.mark.parametrize("anarchy", [False, True])
def test_ranges_of_one_shift_against_linear_fit_candidates(anarchy):
    """Outer l1norm: kiwi_hip_linear_fit_candidates under l2norm bit for bit.  Outer l2norm: the two calls form the same quantity
    m^2 = S / D, S = sum_r v_r^2 (R_r - 2 x.b_r + x.G_r.x), D = sum_r v_r^2 R_r, in two orders: the parent folds the rows
    (per entry nrec products and nrec additions) and evaluates the quadratic form once (an entry passes at most 2 K + 2 more
    roundings and the 2 closing additions); this call evaluates per receiver and folds the values (the same counts, the other way
    round).  Either way a term of S is off by at most (2 nrec + 2 K + 4) u of its size, u = 2^-53, and 2 nrec + 2 K + 4 <=
    nrec NN for these nrec = 6 and K = 6; with A = sum_r v_r^2 (R_r + 2 |x|.|b_r| + |x|.|G_r|.|x|) the two S differ by at most
    2 nrec NN u A.  The two D differ by at most (4 nrec + 6) u D (this call squares the root of R_r again) <= 2 nrec NN u D, which
    moves m^2 = S / D by at most that share of m^2 <= A / D.  The division and the root of either call add 4 u m^2.  On m^2:
    5 nrec NN u A / D -- the multiple is 5."""
    sc, p = build(COMPS)
    try:
        ngroup, K = 3, 6
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(31), ngroup, K))
        cand = np.random.default_rng(32).uniform(-2.0, 2.0, (300, K))
        kw = dict(receiver_weights=w, anarchy=anarchy, receiver_misfit=True)
        fit = p.linear_fit(0, ngroup, K, receiver_weights=w, anarchy=anarchy, by_receiver=True)
        l1 = p.linear_fit_candidates(0, ngroup, K, cand, outer_norm="l1norm", **kw)
        l2 = p.linear_fit_candidates(0, ngroup, K, cand, outer_norm="l2norm", **kw)
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(0, 0.0, 0.0)
        f1 = p.linear_fit_candidates_floating(0, ngroup, K, cand, outer_norm="l1norm", cand_shift=True, **kw)
        f2 = p.linear_fit_candidates_floating(0, ngroup, K, cand, outer_norm="l2norm", **kw)
        for name in ("misfit", "receiver_misfit", "receiver_norm", "best_index", "best_misfit", "status"):
            assert np.array_equal(getattr(f1, name), getattr(l1, name)), name
        assert np.all(f1.cand_shift == 0) and np.all(f1.best_shift == 0)
        nbr, NG, NN, nrec = fit.by_receiver, K * (K + 1) // 2, lr.nn_of(K), sc.nrec
        A, D = np.zeros((ngroup, len(cand))), np.zeros(ngroup)
        ax = np.abs(cand)
        for r in range(nrec):
            R = nbr[:, r, NN - 1]
            if w[r] == 0.0 or not np.all(R > 0):
                continue
            v2 = (w[r] ** 2 / R) if anarchy else np.full(ngroup, w[r] ** 2)
            size = R[:, None] + 2.0 * (ax[None] * np.abs(nbr[:, r, None, NG:NG + K])).sum(2)
            for i in range(K):
                for j in range(K):
                    size = size + ax[None, :, i] * np.abs(nbr[:, r, lr.tri(K, min(i, j), max(i, j))])[:, None] * ax[None, :, j]
            A += v2[:, None] * size
            D += v2 * R
        bound = 5 * nrec * NN * U * A / D[:, None]
        err = np.abs(f2.misfit ** 2 - l2.misfit ** 2)
        print("ranges (0, 0), outer l2norm against linear_fit_candidates: largest |difference of misfit^2| / bound %.3g" % np.max(err / bound))
        assert np.all(err <= bound)
        assert np.array_equal(f2.receiver_misfit, l2.receiver_misfit) and np.array_equal(f2.receiver_norm, l2.receiver_norm)
        assert np.array_equal(f2.status, l2.status)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: against syntheses
GRID_RANGES = [(-2, 2), (-3, 1), (-2, 4), (-1, 3), (-4, 4), (-2, 3)]       # 5 to 9 shifts


def test_a_mechanism_grid_against_its_syntheses_under_floating_l2norm(monkeypatch):
    """12 x 4 x 12 double couples at 30 degrees against `misfits_for_params` of the same rows under floating_l2norm on the same
    context.  The global misfit is formed as the evaluation forms it: sqrt(sum_r m_r^2) of the call's receiver misfits over
    sqrt(sum_k n_k^2) of the evaluation's per-SLOT norm factors (the call's own n_r is receiver-level).  Shifts against
    kiwi_hip_get_floating_shifts: equal except where the two smallest restated val_q of that (mechanism, receiver) differ, as
    roots, by less than MISFIT_RTOL max(m_r, n_r); at most 5 % of the pairs."""
    grid = (range(0, 360, 30), range(0, 91, 30), range(-180, 180, 30))
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt, nrec = sc.gf["dt"], sc.nrec
        for ir in range(nrec):                                # every station late or early by a few samples
            p.shift_ref_seismogram(ir + 1, [1, -2, 3, 0, -3, 2][ir] * dt)
        row = mt_row(np.zeros(6))
        p.set_misfit_method("floating_l2norm")
        set_ranges(p, dt, GRID_RANGES)
        res = mtfit.scan_double_couples_floating(p, "moment_tensor", row, *grid, moment=7e18, outer_norm="l2norm", cube=True, receiver_misfit=True)
        scan = res["scan"]
        assert p.nsrc == 6 and res["status"][0] == 0 and res["cube"].shape == (1, 12, 4, 12) and scan.misfit.shape == (1, 576)
        tensors, sdr = mtfit.double_couple_candidates(*grid, 7e18)
        rows = np.tile(row, (len(tensors), 1))
        rows[:, 4:10] = tensors.astype(np.float32)
        _, n, g, status = p.misfits_for_params("moment_tensor", rows)
        assert len(g) == 576 and not np.any(status) and p.nsrc == 576
        shifts = np.rint(p.get_floating_shifts() / dt).astype(int)                              # [576, nrec]
        predicted = np.sqrt((scan.receiver_misfit[0].astype(np.float64) ** 2).sum(1)) / np.sqrt((n[0].astype(np.float64) ** 2).sum())
        ibest = int(res["index"][0])
        print("576 double couples under floating_l2norm: worst |predicted - evaluated| %.3g; best predicted %.9f at (%g, %g, %g), evaluated "
              "there %.9f, evaluated minimum %.9f" % (np.max(np.abs(predicted - g)), predicted[ibest], res["strike"][0], res["dip"][0],
                                                      res["rake"][0], g[ibest], g.min()))
        contract = common.arith()
        monkeypatch.setenv("KIWI_HIP_ARITH", "fused")         # the rule on the scale of the norm factors, for both contracts
        assert misfit_close(g, predicted, glob=True)
        assert misfit_close(g[ibest], g.min(), glob=True)
        monkeypatch.setenv("KIWI_HIP_ARITH", contract)
        assert [res["strike"][0], res["dip"][0], res["rake"][0]] == list(sdr[ibest]) and res["moment"][0] == 7e18
        assert np.array_equal(res["shifts"][0], scan.cand_shift[0, ibest] * dt) and np.array_equal(scan.best_shift[0], scan.cand_shift[0, ibest])
        differ = np.argwhere(scan.cand_shift[0] != shifts)
        print("shifts: %d of %d (mechanism, receiver) pairs differ from the evaluation's" % (len(differ), shifts.size))
        assert len(differ) <= 0.05 * shifts.size
        if len(differ):
            p.set_source_params("moment_tensor", mtfit.elementary_params("moment_tensor", row))
            nbr, sb, sR = brute_sums(p, dt, GRID_RANGES, 1, 6)
            rs = fr.evaluate(nbr, sb, sR, [lo for lo, _ in GRID_RANGES], None, False, tensors / 1e18, "l2norm")
            for c, r in differ:
                x = [tensors[c:c + 1, i] / 1e18 for i in range(6)]
                _, xgx = fr.cr.quad(nbr[0, r], x, 6)
                vals = np.sort([max(float(sR[r][0, q] - 2.0 * sum(x[i][0] * sb[r][0, q, i] for i in range(6)) + xgx[0]), 0.0)
                                for q in range(sR[r].shape[1])])
                bound = MISFIT_RTOL * max(np.sqrt(vals[0]), float(rs["receiver_norm"][0, r]))
                assert np.sqrt(vals[1]) - np.sqrt(vals[0]) < bound, (c, r, scan.cand_shift[0, c, r], shifts[c, r], vals[:2], bound)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: the same bits however it is cut
def assert_same_floating(a, b, slack, what):
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("best_index", "best_misfit", "best_shift", "misfit", "cand_shift", "receiver_misfit", "receiver_norm"):
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
    kw = dict(outer_norm=norm, anarchy=anarchy, cand_shift=True, receiver_misfit=True)

    def floating(p, sc):
        p.set_misfit_method("floating_l2norm")
        set_ranges(p, sc.gf["dt"], RANGES_A)

    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        p.set_source_params("moment_tensor", rows)
        nbr, sb, sR = brute_sums(p, dt, RANGES_A, ngroup, K)
        floating(p, sc)
        base = p.linear_fit_candidates_floating(0, ngroup, K, cand, **kw)
        rs = fr.evaluate(nbr, sb, sR, [lo for lo, _ in RANGES_A], None, anarchy, cand, norm)
        assert_floating_bits(base, rs, 300, "base")
        slack = slack_of(nbr, rs, cand)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_floating(base, p.linear_fit_candidates_floating(5, ngroup, K, cand, **kw), slack, "isrc0 = 5")
        for piece in (1, 5):
            assert_same_floating(base, p.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, piece=piece, **kw), slack, "piece %d" % piece)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups and of candidate outputs: read at kiwi_hip_init
    sc, q = build(COMPS)
    try:
        floating(q, sc)
        q.set_source_params("moment_tensor", rows)
        assert_same_floating(base, q.linear_fit_candidates_floating(0, ngroup, K, cand, **kw), slack, "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = build(COMPS, engine=multi_engine(2))              # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        floating(m, sc)
        assert_same_floating(base, m.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, **kw), slack, "two contexts")
        assert_same_floating(base, m.linear_fit_candidates_floating_params("moment_tensor", rows, K, cand, piece=2 * K, **kw), slack, "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("floating_l2norm")
        set_ranges(p, dt, RANGES_A)
        before = p.linear_fit_candidates_floating(0, 2, 6, cand, cand_shift=True, receiver_misfit=True)

        def still_usable():
            after = p.linear_fit_candidates_floating(0, 2, 6, cand, cand_shift=True, receiver_misfit=True)
            for name in ("best_index", "best_misfit", "status", "best_shift", "misfit", "cand_shift", "receiver_misfit", "receiver_norm"):
                assert np.array_equal(getattr(before, name), getattr(after, name)), name

        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: a.ctypes.data_as(c_int_p)                                       # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, free=0, cshift=False, misfit=False, isrc0=0, ngroup=2, params_form=True):
            """both C entries with these arguments: refused, with the reason in a message that starts with the call's name"""
            import ctypes
            bi, bm, st, bs = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32), np.zeros(64, np.int32)
            mis = np.zeros(64) if misfit else None
            cs = np.zeros(512, np.int16).ctypes.data_as(ctypes.POINTER(ctypes.c_short)) if cshift else None
            x = np.ascontiguousarray(x, np.float64)
            tail = (ncand, dp(x), outer, None, 0, free, ip(bi), dp(bm), ip(st), ip(bs), dp(mis), cs, None, None)
            rc = p.L.kiwi_hip_linear_fit_candidates_floating(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*" + match):
                p._ck(rc, "linear_fit_candidates_floating")
            if params_form:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_linear_fit_candidates_floating_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*" + match):
                    p._ck(rc, "linear_fit_candidates_floating")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)
            still_usable()

        entry("at least one candidate", ncand=0)
        for bad in (np.nan, np.inf):
            x = cand.copy()
            x[3, 2] = bad
            entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        entry("outer_norm must be 1", outer=0)
        entry("free_scale is not offered", free=1)
        entry("free_scale is not offered", free=2, outer=1)
        entry("cand_shift array without a misfit array", cshift=True)
        for K in (0, 9):
            entry("basis sources per group", K=K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, params_form=False)
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_candidates_floating(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.linear_fit_candidates_floating(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="not defined under per-receiver shifts"):
            mtfit.scan_double_couples_floating(p, "moment_tensor", rows[0], [0.], [45.], [90.], moment=None)
        # the old refusals of the fits under floating_l2norm keep their text
        with pytest.raises(KiwiHipError, match="linear_fit: floating shift ranges make the misfit a minimum over shifts, which is not quadratic"):
            p.linear_fit(0, 2, 6)
        with pytest.raises(KiwiHipError, match="floating shift"):
            p.linear_fit_candidates(0, 2, 6, cand)
        still_usable()
        # the method: floating_l1norm by its name, everything else sent to floating_l2norm
        p.set_misfit_method("floating_l1norm")
        with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*floating_l1norm.*not quadratic"):
            p.linear_fit_candidates_floating(0, 2, 6, cand)
        for method in ("l2norm", "l1norm", "ampspec_l2norm"):
            p.set_misfit_method(method)
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*must be floating_l2norm"):
                p.linear_fit_candidates_floating(0, 2, 6, cand)
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*must be floating_l2norm"):
                p.linear_fit_candidates_floating_params("moment_tensor", rows, 6, cand)
            p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("floating_l2norm")
        still_usable()
    finally:
        p.close()
    # what linear_fit refuses about the set-up otherwise: an enabled receiver without a taper
    from tests.common import Scenario
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[2]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("floating_l2norm")
        with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating: .*has no misfit taper"):
            p.linear_fit_candidates_floating(0, 2, 6, cand)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: helper, bootstrap, example
def test_planted_double_couple_and_delays_through_the_helper_and_the_bootstrap():
    """data of a planted double couple, every station late by its own whole number of samples: the helper returns the planted
    mechanism and the delays; receiver_misfit and receiver_norm go through kiwi_hip_outer_misfits as they are"""
    sdr, moment = (40.0, 60.0, 100.0), 5e18
    planted = np.array(synthetic.mt_from_sdr(*sdr, moment), np.float32)
    from tests.common import Scenario
    sc = Scenario(comps_list=COMPS, true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    e.close()
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        dt, nrec = sc.gf["dt"], sc.nrec
        delays = [2, -1, 0, 3, -2, 1]
        for ir in range(nrec):
            p.shift_ref_seismogram(ir + 1, delays[ir] * dt)
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(0, -3 * dt, 3 * dt)
        grid = ([10., 40., 70.], [30., 60., 90.], [70., 100., 130.])
        for norm in ("l1norm", "l2norm"):
            res = mtfit.scan_double_couples_floating(p, "moment_tensor", mt_row(np.zeros(6)), *grid, moment=moment, outer_norm=norm,
                                                     cube=True, receiver_misfit=True)
            assert (res["strike"][0], res["dip"][0], res["rake"][0]) == sdr and res["status"][0] == 0 and res["moment"][0] == moment
            assert np.array_equal(res["shifts"][0], -np.array(delays) * dt)
            assert res["cube"].shape == (1, 3, 3, 3) and res["cube_shifts"].shape == (1, 3, 3, 3, nrec)
            assert res["misfit"][0] == res["cube"].min() and res["misfit"][0] < 1e-3
            # the bootstrap over the receivers through the existing call: one slot per receiver; draw 0 of ones is the call's own
            # misfit within the float32 rounding of m_r and n_r (2^-23 each, relative, on sums of like signs)
            scan = res["scan"]
            draws = np.concatenate([np.ones((1, nrec)), bootstrap_draw_weights(nrec, 20, np.random.default_rng(3))])
            bv, bi, g0 = p.outer_misfits_slots(scan.receiver_misfit[0], np.tile(scan.receiver_norm[0], (27, 1)), np.arange(nrec), nrec,
                                               outer_norm=norm, draw_weights=draws, which_draw=0)
            assert bi[0] == scan.best_index[0] and np.all(np.abs(g0 - scan.misfit[0]) <= 4 * 2.0 ** -23 * scan.misfit[0] + 1e-300)
            assert np.all(bi == scan.best_index[0])            # noise-free data: every draw finds the planted mechanism
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_station_shifts.py"), "--small"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism and delays found" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
@pytest.mark.parametrize("norm", ["l1norm", "l2norm"])
def test_a_piece_in_which_every_basis_source_fails_to_discretise(norm):
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(COMPS)
    try:
        p.set_misfit_method("floating_l2norm")
        set_ranges(p, sc.gf["dt"], RANGES_A)
        eik, good = eikonal_list_with_a_failed_piece(p)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        kw = dict(outer_norm=norm, cand_shift=True, receiver_misfit=True, piece=2)
        got = p.linear_fit_candidates_floating_params("mt_eikonal", eik, 2, cand, **kw)
        assert list(got.status) == [0, 2, 0]
        assert got.best_index[1] == -1 and np.isnan(got.best_misfit[1]) and np.all(np.isnan(got.misfit[1]))
        assert not np.any(got.best_shift[1]) and not np.any(got.cand_shift[1])
        assert not np.any(got.receiver_misfit[1]) and not np.any(got.receiver_norm[1])
        assert_beside_a_failed_piece(got, p.linear_fit_candidates_floating_params("mt_eikonal", good, 2, cand, **kw), common.arith(), norm)
    finally:
        p.close()
