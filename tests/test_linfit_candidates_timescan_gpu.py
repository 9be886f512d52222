"""kiwi_hip_linear_fit_candidates_time_scan on the device.  The yardsticks are the parent's own calls: with nk = 1 at offset 0 the
call is kiwi_hip_linear_fit_candidates, and offset k is kiwi_hip_linear_fit_candidates on a context whose references and tapers are
moved by -k samples (route B of tests/linfit_timescan_cases.py); the folds over the offsets are pinned to the numpy restatement
(tests/linfit_candidates_timescan_restatement.py) fed with route B's sums, whatever the number of candidates against the kernel's
tile, the number of offsets and the number of receivers against its LDS stage; the same scan however the call is packed; a small
mechanism grid at five origin times against its syntheses; statuses and refusals; the helper, the grid and the example.
Comparison rule: the same bits under the `exact` arithmetic contract; under `fused` the two sides' synthetics may come from
different instantiations of the accumulate kernel, and tests/test_linfit_candidates_gpu.py assert_same_scan's slack and
tests/test_linfit_gpu.py assert_same_fit's bound apply (tests/linfit_candidates_timescan_cases.py assert_scan)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import gridsearch, lib as klib, mtfit
from kiwi_amd.engine import CandidateTimeScan
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_timescan_cases as cc
from tests import linfit_candidates_timescan_restatement as ctr
from tests import linfit_timescan_cases as lc
from tests.common import Scenario, misfit_close
from tests.linfit_cases import PLANTED, mt_row
from tests.test_linfit_candidates_gpu import zero_reference
from tests.test_linfit_gpu import FILTER, assert_same_fit, build, colocated_groups, multi_engine, scattered_groups
from tests.timescan_cases import OFFSETS, offsets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts
ALL = dict(misfit=True, receiver_misfit=True)


def scan_fit(scan):
    """the free tensors of a CandidateTimeScan in the shape tests/test_linfit_gpu.py assert_same_fit takes"""
    from kiwi_amd.engine import LinearFit
    n = scan.fit_status.size
    return LinearFit(scan.fit_coef.reshape(n, -1), scan.fit_misfit.reshape(n), scan.fit_status.reshape(n), None, None, None)


def assert_fit_equals(scan, want, what):
    """fit_coef, fit_misfit, fit_status against a ScanFit (or LinearFit over ngroup x nk groups) with its sums"""
    got, w = scan_fit(scan), lc.flat(want) if want.coef.ndim == 3 else want
    assert np.array_equal(got.status, w.status), what
    if common.arith() == "exact":
        assert np.array_equal(got.coef, w.coef, equal_nan=True) and np.array_equal(got.misfit, w.misfit, equal_nan=True), what
    else:
        assert_same_fit(type(w)(got.coef, got.misfit, got.status, w.pivot_min, w.normal, None), w, what)


# ------------------------------------------------------------------------------------------------ 1: nk = 1 at offset 0
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 7), (6, 1), (6, 7), (8, 1), (8, 7)])
def test_one_offset_at_zero_equals_linear_fit_candidates(K, ngroup):
    sc, p = lc.standard()
    try:
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        for anarchy in (False, True):
            fit = p.linear_fit(0, ngroup, K, receiver_weights=WEIGHTS, anarchy=anarchy, normal=True, by_receiver=True)
            for norm, free in cc.MODES:
                kw = dict(outer_norm=norm, receiver_weights=WEIGHTS, anarchy=anarchy, free_scale=free)
                parent = p.linear_fit_candidates(0, ngroup, K, cand, receiver_misfit=True, **kw)
                got = p.linear_fit_candidates_time_scan(0, ngroup, K, cand, 0, 1, 1, **kw, **ALL)
                what = "K=%d ngroup=%d %s anarchy=%s free=%s" % (K, ngroup, norm, anarchy, free)
                assert got.misfit.shape == (ngroup, 1, 300) and got.receiver_misfit.shape == (ngroup, 1, 300, sc.nrec)
                want = cc.from_parents([parent])
                cc.assert_scan(got, want, cc.slack_of(fit.by_receiver[:, None], WEIGHTS, cand, want["scale"] if free else None), what)
                assert np.all(got.status == 0) and np.all(got.best_offset == 0) and np.all(got.cand_offset == 0)
                assert np.array_equal(got.cand_misfit, got.misfit[:, 0]) and (got.best_scale is None) == (not free)
                if free:
                    rows = np.arange(ngroup)
                    assert np.array_equal(got.best_scale[:, 0], got.scale[rows, 0, got.best_index[:, 0]])
                    assert np.array_equal(got.cand_scale, got.scale[:, 0])
                assert_fit_equals(got, type(fit)(parent.fit_coef, parent.fit_misfit, fit.status, fit.pivot_min, fit.normal, None), what)
        ms = p.linear_fit_candidates_time_scan_ms()
        assert len(ms) == 5 and all(t > 0 for t in ms[:4]) and ms[4] >= 0
    finally:
        p.close()


_WIDE = {}


def wide_scenario():
    """one receiver more than an LDS stage of the candidate kernels, one component each; made once for the cases below"""
    if not _WIDE:
        S = 64
        sc = Scenario(nrec=S + 1, comps_list=["d"] * (S + 1), true_type=6, true_params=mt_row(PLANTED))
        sc.make_references(sc.oracle())
        _WIDE["sc"] = sc
    return _WIDE["sc"]


@pytest.mark.parametrize("K", [1, 6, 8])
def test_plain_call_and_one_offset_scan_share_their_bits_over_chunks(K, monkeypatch):
    """kiwi_hip_linear_fit_candidates is the nk = 1 case of the scan's kernels: both calls on ONE context whose workspace bound
    cuts 3 groups into 2 chunks or more, 65 receivers (a second LDS stage of one receiver) of which one is disabled and one has
    the weight 0, 257 candidates (a second tile of one live lane), traces of 256 samples, a basis source of group 1 that fails to
    discretise.  The arrays both calls make have the same bits (exact contract; fused: the module's rule)"""
    ngroup, ncand = 3, 257
    sc = wide_scenario()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # read when the context is made
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        C, S = p.linear_fit_candidates_time_scan_shape(K)
        assert ncand == C + 1 and sc.nrec == S + 1
        p.switch_receiver(3, False)
        rng = np.random.default_rng(700 + K)
        w = rng.uniform(0.5, 2.0, sc.nrec)
        w[10] = 0.0
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        rows = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32),
                       (ngroup * K, 1))
        rows[:, 13:19] = rng.standard_normal((ngroup * K, 6)) * 1e18
        rows[2 * K - 1, 3] = 500.0                            # "Empty rupture area": the last basis source of group 1
        cand = rng.uniform(-2.0, 2.0, (ncand, K))
        ok = np.array([True, False, True])
        for norm, free in cc.MODES:
            kw = dict(outer_norm=norm, receiver_weights=w, anarchy=True, free_scale=free)
            what = "K=%d %s free=%s" % (K, norm, free)
            p.kernel_ms()
            parent = p.linear_fit_candidates_params("mt_eikonal", rows, K, cand, receiver_misfit=True, **kw)
            chunks_plain = int(p.kernel_ms()[1][1])
            got = p.linear_fit_candidates_time_scan_params("mt_eikonal", rows, K, cand, 0, 1, 1, **kw, **ALL)
            chunks_scan = int(p.kernel_ms()[1][1])
            print(what, "chunks: plain", chunks_plain, "scan", chunks_scan)
            assert chunks_plain >= 2 and chunks_scan >= 2, what
            assert np.array_equal(parent.status, [0, 2, 0]) and np.array_equal(got.status, parent.status), what
            assert np.all(got.best_offset[ok] == 0) and got.best_offset[1] == -1, what
            assert np.all(parent.best_index[ok] >= 0) and parent.best_index[1] == -1 and np.isnan(parent.best_misfit[1]), what
            assert np.all(parent.receiver_norm[ok][:, S] > 0) and np.all(parent.receiver_misfit[..., [2, 10]] == 0), what
            assert (parent.scale is None) == (not free) and (got.scale is None) == (not free), what
            if common.arith() == "exact":
                pairs = [("best_index", got.best_index[:, 0]), ("best_misfit", got.best_misfit[:, 0]), ("status", got.status),
                         ("misfit", got.misfit[:, 0]), ("receiver_misfit", got.receiver_misfit[:, 0]), ("receiver_norm", got.receiver_norm)]
                if free:
                    pairs.append(("scale", got.scale[:, 0]))
                for name, a in pairs:
                    b = getattr(parent, name)
                    assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
                    assert np.array_equal(a, b, equal_nan=a.dtype != np.int32), (what, name)
            else:
                fit = p.linear_fit_params("mt_eikonal", rows, K, receiver_weights=w, anarchy=True, by_receiver=True)
                want = cc.from_parents([parent])
                cc.assert_scan(got, want, cc.slack_of(fit.by_receiver[:, None], w, cand, want["scale"] if free else None), what)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: route B
def test_references_and_tapers_moved_the_other_way():
    """basis sources with fractional centroid times and rise times of 0, 1 and 2 s in one batch; every offset against the parent's
    call on the moved context"""
    K, ngroup = 6, 3
    sc, p = lc.standard(planted=False)
    try:
        tabs, moments, rises = lc.scattered_tables(np.random.default_rng(17), ngroup, K)
        p.set_sources(tabs, moments, rises)
        cand = np.random.default_rng(18).uniform(-2.0, 2.0, (70, K))
        ks = offsets(*OFFSETS)

        def parents():
            fit = p.linear_fit(0, ngroup, K, receiver_weights=WEIGHTS, normal=True, by_receiver=True)
            return fit, [p.linear_fit_candidates(0, ngroup, K, cand, outer_norm=norm, receiver_weights=WEIGHTS, free_scale=free,
                                                 receiver_misfit=True) for norm, free in cc.MODES]

        per_k = lc.route_b(p, sc, ks, parents)
        nbr = np.stack([f.by_receiver for f, _ in per_k], 1)
        fits = p.linear_fit_time_scan(0, ngroup, K, *OFFSETS, receiver_weights=WEIGHTS, normal=True)
        for m, (norm, free) in enumerate(cc.MODES):
            got = p.linear_fit_candidates_time_scan(0, ngroup, K, cand, *OFFSETS, outer_norm=norm, receiver_weights=WEIGHTS, free_scale=free, **ALL)
            want = cc.from_parents([scans[m] for _, scans in per_k])
            cc.assert_scan(got, want, cc.slack_of(nbr, WEIGHTS, cand, want["scale"] if free else None), "route B %s free=%s" % (norm, free))
            assert np.all(got.status == 0) and np.any(got.misfit[:, 0] != got.misfit[:, -1]), "the offsets change the misfits"
            assert_fit_equals(got, fits, "route B, the free tensors")
            assert_fit_equals(got, lc.stacked([f for f, _ in per_k]), "route B, the free tensors of the moved contexts")
        print("route B: best misfit per offset of group 0", got.best_misfit[0], "best offset", got.best_offset)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: the restatement
def test_device_equals_restatement_fed_with_route_b_sums():
    """one disabled receiver, one receiver with zero references, one receiver of weight 0; equal candidates on either side of a
    tile boundary; no direction at all under free_scale; nk 1, 2, 9; ncand around the tile"""
    K, ngroup = 6, 2
    scan9 = (-4, 1, 9)
    sc, p = lc.standard()                                     # (receiver 6 disabled)
    try:
        zero_reference(p, sc, 4)
        C, S = p.linear_fit_candidates_time_scan_shape(K)
        assert C == 256 and S >= sc.nrec
        rng = np.random.default_rng(31)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C] = cand[C - 1] = cand[2]                       # equal misfits across a tile boundary: the lowest index wins
        directions = cand.copy()
        directions[0] = 0.0                                   # no direction at all: NaN at every offset, passed over
        wz = np.where([True] * 5 + [False], WEIGHTS, 0.0)
        for anarchy in (False, True):
            nbr, normal, fits = cc.route_b_sums(p, sc, offsets(*scan9), ngroup, K, WEIGHTS, anarchy)
            assert np.all(nbr[:, :, 3, -1] == 0.0) and np.all(nbr[:, :, 5] == 0.0) and all(np.all(f.status == 0) for f in fits)
            for norm, free in cc.MODES:
                x = directions if free else cand
                for nk in (1, 2, 9):
                    for ncand in (1, C - 1, C, C + 1, 2 * C + 3):
                        rs = ctr.evaluate(nbr[:, :nk], normal[:, :nk], wz, anarchy, x[:ncand], norm, free)
                        got = p.linear_fit_candidates_time_scan(0, ngroup, K, x[:ncand], scan9[0], scan9[1], nk, outer_norm=norm,
                                                                receiver_weights=WEIGHTS, anarchy=anarchy, free_scale=free, **ALL)
                        what = "%s free=%s anarchy=%s nk=%d ncand=%d" % (norm, free, anarchy, nk, ncand)
                        cc.assert_scan(got, rs, cc.slack_of(nbr[:, :nk], wz, x[:ncand], rs["scale"] if free else None), what)
                        assert_fit_equals(got, lc.stacked(fits[:nk]), what)
                        assert np.all(got.status == 0) and np.all(got.receiver_misfit[..., [1, 3, 5]] == 0) and np.all(got.receiver_norm[:, [1, 3, 5]] == 0)
                        if free and ncand > 1:
                            assert np.all(np.isnan(got.misfit[:, :, 0])) and np.all(got.cand_offset[:, 0] == -1) and np.all(got.best_index > 0)
                        if ncand > C and common.arith() == "exact":
                            assert np.all(got.best_index != C) and np.array_equal(got.misfit[..., C], got.misfit[..., 2])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: two LDS stages
def test_more_receivers_than_one_lds_stage():
    """S + 1 receivers of one component: the rows of every offset pass through the LDS in two stages, the second of one receiver"""
    c, s = ctypes.c_int(), ctypes.c_int()
    assert klib.load().kiwi_hip_linear_fit_candidates_time_scan_shape(6, ctypes.byref(c), ctypes.byref(s)) == 0
    S = s.value
    sc = Scenario(nrec=S + 1, comps_list=["d"] * (S + 1), true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        rng = np.random.default_rng(65)
        p.set_source_params("moment_tensor", scattered_groups(rng, 2, 6))
        w = rng.uniform(0.5, 2.0, S + 1)
        w[S - 1] = 0.0
        cand = rng.uniform(-2.0, 2.0, (70, 6))
        scan = (-2, 3, 2)
        nbr, normal, fits = cc.route_b_sums(p, sc, offsets(*scan), 2, 6, w, True)
        for norm, free in cc.MODES:
            rs = ctr.evaluate(nbr, normal, w, True, cand, norm, free)
            got = p.linear_fit_candidates_time_scan(0, 2, 6, cand, *scan, outer_norm=norm, receiver_weights=w, anarchy=True, free_scale=free, **ALL)
            cc.assert_scan(got, rs, cc.slack_of(nbr, w, cand, rs["scale"] if free else None), "%d receivers, %s free=%s" % (S + 1, norm, free))
            assert np.all(got.receiver_misfit[..., S] > 0) and np.all(got.receiver_misfit[..., S - 1] == 0)
        # the last receiver alone decides: only the second stage counts
        only = np.zeros(S + 1)
        only[S] = 1.0
        nbr, normal, fits = cc.route_b_sums(p, sc, offsets(*scan), 2, 6, only, False)
        rs = ctr.evaluate(nbr, normal, only, False, cand, "l1norm")
        got = p.linear_fit_candidates_time_scan(0, 2, 6, cand, *scan, receiver_weights=only, **ALL)
        cc.assert_scan(got, rs, cc.slack_of(nbr, only, cand), "last receiver")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 5: however it is packed
def test_first_source_pieces_chunks_and_contexts(monkeypatch):
    ngroup, K = lc.CHUNK_GROUPS, lc.CHUNK_K
    rows = lc.chunk_rows()
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = cc.pack_candidates()
    base, slack = {}, {}
    sc, p = lc.standard()
    try:
        p.set_source_params("moment_tensor", rows)
        nbr, normal, fits = cc.route_b_sums(p, sc, offsets(*lc.CHUNK_SCAN), ngroup, K, None, True)
        wz = np.where([True] * 5 + [False], 1.0, 0.0)
        for norm, free in cc.MODES:
            kw = dict(outer_norm=norm, anarchy=True, free_scale=free, **ALL)
            b = base[norm, free] = p.linear_fit_candidates_time_scan(0, ngroup, K, cand, *lc.CHUNK_SCAN, **kw)
            rs = ctr.evaluate(nbr, normal, wz, True, cand, norm, free)
            slack[norm, free] = cc.slack_of(nbr, wz, cand, rs["scale"] if free else None)
            cc.assert_scan(b, rs, slack[norm, free], "base %s free=%s" % (norm, free))
        as_dict = lambda s: {name: getattr(s, name) for name in s._fields}      # noqa: E731
        for (norm, free), b in base.items():
            kw = dict(outer_norm=norm, anarchy=True, free_scale=free, **ALL)
            p.set_source_params("moment_tensor", np.concatenate([head, rows]))
            cc.assert_scan(p.linear_fit_candidates_time_scan(5, ngroup, K, cand, *lc.CHUNK_SCAN, **kw), as_dict(b), slack[norm, free], "isrc0 = 5")
            for piece in (K, 3 * K):
                got = p.linear_fit_candidates_time_scan_params("moment_tensor", rows, K, cand, *lc.CHUNK_SCAN, piece=piece, **kw)
                cc.assert_scan(got, as_dict(b), slack[norm, free], "piece %d" % piece)
                assert_fit_equals(got, lc.stacked(fits), "piece %d" % piece)
                assert p.nsrc == piece
                p.eval()                                      # the engine holds the head of the list and knows how long it is
    finally:
        p.close()
    # several chunks: KIWI_HIP_CHUNK_MB is read when a context is made -- a process of its own
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_linfit_candidates_timescan_child_%d.npz" % os.getpid())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "linfit_candidates_timescan_cases.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, KIWI_HIP_CHUNK_MB="1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = dict(np.load(out))
    os.remove(out)
    for (norm, free), b in base.items():
        key = "%s_%d_" % (norm, free)
        assert z[key + "launches"][1] >= 2, z[key + "launches"]       # a chunk boundary between groups
        chunked = CandidateTimeScan(*[z.get(key + name) for name in CandidateTimeScan._fields])
        cc.assert_scan(chunked, as_dict(b), slack[norm, free], "chunks %s free=%s" % (norm, free))
        assert_fit_equals(chunked, lc.stacked(fits), "chunks")
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = lc.standard(engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        for (norm, free), b in base.items():
            kw = dict(outer_norm=norm, anarchy=True, free_scale=free, **ALL)
            for piece in (0, 2 * K):
                got = m2.linear_fit_candidates_time_scan_params("moment_tensor", rows, K, cand, *lc.CHUNK_SCAN, piece=piece, **kw)
                cc.assert_scan(got, as_dict(b), slack[norm, free], "two contexts, piece %d" % piece)
                assert_fit_equals(got, lc.stacked(fits), "two contexts, piece %d" % piece)
    finally:
        m2.close()


# ------------------------------------------------------------------------------------------------ 6: against syntheses
def test_a_mechanism_grid_at_five_origin_times_against_its_syntheses(monkeypatch):
    """12 x 4 x 12 double couples at 30 degrees x 5 origin times; the row's time is dyadic and its rise time of 0.5 s gives two
    centroids at -+ 0.125 s, so every centroid's time / dt and time + k dt are exact in fp32 (tests/timescan_cases.py
    exact_mt_rows) and a source moved by k dt has the scan's synthetic moved by k samples"""
    grid = (range(0, 360, 30), range(0, 91, 30), range(-180, 180, 30))
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt = sc.gf["dt"]
        row = mt_row(np.zeros(6), location=[0.75, 0., 0., 10000.], risetime=0.5)
        scan = (-2, 1, 5)
        res = mtfit.scan_double_couples_time_scan(p, "moment_tensor", row, *grid, *scan, moment=7e18, outer_norm="l2norm", cube=True)
        full = p.linear_fit_candidates_time_scan_params("moment_tensor", mtfit.elementary_params("moment_tensor", row), 6,
                                                        mtfit.double_couple_candidates(*grid, 7.0)[0], *scan, outer_norm="l2norm", misfit=True)
        assert p.nsrc == 6 and res["status"][0] == 0 and res["cube"].shape == (1, 12, 4, 12) and full.misfit.shape == (1, 5, 576)
        tensors, sdr = mtfit.double_couple_candidates(*grid, 7e18)
        rows = np.tile(row, (len(tensors), 1))
        rows[:, 4:10] = tensors.astype(np.float32)
        contract = common.arith()
        evaluated = []
        for j, k in enumerate(offsets(*scan)):
            moved = rows.copy()
            moved[:, 0] += np.float32(k * dt)
            _, _, g, status = p.misfits_for_params("moment_tensor", moved)
            assert not np.any(status)
            evaluated.append(g)
            print("offset %+d: worst |predicted - evaluated| %.3g, best predicted %.9f evaluated minimum %.9f" % (
                k, np.max(np.abs(full.misfit[0, j] - g)), full.best_misfit[0, j], g.min()))
            monkeypatch.setenv("KIWI_HIP_ARITH", "fused")     # the rule on the scale of the norm factors, for both contracts
            assert misfit_close(g, full.misfit[0, j], glob=True)
            assert misfit_close(g[full.best_index[0, j]], g.min(), glob=True)
            monkeypatch.setenv("KIWI_HIP_ARITH", contract)
        evaluated = np.stack(evaluated)                       # [nk, ncand]
        monkeypatch.setenv("KIWI_HIP_ARITH", "fused")
        assert misfit_close(evaluated.min(0), res["cube"].reshape(-1), glob=True)
        assert misfit_close(evaluated[res["offset"][0], res["index"][0]], evaluated.min(), glob=True)
        monkeypatch.setenv("KIWI_HIP_ARITH", contract)
        assert [res["strike"][0], res["dip"][0], res["rake"][0]] == list(sdr[res["index"][0]]) and res["moment"][0] == 7e18
        assert np.all(res["tensor_misfit"][0] <= res["misfits"][0]) and np.array_equal(res["misfits"][0], full.best_misfit[0])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7: statuses and refusals
def test_statuses():
    sc, p = build(None, planted=False)
    try:
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_source_params("moment_tensor", colocated_groups(np.random.default_rng(4), 2))
        for norm, free in cc.MODES:                           # no receiver counts: status 1 whatever the offset
            got = p.linear_fit_candidates_time_scan(0, 2, 6, cand, *OFFSETS, outer_norm=norm, receiver_weights=np.zeros(6), free_scale=free, **ALL)
            assert np.all(got.status == 1) and np.all(got.best_offset == -1) and np.all(got.best_index == -1) and np.all(got.cand_offset == -1)
            assert np.all(np.isnan(got.misfit)) and np.all(np.isnan(got.best_misfit)) and np.all(np.isnan(got.cand_misfit))
            assert np.all(got.receiver_misfit == 0) and np.all(got.receiver_norm == 0)
        # the arrays that are not asked for are not made
        got = p.linear_fit_candidates_time_scan(0, 2, 6, cand, *OFFSETS, marginal=False)
        for name in ("best_scale", "cand_misfit", "cand_offset", "cand_scale", "misfit", "scale", "receiver_misfit", "receiver_norm"):
            assert getattr(got, name) is None, name
        assert got.best_index.shape == got.best_misfit.shape == got.fit_misfit.shape == got.fit_status.shape == (2, 6) and got.fit_coef.shape == (2, 6, 6)
        assert np.all(got.status == 0) and np.all((got.best_index >= 0) & (got.best_index < 5)) and np.all((got.best_offset >= 0) & (got.best_offset < 6))
        # a basis source that fails to discretise ("Empty rupture area": above the constraining planes): status 2
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (4, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((4, 6)) * 1e18
        eik[3, 3] = 500.0
        for piece in (0, 2):
            if piece == 2:
                eik[2, 3] = 500.0                             # a piece in which nothing could be discretised: nothing is uploaded for it
            for norm, free in cc.MODES:
                got = p.linear_fit_candidates_time_scan_params("mt_eikonal", eik, 2, cand[:, :2], *OFFSETS, outer_norm=norm, free_scale=free,
                                                               piece=piece, **ALL)
                assert got.status[0] == 0 and got.best_offset[0] >= 0 and np.all(got.best_index[0] >= 0) and np.all(np.isfinite(got.misfit[0]))
                assert np.all(got.fit_status[0] == 0) and np.all(got.cand_offset[0] >= 0)
                assert got.status[1] == 2 and got.best_offset[1] == -1 and np.all(got.best_index[1] == -1) and np.all(got.cand_offset[1] == -1)
                assert np.all(np.isnan(got.best_misfit[1])) and np.all(np.isnan(got.misfit[1])) and np.all(np.isnan(got.cand_misfit[1]))
                assert np.all(got.fit_status[1] == 2) and np.all(np.isnan(got.fit_coef[1])) and np.all(np.isnan(got.fit_misfit[1]))
                assert np.all(got.receiver_misfit[1] == 0) and np.all(got.receiver_norm[1] == 0)
                if free:
                    assert np.all(np.isnan(got.best_scale[1])) and np.all(np.isnan(got.scale[1])) and np.all(np.isnan(got.cand_scale[1]))
    finally:
        p.close()


def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = lc.standard()
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        scan_before = p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2, misfit=True)

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)
            again = p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2, misfit=True)
            assert np.array_equal(again.misfit, scan_before.misfit) and np.array_equal(again.best_offset, scan_before.best_offset)

        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)               # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, free=0, scan=(0, 1, 2), isrc0=0, ngroup=2, listed=True, best_scale=False,
                  cand_misfit=False, cand_offset=False, cand_scale=False, scale=False):
            """both C entries with these arguments: refused, with the call's name in front and the reason in the message"""
            bo, bi, bm, st = np.zeros(8, np.int32), np.zeros(4096, np.int32), np.zeros(4096), np.zeros(8, np.int32)
            bs, cm, cs, sca = (np.zeros(8192) if on else None for on in (best_scale, cand_misfit, cand_scale, scale))
            co = np.zeros(64, np.int32) if cand_offset else None
            x = np.ascontiguousarray(x, np.float64)
            tail = (scan[0], scan[1], scan[2], ncand, dp(x), outer, None, 0, free, ip(bo), ip(bi), dp(bm), dp(bs), ip(st), dp(cm), ip(co),
                    dp(cs), None, dp(sca), None, None, None, None, None)
            rc = p.L.kiwi_hip_linear_fit_candidates_time_scan(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_time_scan: .*" + match):
                p._ck(rc, "linear_fit_candidates_time_scan")
            if listed:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_linear_fit_candidates_time_scan_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_time_scan: .*" + match):
                    p._ck(rc, "linear_fit_candidates_time_scan")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)

        # what check_candidates refuses
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
        # what this call adds
        entry("best_scale or cand_scale array without free_scale", best_scale=True)
        entry("best_scale or cand_scale array without free_scale", cand_misfit=True, cand_scale=True)
        entry("cand_offset array without cand_misfit", cand_offset=True)
        still_usable()
        # what linear_fit_time_scan refuses
        for K in (0, 9):
            entry("basis sources per group", K=K)
        entry("need at least one offset", scan=(0, 1, 0))
        entry("257 offsets; at most 256", scan=(-128, 1, 257))
        entry("kstep = 0", scan=(0, 0, 3))
        entry(r"offsets 1025 \.\. 1025 samples; the largest shift is 1024", scan=(1025, 1, 1))
        entry("the largest shift is 1024", scan=(-1025, 1, 2))
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, listed=False)
        still_usable()
        p.set_misfit_filter(2, *FILTER)
        entry("misfit filter")
        p.set_misfit_filter(2, [], [])
        still_usable()
        for method in ("l1norm", "ampspec_l2norm"):
            p.set_misfit_method(method)
            entry("l2norm")
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(1, -1.0, 1.0)
        entry("floating shift")
        p.set_misfit_method("l2norm")
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_candidates_time_scan(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.linear_fit_candidates_time_scan(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="needs outer_norm l2norm"):
            mtfit.scan_double_couples_time_scan(p, "moment_tensor", rows[0], [0.], [45.], [90.], 0, 1, 2, moment=None, outer_norm="l1norm")
        fit = p.linear_fit_candidates_time_scan(0, 2, 6, cand, -1024, 2048, 2)       # the largest shift either way
        assert fit.best_index.shape == (2, 2)
        still_usable()
    finally:
        p.close()
    # an enabled receiver without a taper, without references
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[2]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_time_scan: .*no misfit taper"):
            p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2)
        p.eval()
        assert np.all(p.get_misfits()[0] > 0)
        p.switch_receiver(2, False)                           # disabled: it does not matter any more
        assert np.all(p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2).status == 0)
    finally:
        p.close()
    sc = Scenario(true_type=6, true_params=mt_row(PLANTED))
    e = sc.oracle()
    sc.make_references(e)
    del sc.refs[(3, 2)]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_time_scan: .*needs a reference seismogram"):
            p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2)
        with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_time_scan: .*needs a reference seismogram"):
            p.linear_fit_candidates_time_scan_params("moment_tensor", rows, 6, cand, 0, 1, 2)
        p.set_source_params("moment_tensor", rows)
        p.switch_receiver(3, False)
        assert np.all(p.linear_fit_candidates_time_scan(0, 2, 6, cand, 0, 1, 2).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 8: the helper, the grid, the example
DC = (60.0, 60.0, -90.0, 3.0e18)
MECH = (range(0, 360, 30), range(0, 91, 30), range(-180, 180, 30))


def _planted_dc_later(depth=10000., shift=2):
    """(scenario, engine, dt) whose references are the double couple DC `shift` samples later than the rows the tests scan"""
    dt = Scenario().gf["dt"]
    tensor = mtfit.double_couple_candidates([DC[0]], [DC[1]], [DC[2]], DC[3])[0][0].astype(np.float32)
    sc = Scenario(true_type=6, true_params=mt_row(tensor, location=[shift * dt, 0., 0., depth]))
    e = sc.oracle()
    sc.make_references(e)
    p = sc.product()
    sc.apply_setup(p, False)
    return sc, p, dt


def test_planted_double_couple_at_a_planted_offset_through_the_helper():
    sc, p, dt = _planted_dc_later()
    try:
        rows = np.stack([mt_row(np.zeros(6)), mt_row(np.ones(6), location=[0., 800., -500., 11000.])])
        for norm, moment in (("l1norm", DC[3]), ("l2norm", DC[3]), ("l2norm", None)):
            res = mtfit.scan_double_couples_time_scan(p, "moment_tensor", rows, *MECH, -3, 1, 8, moment=moment, outer_norm=norm, cube=True)
            print(norm, moment, "best misfit per offset of row 0", res["misfits"][0], "found", res["strike"][0], res["dip"][0], res["rake"][0],
                  res["moment"][0], "offset", res["offset"][0])
            assert np.all(res["status"] == 0) and res["offset"][0] == 5           # offsets -3 .. 4: +2 is index 5
            found = mtfit.double_couple_candidates([res["strike"][0]], [res["dip"][0]], [res["rake"][0]], res["moment"][0])[0][0]
            planted = mtfit.double_couple_candidates(*[[v] for v in DC[:3]], DC[3])[0][0]
            assert np.all(np.abs(found - planted) <= 1e-4 * DC[3])                # (the mechanism or its auxiliary plane: the same tensor)
            assert res["misfit"][0] <= 1e-4 and np.all(np.delete(res["misfits"][0], 5) > 100 * res["misfit"][0])
            assert res["misfit"][1] > 10 * res["misfit"][0]
            assert res["cube"].shape == res["cube_offset"].shape == (2, 12, 4, 12)
            assert res["cube"][0].reshape(-1)[res["index"][0]] == res["misfit"][0] == np.nanmin(res["cube"][0])
            assert res["cube_offset"][0].reshape(-1)[res["index"][0]] == 5
            assert res["tensor"].shape == (2, 8, 6) and res["tensor_misfit"].shape == res["tensor_status"].shape == (2, 8)
            if norm == "l2norm":                              # no double couple fits better than the free tensor of its offset
                assert np.all(res["tensor_misfit"] <= res["misfits"] + 1e-12)
            assert ("cube_moments" in res) == (moment is None)
        # the bootstrap over mechanism and origin time jointly through the existing call: nk x ncand "sources", one slot per receiver
        res = mtfit.scan_double_couples_time_scan(p, "moment_tensor", rows[:1], *MECH, -3, 1, 8, moment=DC[3], outer_norm="l1norm", receiver_misfit=True)
        scan = res["scan"]
        nk, ncand, nrec = scan.receiver_misfit.shape[1:]
        m = scan.receiver_misfit[0].reshape(nk * ncand, nrec)[:, :, None]
        n = np.broadcast_to(scan.receiver_norm[0][None, :, None], m.shape)
        weights = np.random.default_rng(0).multinomial(nrec, np.full(nrec, 1.0 / nrec), size=20).astype(np.float64)
        _, winner, _ = p.outer_misfits(m, n, outer_norm="l1norm", draw_weights=weights, ncomponents=[1] * nrec)
        planted = mtfit.double_couple_candidates(*[[v] for v in DC[:3]], DC[3])[0][0]
        tensors = mtfit.double_couple_candidates(*MECH, DC[3])[0]
        assert np.all(winner // ncand == 5)                   # every draw finds the planted offset and the planted tensor (either plane)
        assert np.all(np.abs(tensors[winner % ncand] - planted[None, :]) <= 1e-4 * DC[3])
    finally:
        p.close()


def test_grid_search_over_depth_and_time_with_the_best_double_couple_per_node():
    sc, p, dt = _planted_dc_later(depth=11000.)
    try:
        times = dt * np.arange(-2, 5)
        axes = [("depth", [10000., 11000., 12000.]), ("time", times)]
        grid = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=axes)
        assert len(grid.sources) == 21
        grid.compute_dc_time_scan(p, *MECH, moment=DC[3], cube=True)
        best = grid.best_source
        print("grid: best node", best[:4], grid.dc_sdr[grid.ibest], "misfit", grid.dc_misfits[grid.ibest], "second best", np.sort(grid.dc_misfits)[1])
        assert grid.syntheses_saved == 576 * 21 - 6 * 3
        assert best[3] == 11000.0 and best[0] == np.float32(2 * dt)
        planted = mtfit.double_couple_candidates(*[[v] for v in DC[:3]], DC[3])[0][0]
        assert np.all(np.abs(best[4:10] - planted) <= 1e-4 * DC[3])
        assert np.all(grid.dc_status == 0) and grid.dc_misfits[grid.ibest] <= 1e-4
        assert np.sort(grid.dc_misfits)[1] > 100 * grid.dc_misfits[grid.ibest]
        assert grid.dc_cube.shape == (3, 12, 4, 12) and np.nanmin(grid.dc_cube[1]) == grid.dc_misfits[grid.ibest]
        # the best source evaluated like any source reproduces the scan's misfit (l2norm outside: the engine's global misfit)
        l2 = gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=axes)
        l2.compute_dc_time_scan(p, *MECH, outer_norm="l2norm")                    # the best moment of every mechanism on the way
        assert l2.ibest == grid.ibest and abs(abs(l2.dc_moments[l2.ibest]) - DC[3]) <= 1e-4 * DC[3]
        _, _, g, _ = p.misfits_for_params("moment_tensor", l2.sources[[l2.ibest, 0]])
        assert abs(g[0] - l2.dc_misfits[l2.ibest]) <= 1e-5 and abs(g[1] - l2.dc_misfits[0]) <= 1e-5 * np.sqrt(g[1] ** 2 + 1)
        with pytest.raises(ValueError, match="exactly one `time` axis"):
            gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("depth", [10000.])]).compute_dc_time_scan(p, *MECH)
        with pytest.raises(ValueError, match="not evenly spaced by a whole number of samples"):
            gridsearch.MisfitGrid("moment_tensor", mt_row(np.full(6, 1e18)), param_values=[("time", [0.0, 0.3 * dt])]).compute_dc_time_scan(p, *MECH)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith(), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_timescan.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted node found" in out.stdout and "syntheses saved" in out.stdout, out.stdout
