"""kiwi_hip_spectral_candidates on the device: the candidate kernels have the same BITS as the numpy restatement
(tests/spectral_candidates_restatement.py) fed with the device's own spectra, whatever K, the number of groups, the method, the
outer norm, anarchy and the number of candidates against the kernel's tile; unit candidates against the basis sources' own
misfits; the fold against kiwi_hip_outer_misfits; a 576-mechanism grid against its syntheses; the same bits however the call is
cut; the refusals; the helper, the example and the bootstrap."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import spectral_candidates_restatement as sr
from tests.common import FFT_ROUNDOFF_C, MISFIT_RTOL, SYN_RTOL, Scenario, fft_roundoff_bound
from tests.linfit_cases import UNIT, assert_beside_a_failed_piece, device_traces, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {3: "ampspec_l2norm", 4: "ampspec_l1norm"}
CORNERS = (0.05, 0.1, 0.3, 0.4)                              # pass band, of Nyquist
GRID = (range(0, 360, 30), (0, 30, 60, 90), range(-180, 180, 30))      # 12 x 4 x 12 = 576 double couples


def band(dt):
    return [c * 0.5 / dt for c in CORNERS], [0., 1., 1., 0.]


def slot_map(sc, enabled):
    """the 0-based receiver of every slot of the enabled receivers"""
    return [ir for ir, c in enumerate(sc.comps) if enabled[ir] for _ in c]


def zero_reference(p, sc, ir):
    for k in range(len(sc.comps[ir - 1])):
        lo, d = sc.refs[(ir, k + 1)]
        p.set_ref_seismogram(ir, k + 1, lo, np.zeros_like(d))


def long_reference(p, sc, ir, n=600):
    """receiver ir (1-based) with its data followed by zeros up to n samples: its transforms are twice as long as the others'"""
    for k in range(len(sc.comps[ir - 1])):
        lo, d = sc.refs[(ir, k + 1)]
        p.set_ref_seismogram(ir, k + 1, lo, np.concatenate([d, np.zeros(n - len(d), np.float32)]))


def short_taper(p, sc, ir, n=100):
    """receiver ir (1-based) with a taper over n samples from 20 samples behind its first one: a window well below the others', so
    that most of its transform is the zero padding"""
    p.set_misfit_taper(ir, *synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, n, sc.gf["dt"], 10.0))


def refused_by_both_entries(p, rows, cand, match, K=6):
    """kiwi_hip_spectral_candidates on the uploaded sources and kiwi_hip_spectral_candidates_params on a list of the same shape, with
    plain arguments: both refused, with `match` behind the call's name"""
    dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
    bi, bm, st = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32)
    x = np.ascontiguousarray(cand, np.float64)
    tail = (len(x), dp(x), 2, None, 0, 0, bi.ctypes.data_as(c_int_p), dp(bm), st.ctypes.data_as(c_int_p), None, None, None, None, 0, None, None,
            None)
    p.set_source_params("moment_tensor", rows)
    rc = p.L.kiwi_hip_spectral_candidates(p.h, 0, len(rows) // K, K, *tail)
    assert rc != 0
    with pytest.raises(KiwiHipError, match="spectral_candidates: " + match):
        p._ck(rc, "spectral_candidates")
    basis = np.ascontiguousarray(rows, np.float32)
    rc = p.L.kiwi_hip_spectral_candidates_params(p.h, 6, len(rows) // K, K, basis.ctypes.data_as(c_float_p), 0, *tail)
    assert rc != 0
    with pytest.raises(KiwiHipError, match="spectral_candidates: " + match):
        p._ck(rc, "spectral_candidates")


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ok = np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if not ok:
        bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
        print(what, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])], len(bad), "of", a.size)
    assert ok, what


# ------------------------------------------------------------------------------------------------ 4: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_candidate_kernels_equal_the_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy,
        long_reference(p, sc, 5)                              # one whose transforms are longer
        short_taper(p, sc, 5)                                 # and whose window is shorter: 100 samples in a transform of 2048
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])          # and one of weight 0; the weight of the disabled receiver never counts
        wz = np.where([True] * 5 + [False], w, 0.0)
        enabled = [True] * 5 + [False]
        for ir in (1, 3, 5):                                  # a pass band on three of the six receivers
            p.set_misfit_filter(ir, *band(dt))
        has_filter = [ir in (0, 2, 4) for ir in slot_map(sc, enabled)]
        rec = slot_map(sc, enabled)
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))     # (a group's basis sources share place and time)
        C, B, nbins = p.spectral_candidates_shape(K)          # (the row length of the spectra follows the uploaded sources)
        assert C == 256 and B >= 1 and nbins >= 513
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C - 1] = cand[2]                                 # equal misfits across a tile boundary: the lower index wins
        cand[5] = -cand[4]                                    # and a candidate's opposite has its misfit
        for method in (3, 4):
            p.set_misfit_method(NAMES[method])
            full = p.spectral_candidates(0, ngroup, K, cand, outer_norm="l2norm", receiver_weights=w, slot_misfit=True, spectra=True)
            groups = sr.groups_from_scan(full, has_filter)
            lengths = set(int(sl["ntrans"]) for g in groups for sl in g)
            stages = max(sl["khi"] - sl["klo"] + 1 for g in groups for sl in g)
            assert len(lengths) == 2 and stages > B, (lengths, stages, B)      # two transform lengths; more bins than one stage
            assert any(sl["khi"] - sl["klo"] + 1 < sl["ntrans"] // 2 + 1 for sl in groups[0])      # the pass band skips bins
            cache = {}
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    rs = sr.evaluate(groups, rec, wz, anarchy, cand, method, norm, dt, cache=cache)
                    for ncand in (1, C - 1, C, C + 1, 2 * C + 3):
                        what = "K=%d ngroup=%d %s %s anarchy=%s ncand=%d" % (K, ngroup, NAMES[method], norm, anarchy, ncand)
                        scan = p.spectral_candidates(0, ngroup, K, cand[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                     slot_misfit=True, spectra=ncand == 1)
                        same(scan.misfit, rs["misfit"][:, :ncand], what + " misfit")
                        same(scan.slot_misfit, rs["slot_misfit"][:, :ncand], what + " slot_misfit")
                        same(scan.slot_norm, full.slot_norm, what + " slot_norm")
                        bi, bv = sr.best_of(rs["misfit"][:, :ncand])
                        same(scan.best_index, bi, what + " best_index")
                        same(scan.best_misfit, bv, what + " best_misfit")
                        same(scan.status, rs["status"], what + " status")
                        if ncand == 1:                        # the spectra do not depend on the candidates
                            same(scan.spectra, full.spectra, what + " spectra")
                            same(scan.spectra_range, full.spectra_range, what + " spectra_range")
                    assert np.all(scan.status == 0) and np.all(scan.best_index >= 0) and np.all(scan.misfit[:, 5] == scan.misfit[:, 4])
                    assert np.all(scan.slot_norm[:, [s for s, r in enumerate(rec) if r == 3]] == 0)
            if method == 3:                                   # the free scale: directions, one of them no direction at all
                directions = cand.copy()
                directions[0] = 0.0
                cache = {}
                for anarchy in (False, True):
                    rs = sr.evaluate(groups, rec, wz, anarchy, directions, 3, "l2norm", dt, free_scale=True, cache=cache)
                    for ncand in (1, C + 1, 2 * C + 3):
                        what = "K=%d ngroup=%d free scale anarchy=%s ncand=%d" % (K, ngroup, anarchy, ncand)
                        scan = p.spectral_candidates(0, ngroup, K, directions[:ncand], outer_norm="l2norm", receiver_weights=w, anarchy=anarchy,
                                                     free_scale=True)
                        same(scan.misfit, rs["misfit"][:, :ncand], what + " misfit")
                        same(scan.scale, rs["scale"][:, :ncand], what + " scale")
                        bi, bv = sr.best_of(rs["misfit"][:, :ncand])
                        same(scan.best_index, bi, what + " best_index")
                        same(scan.best_misfit, bv, what + " best_misfit")
                    assert np.all(np.isnan(scan.misfit[:, 0])) and np.all(np.isnan(scan.scale[:, 0])) and np.all(scan.best_index > 0)
            ms = p.spectral_candidates_ms()
            assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        # no receiver counts: status 1, NaN, no winner; the arrays that are not asked for are not made
        scan = p.spectral_candidates(0, ngroup, K, cand[:3], receiver_weights=np.zeros(6))
        assert np.all(scan.status == 1) and np.all(scan.best_index == -1) and np.all(np.isnan(scan.misfit))
        scan = p.spectral_candidates(0, ngroup, K, cand[:3], misfit=False)
        assert scan.misfit is None and scan.slot_misfit is None and scan.spectra is None and scan.scale is None
        assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 5: unit candidates
@pytest.mark.parametrize("method", [3, 4])
def test_unit_candidates_against_the_basis_sources_own_misfits(method):
    """x = e_a returns basis source a's own misfit: the amplitudes differ by at most one fp32 ulp (hardware root against rounded
    root), the sums by fp64 reordering, so |dm| <= 2^-23 sqrt(df sum_k (fw b_k)^2) + 2^-23 m under ampspec_l2norm and
    2^-23 df sum_k fw b_k + 2^-23 m under ampspec_l1norm -- which pins the spectra kernel to the plain path without any
    calibrated constant."""
    sc, p = build(COMPS)
    try:
        dt, K, ngroup = sc.gf["dt"], 6, 3
        for ir in (1, 3, 5):
            p.set_misfit_filter(ir, *band(dt))
        long_reference(p, sc, 5)
        short_taper(p, sc, 5)                                 # (the zero padding behind a short window, against the evaluation's own)
        has_filter = [ir in (0, 2, 4) for ir in slot_map(sc, [True] * 6)]
        p.set_misfit_method(NAMES[method])
        p.set_source_params("moment_tensor", colocated_groups(np.random.default_rng(3), ngroup, K))
        p.eval()
        m, n, g = p.get_misfits()
        scan = p.spectral_candidates(0, ngroup, K, np.eye(K), outer_norm="l2norm", slot_misfit=True, spectra=True)
        m2, n2, g2 = p.get_misfits()
        assert np.array_equal(m, m2) and np.array_equal(n, n2) and np.array_equal(g, g2)       # the evaluation it leaves is eval's
        groups = sr.groups_from_scan(scan, has_filter)
        worst = 0.0
        for gi in range(ngroup):
            assert np.array_equal(scan.slot_norm[gi], n[gi * K])
            for s, sl in enumerate(groups[gi]):
                df = float(sr.df_of(sl["ntrans"], dt))
                for a in range(K):
                    b = sr.amp_rn(sl["spectra"][:, a, 0], sl["spectra"][:, a, 1]).astype(np.float64)
                    if sl["has_filter"]:
                        b = b * sl["filtw"]
                    mine, theirs = float(scan.slot_misfit[gi, a, s]), float(m[gi * K + a, s])
                    bound = 2.0 ** -23 * (np.sqrt(df * np.sum(b * b)) if method == 3 else df * np.sum(b)) + 2.0 ** -23 * theirs
                    worst = max(worst, abs(mine - theirs) / bound)
                    assert abs(mine - theirs) <= bound, (gi, s, a, mine, theirs, bound)
        print("%s: unit candidates against get_misfits, largest |dm| / bound %.3g" % (NAMES[method], worst))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: the fold is outer_misfits'
@pytest.mark.parametrize("method", [3, 4])
def test_outer_fold_is_kiwi_hip_outer_misfits_on_the_calls_own_slots(method):
    sc, p = build(COMPS)
    try:
        dt, K, ngroup = sc.gf["dt"], 6, 2
        p.switch_receiver(6, False)
        zero_reference(p, sc, 4)
        p.set_misfit_filter(1, *band(dt))
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        rec = slot_map(sc, [True] * 5 + [False])
        p.set_misfit_method(NAMES[method])
        rng = np.random.default_rng(61)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                scan = p.spectral_candidates(0, ngroup, K, cand, outer_norm=norm, receiver_weights=w, anarchy=anarchy, slot_misfit=True)
                for g in range(ngroup):
                    bv, bi, gl = p.outer_misfits_slots(scan.slot_misfit[g], np.tile(scan.slot_norm[g], (len(cand), 1)), rec, sc.nrec,
                                                       outer_norm=norm, receiver_weights=w, anarchy=anarchy, which_draw=0)
                    same(scan.misfit[g], gl, "%s %s anarchy=%s group %d" % (NAMES[method], norm, anarchy, g))
                    assert scan.best_index[g] == bi[0] and scan.best_misfit[g] == bv[0]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7: against syntheses
def slot_bounds(name, dt, ntrans, wlen, n2_ref, n2_basis, cand, c):
    """test 2's round-off bound per (candidate, slot): the synthetic's norm is sum_a |x_a| n2(s_a), log2 N is log2 N + K + 1"""
    K = cand.shape[1]
    n2x = np.abs(cand) @ n2_basis.T                                   # [ncand, nmis]
    return fft_roundoff_bound(name, dt, ntrans[None, :] * 2.0 ** (K + 1), wlen[None, :], n2_ref[None, :], n2x, c=c)


def basis_scales(p, sc, enabled, scan, dt, K, ngroup=1):
    """(ntrans, window length, n2 of the tapered reference [nmis], n2 of the kept basis traces [ngroup, nmis, K])"""
    syn, ref, _ = device_traces(p, sc.comps, enabled, 0, ngroup, K, 2)
    n2 = lambda x: np.sqrt(dt * np.sum(np.asarray(x, np.float64) ** 2, axis=-1))       # noqa: E731
    return (scan.spectra_range[0, :, 2].astype(np.float64), np.array([float(len(r)) for r in ref]), np.array([n2(r) for r in ref]),
            np.stack([n2(s) for s in syn], axis=1))


@pytest.mark.parametrize("method", [3, 4])
@pytest.mark.parametrize("filtered", [False, True])
def test_the_mechanism_grid_against_its_syntheses(method, filtered):
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt, K, moment = sc.gf["dt"], 6, 7e18
        if filtered:
            for ir in range(1, sc.nrec + 1):
                p.set_misfit_filter(ir, *band(dt))
        p.set_misfit_method(NAMES[method])
        row = mt_row(np.zeros(6))
        cand, sdr = mtfit.double_couple_candidates(*GRID, moment / UNIT)
        scan = p.spectral_candidates_params("moment_tensor", mtfit.elementary_params("moment_tensor", row[None, :], UNIT), K, cand,
                                            outer_norm="l2norm", slot_misfit=True, spectra=True)
        assert p.nsrc == 6 and scan.status[0] == 0 and scan.slot_misfit.shape[:2] == (1, 576)
        nt, wl, na, nb = basis_scales(p, sc, [True] * 6, scan, dt, K)
        grid = np.array([mt_row(np.asarray(t * UNIT, np.float32), row[:4], row[10]) for t in cand], np.float32)
        m, n, g, status = p.misfits_for_params("moment_tensor", grid)
        assert len(g) == 576 and not np.any(status) and np.array_equal(n[0], scan.slot_norm[0])
        m, n = m.astype(np.float64), n.astype(np.float64)
        b1 = slot_bounds(NAMES[method], dt, nt, wl, na, nb[0], cand, 1.0)
        excess = np.abs(scan.slot_misfit[0].astype(np.float64) - m) - MISFIT_RTOL * np.maximum(m, n)
        ratio = float(np.max(excess / b1))
        # the global misfit of the outer l2norm, sqrt(sum m^2) / sqrt(sum n^2), moves by at most |bound| / |n|
        B = np.sqrt(np.sum((MISFIT_RTOL * np.maximum(m, n) + FFT_ROUNDOFF_C * b1) ** 2, axis=1)) / np.sqrt(np.sum(n * n, axis=1))
        ibest, imin = int(scan.best_index[0]), int(np.argmin(g))
        print("%s, filter %s: 576 double couples, largest excess over bound(c = 1) %.3g (limit %.2f); best predicted %.9f at (%g, %g, %g), "
              "evaluated there %.9f, evaluated minimum %.9f" % (NAMES[method], filtered, max(ratio, 0.0), FFT_ROUNDOFF_C, scan.best_misfit[0],
                                                               sdr[ibest, 0], sdr[ibest, 1], sdr[ibest, 2], g[ibest], g[imin]))
        assert np.all(excess <= FFT_ROUNDOFF_C * b1)
        assert np.all(np.abs(scan.misfit[0] - g) <= B)
        assert g[ibest] - g[imin] <= B[ibest] + B[imin]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 8: the same bits however it is cut
def assert_same_scan(a, b, slack, what, free=False):
    """two scans of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.  fused: the
    batch shape chooses the accumulate kernel instantiation, so the kept traces agree within SYN_RTOL of their maximum, 64 SYN_RTOL
    of their norm (assert_same_fit of tests/test_linfit_gpu.py); through the linear transform and the combination a slot misfit then
    moves by at most the round-off bound's expression with 64 SYN_RTOL in place of eps log2 N, and the global misfit of the outer
    l2norm by slack[g, c] = |those| / |n|.  With a free scale s the minimum over s moves by at most |s| times the slack of the
    direction (the value at the other scan's s bounds it from either side)."""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("best_index", "best_misfit", "misfit") + (("scale",) if free else ("slot_misfit", "slot_norm")):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    s = np.maximum(np.abs(a.scale), np.abs(b.scale)) if free else 1.0
    assert np.all(np.abs(a.misfit - b.misfit) <= s * slack), what
    assert np.all(np.abs(a.best_misfit - b.best_misfit) <= np.max(s * slack, axis=1)), what


@pytest.mark.parametrize("method,free", [(3, False), (4, False), (3, True)])
def test_first_source_chunks_pieces_and_contexts(method, free, monkeypatch):
    ngroup, K = 12, 6
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    kw = dict(outer_norm="l2norm", free_scale=free, slot_misfit=not free)

    def prepared(**more):
        sc, q = build(COMPS, **more)
        for ir in (1, 3, 5):
            q.set_misfit_filter(ir, *band(sc.gf["dt"]))
        q.set_misfit_method(NAMES[method])
        return sc, q

    sc, p = prepared()
    try:
        dt = sc.gf["dt"]
        p.set_source_params("moment_tensor", rows)
        base = p.spectral_candidates(0, ngroup, K, cand, spectra=True, **kw)
        assert np.all(base.status == 0)
        nt, wl, na, nb = basis_scales(p, sc, [True] * 6, base, dt, K, ngroup)
        slack = np.zeros((ngroup, len(cand)))
        for g in range(ngroup):
            # (ntrans 2^-K: log2 N + K + 1 = 1; c: 64 SYN_RTOL in place of eps; no reference term)
            per_slot = slot_bounds(NAMES[method], dt, np.full(len(nt), 2.0 ** -K), wl, 0.0 * na, nb[g], cand, 64 * SYN_RTOL * 2.0 ** 24)
            norms = p.get_misfits(g * K, 1)[1][0].astype(np.float64)
            slack[g] = np.sqrt(np.sum(per_slot ** 2, axis=1)) / np.sqrt(np.sum(norms * norms))
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_scan(base, p.spectral_candidates(5, ngroup, K, cand, **kw), slack, "isrc0 = 5", free)
        for piece in (1, 5):
            assert_same_scan(base, p.spectral_candidates_params("moment_tensor", rows, K, cand, piece=piece, **kw), slack, "piece %d" % piece, free)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups: read at kiwi_hip_init
    sc, q = prepared()
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_scan(base, q.spectral_candidates(0, ngroup, K, cand, **kw), slack, "chunks", free)
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = prepared(engine=multi_engine(2))                  # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        assert_same_scan(base, m.spectral_candidates_params("moment_tensor", rows, K, cand, **kw), slack, "two contexts", free)
        assert_same_scan(base, m.spectral_candidates_params("moment_tensor", rows, K, cand, piece=2 * K, **kw), slack, "two contexts, pieces", free)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable(monkeypatch):
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_misfit_method("ampspec_l2norm")
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.eval()
            for a, b in zip(before, p.get_misfits()):
                assert np.array_equal(a, b)

        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        fp = lambda a: None if a is None else a.ctypes.data_as(c_float_p)            # noqa: E731
        ip = lambda a: a.ctypes.data_as(c_int_p)                                       # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, free=0, scale=False, slots=False, isrc0=0, ngroup=2, params_form=True):
            """both C entries with these arguments: refused, with the reason in a message that starts with the call's name"""
            bi, bm, st = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32)
            sca = np.zeros(64) if scale else None
            sm, sn = (np.zeros(2 * 5 * 32, np.float32), np.zeros(2 * 32, np.float32)) if slots else (None, None)
            x = np.ascontiguousarray(x, np.float64)
            tail = (ncand, dp(x), outer, None, 0, free, ip(bi), dp(bm), ip(st), None, dp(sca), fp(sm), fp(sn), 0, None, None, None)
            rc = p.L.kiwi_hip_spectral_candidates(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="spectral_candidates: .*" + match):
                p._ck(rc, "spectral_candidates")
            if params_form:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_spectral_candidates_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="spectral_candidates: .*" + match):
                    p._ck(rc, "spectral_candidates")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)
            still_usable()

        entry("at least one candidate", ncand=0)
        entry("at least one candidate", ncand=-3)
        for bad in (np.nan, np.inf):
            x = cand.copy()
            x[3, 2] = bad
            entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        entry("free_scale = 2 must be 0 or 1", free=2)
        entry("free_scale needs ampspec_l2norm and the outer l2norm", outer=1, free=1)
        entry("free_scale together with slot_misfit", free=1, slots=True)
        entry("scale array without free_scale", scale=True)
        for K in (0, 9):
            entry("basis sources per group", K=K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, params_form=False)
        p.set_misfit_method("ampspec_l1norm")
        with pytest.raises(KiwiHipError, match="spectral_candidates: free_scale needs ampspec_l2norm"):
            p.spectral_candidates(0, 2, 6, cand, outer_norm="l2norm", free_scale=True)
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.spectral_candidates(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.spectral_candidates(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="needs outer_norm l2norm"):
            mtfit.scan_double_couples_spectral(p, "moment_tensor", rows[0], [0.], [45.], [90.], moment=None, outer_norm="l1norm")
        # a method other than 3 or 4
        for method in ("l2norm", "l1norm", "floating_l2norm"):
            p.set_misfit_method(method)
            with pytest.raises(KiwiHipError, match="spectral_candidates: the misfit method must be ampspec"):
                p.spectral_candidates(0, 2, 6, cand)
            with pytest.raises(KiwiHipError, match="spectral_candidates: the misfit method must be ampspec"):
                p.spectral_candidates_params("moment_tensor", rows, 6, cand)
            p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("ampspec_l2norm")
        still_usable()
        assert np.all(p.spectral_candidates(0, 2, 6, cand).status == 0)
        still_usable()
        # a transform length the in-LDS transforms do not take: a reference of 20000 samples asks for 65536; slot and length are named
        lo, d = sc.refs[(2, 2)]
        p.set_ref_seismogram(2, 2, lo, np.concatenate([d, np.zeros(20000 - len(d), np.float32)]))
        refused_by_both_entries(p, rows, cand, "slot 3 needs a transform of 65536 samples; 64 to 32768 are supported")
        p.set_ref_seismogram(2, 2, lo, d)
        p.set_source_params("moment_tensor", rows)
        still_usable()
        assert np.all(p.spectral_candidates(0, 2, 6, cand).status == 0)
    finally:
        p.close()
    # an enabled receiver component without a reference: the call's own message, in the list form too
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(np.array(synthetic.mt_from_sdr(40., 60., 100., 5e18), np.float32)))
    e = sc.oracle()
    sc.make_references(e)
    q = sc.product()
    try:
        for (ir, k), (lo, d) in sc.refs.items():
            if (ir, k) != (3, 2):
                q.set_ref_seismogram(ir, k, lo, d)
        for ir, (x, y) in sc.tapers.items():
            q.set_misfit_taper(ir, x, y)
        q.set_misfit_method("ampspec_l2norm")
        refused_by_both_entries(q, rows, cand, ".*needs a reference seismogram")
        q.set_ref_seismogram(3, 2, *sc.refs[(3, 2)])
        q.set_source_params("moment_tensor", rows)
        scan = q.spectral_candidates(0, 2, 6, cand)
        assert np.all(scan.status == 0) and np.all(np.isfinite(scan.misfit))
    finally:
        q.close()
    # an enabled receiver without a misfit taper; the library transforms
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(np.array(synthetic.mt_from_sdr(40., 60., 100., 5e18), np.float32)))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[3]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_misfit_method("ampspec_l2norm")
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="spectral_candidates: an enabled receiver has no misfit taper"):
            p.spectral_candidates(0, 2, 6, cand)
        p.switch_receiver(3, False)
        assert np.all(p.spectral_candidates(0, 2, 6, cand).status == 0)
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_FUSED_FFT", "0")             # read at kiwi_hip_init
    sc, p = build(COMPS)
    try:
        p.set_misfit_method("ampspec_l2norm")
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="spectral_candidates: KIWI_HIP_FUSED_FFT=0"):
            p.spectral_candidates(0, 2, 6, cand)
        p.eval()
        assert np.all(np.isfinite(p.get_misfits()[0]))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 10: helper, example, bootstrap
PLANTED_SDR = (60.0, 60.0, 90.0, 5e18)


def same_mechanism(strike, dip, rake, planted):
    """equal up to the sign: amplitude spectra leave the polarity open, and a double couple has two planes"""
    a = np.array(synthetic.mt_from_sdr(strike, dip, rake, 1.0))
    b = np.array(synthetic.mt_from_sdr(planted[0], planted[1], planted[2], 1.0))
    return min(np.max(np.abs(a - b)), np.max(np.abs(a + b))) <= 1e-6


def test_helper_recovers_the_planted_mechanism_moment_and_bootstrap_mode():
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    rng = np.random.default_rng(12)
    for key, (lo, d) in list(sc.refs.items()):
        sc.refs[key] = (lo, (d + 0.02 * np.std(d) * rng.standard_normal(len(d))).astype(np.float32))
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        dt = sc.gf["dt"]
        for ir in range(1, sc.nrec + 1):
            p.set_misfit_filter(ir, *band(dt))
        row = mt_row(np.zeros(6))
        fixed = {}
        for method in (3, 4):
            p.set_misfit_method(NAMES[method])
            res = fixed[method] = mtfit.scan_double_couples_spectral(p, "moment_tensor", row, *GRID, moment=PLANTED_SDR[3], outer_norm="l2norm", cube=True,
                                                     slot_misfit=True)
            assert res["status"][0] == 0 and res["cube"].shape == (1, 12, 4, 12) and res["moment"][0] == PLANTED_SDR[3]
            assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR), (res["strike"], res["dip"], res["rake"])
            assert res["misfit"][0] == np.nanmin(res["cube"])
        p.set_misfit_method("ampspec_l2norm")
        free = mtfit.scan_double_couples_spectral(p, "moment_tensor", row, *GRID, outer_norm="l2norm", cube=True)
        assert same_mechanism(free["strike"][0], free["dip"][0], free["rake"][0], PLANTED_SDR)
        assert abs(free["moment"][0] - PLANTED_SDR[3]) <= 0.05 * PLANTED_SDR[3], free["moment"]
        # the best moment of every mechanism is never worse than the fixed one (the sums are the same, up to their rounding)
        assert np.all(free["cube"] <= fixed[3]["cube"] * (1 + 1e-9)) and free["moments"].shape == (1, 12, 4, 12)
        # the bootstrap over the receivers through the existing call: the planted mechanism is the mode
        scan = mtfit.scan_double_couples_spectral(p, "moment_tensor", row, *GRID, moment=PLANTED_SDR[3], outer_norm="l2norm", slot_misfit=True)["scan"]
        rec = slot_map(sc, [True] * 6)
        draws = rng.multinomial(sc.nrec, np.full(sc.nrec, 1.0 / sc.nrec), 200).astype(np.float64)
        bv, bi, _ = p.outer_misfits_slots(scan.slot_misfit[0], np.tile(scan.slot_norm[0], (576, 1)), rec, sc.nrec, outer_norm="l2norm",
                                          draw_weights=draws)
        mode = int(np.bincount(bi).argmax())
        sdr = mtfit.double_couple_candidates(*GRID)[1]
        assert same_mechanism(sdr[mode, 0], sdr[mode, 1], sdr[mode, 2], PLANTED_SDR), sdr[mode]
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_ampspec.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism and depth found" in out.stdout and "polarity" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
@pytest.mark.parametrize("method", [3, 4])
def test_a_piece_in_which_every_basis_source_fails_to_discretise(method):
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(COMPS)
    try:
        p.set_misfit_method(NAMES[method])
        eik, good = eikonal_list_with_a_failed_piece(p)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        kw = dict(outer_norm="l2norm", slot_misfit=True, spectra=True, piece=2)
        got = p.spectral_candidates_params("mt_eikonal", eik, 2, cand, **kw)
        assert list(got.status) == [0, 2, 0]
        assert got.best_index[1] == -1 and np.isnan(got.best_misfit[1]) and np.all(np.isnan(got.misfit[1]))
        assert not np.any(got.slot_misfit[1]) and not np.any(got.slot_norm[1])
        assert not np.any(got.spectra[1]) and not np.any(got.spectra_ref[1])
        assert np.all(got.spectra_range[1] == [0, -1, 0])
        assert_beside_a_failed_piece(got, p.spectral_candidates_params("mt_eikonal", good, 2, cand, **kw), common.arith(), NAMES[method])
    finally:
        p.close()
