"""kiwi_hip_waveform_candidates on the device: the slot and fold kernels have the same BITS as the numpy restatement
(tests/waveform_candidates_restatement.py) fed with the device's own kept traces, whatever K, the number of groups, the method,
the outer norm, anarchy, the window length against the LDS stage and the number of candidates against the kernel's tile; unit
candidates against the basis sources' own misfits; the fold against kiwi_hip_outer_misfits; a 576-mechanism grid against its
syntheses; method 1 against the Gram route; the same bits however the call is cut; the refusals; the helper, the bootstrap and
the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import waveform_candidates_restatement as wr
from tests.common import MISFIT_RTOL, SYN_RTOL, Scenario, misfit_close
from tests.linfit_cases import UNIT, assert_beside_a_failed_piece, device_traces, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {1: "l2norm", 2: "l1norm"}
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


def window(p, sc, ir, n):
    """receiver ir (1-based) with a taper over n samples from 20 samples behind its first one, its data followed by zeros where
    the taper reaches beyond them"""
    for k in range(len(sc.comps[ir - 1])):
        lo, d = sc.refs[(ir, k + 1)]
        if len(d) < n + 40:
            p.set_ref_seismogram(ir, k + 1, lo, np.concatenate([d, np.zeros(n + 40 - len(d), np.float32)]))
    p.set_misfit_taper(ir, *synthetic.full_taper(sc.refs[(ir, 1)][0] + 20, n, sc.gf["dt"], 10.0))


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ok = np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if not ok:
        bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
        print(what, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])], len(bad), "of", a.size)
    assert ok, what


def slot_bound(name, dt, syn, ref, cand, m, n):
    """the bound per (candidate, slot) against a synthesis of the combined source: MISFIT_RTOL max(m, n) for the comparison itself
    plus SYN_RTOL T (sum_a |xf_a| max|s_a| + max|v|) for the traces -- the synthesis and the combination each lie within SYN_RTOL of
    their largest sample of the exact trace --, T = dt wlen under l1norm and sqrt(dt wlen) under l2norm.  syn[m] [K, wlen]"""
    xf = np.asarray(cand, np.float64).astype(np.float32)
    out = np.zeros((len(xf), len(syn)))
    for j, rows in enumerate(syn):
        wlen = rows.shape[1]
        T = dt * wlen if name == "l1norm" else np.sqrt(dt * wlen)
        top = np.abs(xf.astype(np.float64)) @ np.max(np.abs(rows.astype(np.float64)), axis=1)
        v = np.max(np.abs(wr.combine(rows, xf).astype(np.float64)), axis=1)
        out[:, j] = SYN_RTOL * T * (top + v)
    return MISFIT_RTOL * np.maximum(m, n) + out


# ------------------------------------------------------------------------------------------------ G1: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_kernels_equal_the_restatement_bit_for_bit(K, ngroup, monkeypatch):
    # (the filtered references a context hands out are made by the transform of its evaluations; the call keeps its filtered rows
    # through the library transforms like kiwi_hip_linear_fit, so the context is made with those throughout: read at kiwi_hip_init)
    monkeypatch.setenv("KIWI_HIP_FUSED_FFT", "0")
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        C, S = p.waveform_candidates_shape(K)
        assert C >= 64 and S >= 64
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy,
        window(p, sc, 2, 100)                                 # one with a window inside one stage
        window(p, sc, 5, 2 * S + 37)                          # and one with a window of two stages and a part of a third
        w = np.array([0.0, 0.7, 2.5, 1.3, 1.0, 4.0])          # one of weight 0; the weight of the disabled receiver never counts
        enabled = [True] * 5 + [False]
        wz = np.where(enabled, w, 0.0)
        for ir in (1, 3, 5):                                  # a pass band on three of the six receivers
            p.set_misfit_filter(ir, *band(dt))
        rec = slot_map(sc, enabled)
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))     # (a group's basis sources share place and time)
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C - 1] = cand[2]                                 # equal misfits across a tile boundary
        cand[C] = cand[2]
        for factor in (1.0, 0.75):
            p.set_synthetics_factor(factor)
            for method in ((1, 2) if factor == 1.0 else (2,)):
                p.set_misfit_method(NAMES[method])
                full = p.waveform_candidates(0, ngroup, K, cand, outer_norm="l2norm", receiver_weights=w, slot_misfit=True)
                assert np.array_equal(full.slot_norm, np.array([p.get_misfits(g * K, 1)[1][0] for g in range(ngroup)]))
                syn, ref, _ = device_traces(p, sc.comps, enabled, 0, ngroup, K, 3)
                wlens = [len(r) for r in ref]
                assert min(wlens) < S and any(n > S and n % S for n in wlens) and max(wlens) == 2 * S + 37, (wlens, S)
                smis = wr.slot_misfits_of(syn, ref, cand, method, dt, factor)
                for norm in ("l1norm", "l2norm"):
                    for anarchy in (False, True):
                        for ncand in (1, C - 1, C, C + 1, 2 * C + 3):
                            what = "K=%d ngroup=%d factor=%g %s %s anarchy=%s ncand=%d" % (K, ngroup, factor, NAMES[method], norm, anarchy, ncand)
                            rs = wr.evaluate(syn, ref, full.slot_norm, rec, wz, anarchy, cand[:ncand], method, norm, dt, factor, smis=smis[:, :ncand])
                            scan = p.waveform_candidates(0, ngroup, K, cand[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                         slot_misfit=True)
                            same(scan.slot_misfit, rs["slot_misfit"], what + " slot_misfit")
                            same(scan.misfit, rs["misfit"], what + " misfit")
                            same(scan.slot_norm, full.slot_norm, what + " slot_norm")
                            same(scan.best_index, rs["best_index"], what + " best_index")
                            same(scan.best_misfit, rs["best_misfit"], what + " best_misfit")
                            same(scan.status, rs["status"], what + " status")
                        assert np.all(scan.status == 0) and np.all(scan.best_index >= 0)
                        assert np.all(scan.misfit[:, C - 1] == scan.misfit[:, 2]) and np.all(scan.misfit[:, C] == scan.misfit[:, 2])
                        assert np.all(scan.slot_norm[:, [s for s, r in enumerate(rec) if r == 3]] == 0)
                ms = p.waveform_candidates_ms()
                assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        p.set_synthetics_factor(1.0)
        # equal misfits on both sides of the tile boundaries: the lowest index wins
        scan = p.waveform_candidates(0, ngroup, K, np.tile(cand[:1], (2 * C + 3, 1)), receiver_weights=w)
        assert np.all(scan.best_index == 0) and np.all(scan.misfit == scan.misfit[:, :1])
        worse = np.tile(3.0 * cand[:1], (2 * C + 3, 1))
        worse[C - 1:C + 1] = 0.0                              # nothing predicted: misfit 1 under the normalised norms, on both sides of a boundary
        scan = p.waveform_candidates(0, ngroup, K, worse, receiver_weights=w)
        lowest = np.argmin(scan.misfit, axis=1)               # (numpy: the first of equal values)
        same(scan.best_index, lowest.astype(np.int32), "lowest index")
        assert np.all(scan.misfit[:, C - 1] == scan.misfit[:, C])
        # no receiver counts: status 1, NaN, no winner; the arrays that are not asked for are not made
        scan = p.waveform_candidates(0, ngroup, K, cand[:3], receiver_weights=np.zeros(6))
        assert np.all(scan.status == 1) and np.all(scan.best_index == -1) and np.all(np.isnan(scan.misfit)) and np.all(np.isnan(scan.best_misfit))
        scan = p.waveform_candidates(0, ngroup, K, cand[:3], misfit=False)
        assert scan.misfit is None and scan.slot_misfit is None and scan.slot_norm is None
        assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G2: unit candidates
@pytest.mark.parametrize("method", [1, 2])
def test_unit_candidates_against_the_basis_sources_own_misfits(method):
    """x = e_a gives v = s_a[i] exactly, so the slot misfit is basis source a's own up to the order of the fp64 sum over the
    samples (a tree over 256 threads there, ascending here): one flipped rounding of the fp32 result at the most, 2^-23."""
    sc, p = build(COMPS)
    try:
        K, ngroup = 6, 3
        S = p.waveform_candidates_shape(K)[1]
        window(p, sc, 2, 100)
        window(p, sc, 5, 2 * S + 37)
        p.set_misfit_method(NAMES[method])
        p.set_source_params("moment_tensor", colocated_groups(np.random.default_rng(3), ngroup, K))
        p.eval()
        m, n, g = p.get_misfits()
        scan = p.waveform_candidates(0, ngroup, K, np.eye(K), outer_norm="l2norm", slot_misfit=True)
        m2, n2, g2 = p.get_misfits()
        assert np.array_equal(m, m2) and np.array_equal(n, n2) and np.array_equal(g, g2)       # the evaluation it leaves is eval's
        mine = scan.slot_misfit.reshape(ngroup * K, -1)
        assert np.array_equal(scan.slot_norm, n[::K])
        rel = np.max(np.abs(mine.astype(np.float64) - m) / np.maximum(np.abs(m), 1e-30))
        print("%s: unit candidates against get_misfits, largest relative difference %.3g (2^-23 = %.3g)" % (NAMES[method], rel, 2.0 ** -23))
        assert misfit_close(mine, m, norm=n)
        assert rel <= 2.0 ** -23
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G3: the fold is outer_misfits'
@pytest.mark.parametrize("method", [1, 2])
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
                scan = p.waveform_candidates(0, ngroup, K, cand, outer_norm=norm, receiver_weights=w, anarchy=anarchy, slot_misfit=True)
                for g in range(ngroup):
                    bv, bi, gl = p.outer_misfits_slots(scan.slot_misfit[g], np.tile(scan.slot_norm[g], (len(cand), 1)), rec, sc.nrec,
                                                       outer_norm=norm, receiver_weights=w, anarchy=anarchy, which_draw=0)
                    same(scan.misfit[g], gl, "%s %s anarchy=%s group %d" % (NAMES[method], norm, anarchy, g))
                    assert scan.best_index[g] == bi[0] and scan.best_misfit[g] == bv[0]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G4: against syntheses
@pytest.mark.parametrize("method,norm", [(2, "l1norm"), (2, "l2norm"), (1, "l2norm")])
def test_the_mechanism_grid_against_its_syntheses(method, norm, monkeypatch):
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt, K, moment = sc.gf["dt"], 6, 7e18
        p.set_misfit_method(NAMES[method])
        row = mt_row(np.zeros(6))
        rec = slot_map(sc, [True] * 6)
        cand, sdr = mtfit.double_couple_candidates(*GRID, moment / UNIT)
        scan = p.waveform_candidates_params("moment_tensor", mtfit.elementary_params("moment_tensor", row[None, :], UNIT), K, cand,
                                            outer_norm=norm, slot_misfit=True)
        assert p.nsrc == 6 and scan.status[0] == 0 and scan.slot_misfit.shape[:2] == (1, 576)
        syn, ref, _ = device_traces(p, sc.comps, [True] * 6, 0, 1, K, 2)
        grid = np.array([mt_row(np.asarray(t * UNIT, np.float32), row[:4], row[10]) for t in cand], np.float32)
        m, n, _, status = p.misfits_for_params("moment_tensor", grid)
        assert len(m) == 576 and not np.any(status) and np.array_equal(n[0], scan.slot_norm[0])
        g = p.outer_misfits_slots(m, n, rec, sc.nrec, outer_norm=norm, which_draw=0)[2]
        m, n = m.astype(np.float64), n.astype(np.float64)
        bound = slot_bound(NAMES[method], dt, [s[0] for s in syn], ref, cand, m, n)
        dm = np.abs(scan.slot_misfit[0].astype(np.float64) - m)
        ibest, imin = int(scan.best_index[0]), int(np.argmin(g))
        print("%s inside, %s outside: 576 double couples, largest |dm| / max(m, n) %.3g, largest |dm| / bound %.3g, worst |predicted - evaluated| "
              "%.3g; best predicted %.9f at (%g, %g, %g), evaluated there %.9f, evaluated minimum %.9f" % (
                  NAMES[method], norm, np.max(dm / np.maximum(m, n)), np.max(dm / bound), np.max(np.abs(scan.misfit[0] - g)), scan.best_misfit[0],
                  sdr[ibest, 0], sdr[ibest, 1], sdr[ibest, 2], g[ibest], g[imin]))
        assert np.all(dm <= bound)
        contract = common.arith()
        monkeypatch.setenv("KIWI_HIP_ARITH", "fused")         # the rule on the scale of the norm factors, for both contracts
        assert misfit_close(scan.misfit[0], g, glob=True)
        assert misfit_close(g[ibest], g[imin], glob=True)
        monkeypatch.setenv("KIWI_HIP_ARITH", contract)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G5: against the Gram route
def test_l2norm_from_the_residual_against_linear_fit_candidates():
    """Under the outer l2norm the per-slot fold and the Gram route's receiver-level fold are the same quantity,
    sqrt(sum_r w_r^2 |d_r - v_r|^2 / sum_r w_r^2 |d_r|^2); with candidates that are exact in fp32 both routes evaluate the same
    coefficients, and each lies within MISFIT_RTOL sqrt(g^2 + 1) of it by the suite's rule for global misfits."""
    sc, p = build(COMPS)
    try:
        K, ngroup = 6, 3
        p.set_misfit_method("l2norm")
        rng = np.random.default_rng(17)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K)).astype(np.float32).astype(np.float64)
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        worst = 0.0
        for anarchy in (False, True):
            wave = p.waveform_candidates(0, ngroup, K, cand, outer_norm="l2norm", receiver_weights=w, anarchy=anarchy)
            gram = p.linear_fit_candidates(0, ngroup, K, cand, outer_norm="l2norm", receiver_weights=w, anarchy=anarchy)
            ratio = np.abs(wave.misfit - gram.misfit) / (MISFIT_RTOL * np.sqrt(gram.misfit ** 2 + 1.0))
            worst = max(worst, float(np.max(ratio)))
            assert np.array_equal(wave.status, gram.status)
            assert np.all(ratio <= 1.0), (anarchy, np.max(ratio))
        print("l2norm from the residual against the Gram route: largest |dg| / (MISFIT_RTOL sqrt(g^2 + 1)) %.3g" % worst)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G6: the same bits however it is cut
def assert_same_scan(a, b, slack, what):
    """two scans of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.  fused: the
    batch shape chooses the accumulate kernel instantiation, so the kept traces agree within SYN_RTOL of their maximum, 64 SYN_RTOL
    of their norm (assert_same_fit of tests/test_linfit_gpu.py); carried through the combination a slot misfit moves by at most
    64 SYN_RTOL sum_a |x_a| norm(s_a) and the global misfit by slack[g, c], those over the norm factors folded the same way."""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("best_index", "best_misfit", "misfit", "slot_misfit", "slot_norm"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (what, name)
        return
    assert np.all(np.abs(a.misfit - b.misfit) <= slack), what
    assert np.all(np.abs(a.best_misfit - b.best_misfit) <= np.max(slack, axis=1)), what


@pytest.mark.parametrize("method,norm", [(2, "l1norm"), (1, "l2norm")])
def test_first_source_chunks_pieces_and_contexts(method, norm, monkeypatch):
    ngroup, K = 12, 6
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    kw = dict(outer_norm=norm, slot_misfit=True)

    def prepared(**more):
        sc, q = build(COMPS, **more)
        q.set_misfit_method(NAMES[method])
        return sc, q

    sc, p = prepared()
    try:
        dt = sc.gf["dt"]
        p.set_source_params("moment_tensor", rows)
        base = p.waveform_candidates(0, ngroup, K, cand, **kw)
        assert np.all(base.status == 0)
        syn, ref, _ = device_traces(p, sc.comps, [True] * 6, 0, ngroup, K, 2)
        rec = np.array(slot_map(sc, [True] * 6))
        slack = np.zeros((ngroup, len(cand)))
        for g in range(ngroup):
            # the norm of basis trace a under the inner norm, [nmis, K]
            if method == 2:
                nb = np.array([dt * np.sum(np.abs(s[g].astype(np.float64)), axis=1) for s in syn])
            else:
                nb = np.array([np.sqrt(dt * np.sum(s[g].astype(np.float64) ** 2, axis=1)) for s in syn])
            per_slot = 64 * SYN_RTOL * (np.abs(cand) @ nb.T)                      # [ncand, nmis]
            n = base.slot_norm[g].astype(np.float64)
            if norm == "l2norm":
                slack[g] = np.sqrt(np.sum(per_slot ** 2, axis=1)) / np.sqrt(np.sum(n * n))
            else:
                slack[g] = np.sum(per_slot, axis=1) / np.sum(n)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_scan(base, p.waveform_candidates(5, ngroup, K, cand, **kw), slack, "isrc0 = 5")
        for piece in (1, 5):
            assert_same_scan(base, p.waveform_candidates_params("moment_tensor", rows, K, cand, piece=piece, **kw), slack, "piece %d" % piece)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups: read at kiwi_hip_init
    sc, q = prepared()
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_scan(base, q.waveform_candidates(0, ngroup, K, cand, **kw), slack, "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = prepared(engine=multi_engine(2))                  # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        assert_same_scan(base, m.waveform_candidates_params("moment_tensor", rows, K, cand, **kw), slack, "two contexts")
        assert_same_scan(base, m.waveform_candidates_params("moment_tensor", rows, K, cand, piece=2 * K, **kw), slack, "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ G7: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable(monkeypatch):
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_misfit_method("l1norm")
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()

        def still_usable():
            p.eval()
            for a, b in zip(before, p.get_misfits()):
                assert np.array_equal(a, b)

        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        fp = lambda a: None if a is None else a.ctypes.data_as(c_float_p)            # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)              # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, slots=(False, False), isrc0=0, ngroup=2, params_form=True, null=None):
            """both C entries with these arguments: refused, with the reason in a message that starts with the call's name"""
            bi, bm, st = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32)
            sm = np.zeros(2 * 5 * 32, np.float32) if slots[0] else None
            sn = np.zeros(2 * 32, np.float32) if slots[1] else None
            x = None if null == "candidates" else np.ascontiguousarray(x, np.float64)
            tail = (ncand, dp(x), outer, None, 0, ip(None if null == "best_index" else bi), dp(None if null == "best_misfit" else bm),
                    ip(None if null == "status" else st), None, fp(sm), fp(sn))
            rc = p.L.kiwi_hip_waveform_candidates(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="waveform_candidates: .*" + match):
                p._ck(rc, "waveform_candidates")
            if params_form:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_waveform_candidates_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="waveform_candidates: .*" + match):
                    p._ck(rc, "waveform_candidates")
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
        entry("slot_misfit and slot_norm come together", slots=(True, False))
        entry("slot_misfit and slot_norm come together", slots=(False, True))
        for null in ("candidates", "best_index", "best_misfit", "status"):
            entry("null candidates, best_index, best_misfit or status array", null=null)
        for K in (0, 9):
            entry("basis sources per group", K=K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, params_form=False)
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.waveform_candidates(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.waveform_candidates(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="no closed form under l1norm"):
            mtfit.scan_double_couples_waveform(p, "moment_tensor", rows[0], [0.], [45.], [90.], moment=None)
        # a method other than 1 or 2: the message says where the others go
        for method in ("ampspec_l2norm", "ampspec_l1norm", "floating_l2norm", "peak"):
            p.set_misfit_method(method)
            with pytest.raises(KiwiHipError, match="waveform_candidates: the misfit method must be l1norm or l2norm .*linear_fit_candidates_floating.*spectral_candidates"):
                p.waveform_candidates(0, 2, 6, cand)
            with pytest.raises(KiwiHipError, match="waveform_candidates: the misfit method must be l1norm or l2norm"):
                p.waveform_candidates_params("moment_tensor", rows, 6, cand)
            p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("l1norm")
        still_usable()
        assert np.all(p.waveform_candidates(0, 2, 6, cand).status == 0)
        still_usable()
    finally:
        p.close()
    # a transform workspace that does not hold one group: a misfit filter sends the kept rows through the transforms, and windows
    # of 2000 samples need 17 slots x 2048 samples x 12 bytes and more per source, of which 1 MiB holds fewer than six
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # read at kiwi_hip_init
    sc, p = build(COMPS)
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    try:
        p.set_misfit_method("l1norm")
        p.set_misfit_filter(1, *band(sc.gf["dt"]))
        for ir in range(1, 7):
            window(p, sc, ir, 2000)
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="waveform_candidates: the transform workspace .* does not hold one group"):
            p.waveform_candidates(0, 2, 6, cand)
        with pytest.raises(KiwiHipError, match="waveform_candidates: the transform workspace .* does not hold one group"):
            p.waveform_candidates_params("moment_tensor", rows, 6, cand)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        assert np.all(np.isfinite(p.get_misfits()[0]))
        assert np.all(p.waveform_candidates(0, 12, 1, cand[:, :1]).status == 0)       # (groups of one source fit)
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
        q.set_misfit_method("l1norm")
        q.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="waveform_candidates: .*needs a reference seismogram"):
            q.waveform_candidates(0, 2, 6, cand)
        with pytest.raises(KiwiHipError, match="waveform_candidates: .*needs a reference seismogram"):
            q.waveform_candidates_params("moment_tensor", rows, 6, cand)
        q.set_ref_seismogram(3, 2, *sc.refs[(3, 2)])
        q.set_source_params("moment_tensor", rows)
        scan = q.waveform_candidates(0, 2, 6, cand)
        assert np.all(scan.status == 0) and np.all(np.isfinite(scan.misfit))
    finally:
        q.close()
    # an enabled receiver without a misfit taper
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(np.array(synthetic.mt_from_sdr(40., 60., 100., 5e18), np.float32)))
    e = sc.oracle()
    sc.make_references(e)
    del sc.tapers[3]
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_misfit_method("l1norm")
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="waveform_candidates: an enabled receiver has no misfit taper"):
            p.waveform_candidates(0, 2, 6, cand)
        p.switch_receiver(3, False)
        assert np.all(p.waveform_candidates(0, 2, 6, cand).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G8: helper, bootstrap, example
PLANTED_SDR = (60.0, 60.0, 90.0, 5e18)


def same_mechanism(strike, dip, rake, planted):
    """equal as tensors: a double couple has two planes (the waveform fixes the polarity)"""
    a = np.array(synthetic.mt_from_sdr(strike, dip, rake, 1.0))
    b = np.array(synthetic.mt_from_sdr(planted[0], planted[1], planted[2], 1.0))
    return np.max(np.abs(a - b)) <= 1e-6


def test_helper_recovers_the_planted_mechanism_under_a_glitch_moment_axis_and_bootstrap_mode():
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    rng = np.random.default_rng(12)
    for key, (lo, d) in list(sc.refs.items()):
        sc.refs[key] = (lo, (d + 0.02 * np.std(d) * rng.standard_normal(len(d))).astype(np.float32))
    for k in range(len(sc.comps[2])):                         # station 3: its data replaced by a glitch, a step of 20 times their size
        lo, d = sc.refs[(3, k + 1)]
        sc.refs[(3, k + 1)] = (lo, (20.0 * np.max(np.abs(d)) * (np.arange(len(d)) > len(d) // 3)).astype(np.float32))
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_misfit_method("l1norm")
        row = mt_row(np.zeros(6))
        res = mtfit.scan_double_couples_waveform(p, "moment_tensor", row, *GRID, moment=PLANTED_SDR[3], outer_norm="l1norm", cube=True,
                                                 slot_misfit=True)
        assert res["status"][0] == 0 and res["cube"].shape == (1, 12, 4, 12) and res["moment"][0] == PLANTED_SDR[3]
        assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR), (res["strike"], res["dip"], res["rake"])
        assert res["misfit"][0] == np.nanmin(res["cube"])
        # a moment axis: the planted moment comes out first among three
        moments = (PLANTED_SDR[3], 0.5 * PLANTED_SDR[3], 2.0 * PLANTED_SDR[3])
        axis = mtfit.scan_double_couples_waveform(p, "moment_tensor", row, *GRID, moment=moments, outer_norm="l1norm", cube=True)
        assert axis["cube"].shape == (1, 12, 4, 12, 3) and axis["moment"][0] == PLANTED_SDR[3] and axis["index"][0] == 3 * res["index"][0]
        assert same_mechanism(axis["strike"][0], axis["dip"][0], axis["rake"][0], PLANTED_SDR)
        assert np.array_equal(axis["cube"][..., 0], res["cube"])
        # the bootstrap over the receivers through the existing call: the planted mechanism is the mode
        scan = res["scan"]
        rec = slot_map(sc, [True] * 6)
        draws = rng.multinomial(sc.nrec, np.full(sc.nrec, 1.0 / sc.nrec), 200).astype(np.float64)
        bv, bi, _ = p.outer_misfits_slots(scan.slot_misfit[0], np.tile(scan.slot_norm[0], (576, 1)), rec, sc.nrec, outer_norm="l1norm",
                                          draw_weights=draws)
        mode = int(np.bincount(bi).argmax())
        sdr = mtfit.double_couple_candidates(*GRID)[1]
        assert same_mechanism(sdr[mode, 0], sdr[mode, 1], sdr[mode, 2], PLANTED_SDR), sdr[mode]
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_l1.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism and depth found" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
@pytest.mark.parametrize("method,norm", [(2, "l1norm"), (1, "l2norm")])
def test_a_piece_in_which_every_basis_source_fails_to_discretise(method, norm):
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(COMPS)
    try:
        p.set_misfit_method(NAMES[method])
        eik, good = eikonal_list_with_a_failed_piece(p)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        kw = dict(outer_norm=norm, slot_misfit=True, piece=2)
        got = p.waveform_candidates_params("mt_eikonal", eik, 2, cand, **kw)
        assert list(got.status) == [0, 2, 0]
        assert got.best_index[1] == -1 and np.isnan(got.best_misfit[1]) and np.all(np.isnan(got.misfit[1]))
        assert not np.any(got.slot_misfit[1]) and not np.any(got.slot_norm[1])
        assert_beside_a_failed_piece(got, p.waveform_candidates_params("mt_eikonal", good, 2, cand, **kw), common.arith(), norm)
    finally:
        p.close()
