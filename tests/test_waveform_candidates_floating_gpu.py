"""kiwi_hip_waveform_candidates_floating on the device: the floating slot kernel, the fold and the shift gather have the same BITS
as the numpy restatement (tests/waveform_candidates_floating_restatement.py) fed with the device's own kept traces and its own moved,
tapered references, whatever K, the number of groups, the method, the outer norm, anarchy, the window length against the LDS stage,
the number of candidates against the tile and the number of shifts against the pass; every range (0, 0) against
kiwi_hip_waveform_candidates; unit candidates against the basis sources' own floating evaluation; a 576-mechanism grid against its
syntheses under floating_l1norm; the fold against kiwi_hip_outer_misfits; the same bits however the call is cut; a failed basis
source; the refusals; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import waveform_candidates_floating_restatement as fr
from tests.common import MISFIT_RTOL, SYN_RTOL, Scenario
from tests.linfit_cases import PLANTED, UNIT, assert_beside_a_failed_piece, device_traces, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups
from tests.test_waveform_candidates_gpu import GRID, NAMES, same, same_mechanism, slot_bound, slot_map, window, zero_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("slot_misfit", "cand_shift", "misfit", "best_index", "best_misfit", "best_shift", "status")


def set_ranges(p, dt, ranges):
    for ir, (lo, hi) in enumerate(ranges):
        p.set_floating_shiftrange(ir + 1, lo * dt, hi * dt)


def device_shifted_references(p, sc, enabled, ranges, dt):
    """aq[m] [ns, wlen] of the enabled receivers' slots: the device's own tapered references with the data moved by every shift of
    the range (`shift_ref_seismogram`, and back).  Under a plain norm"""
    ns = [hi - lo + 1 for lo, hi in ranges]
    aq = {}
    for j in range(max(ns)):
        sh = [ranges[r][0] + min(j, ns[r] - 1) for r in range(len(ranges))]
        for r, s in enumerate(sh):
            p.shift_ref_seismogram(r + 1, s * dt)
        m = 0
        for r, c in enumerate(sc.comps):
            if not enabled[r]:
                continue
            for k in range(len(c)):
                a = p.get_reference(r + 1, k + 1, 2, maxn=1 << 14)[1]
                if j == 0:
                    aq[m] = np.zeros((ns[r], len(a)), np.float32)
                if j < ns[r]:
                    aq[m][j] = a
                m += 1
        for r, s in enumerate(sh):
            p.shift_ref_seismogram(r + 1, -s * dt)
    return [aq[m] for m in range(len(aq))]


def receiver_sums(smis, rec, nrec, method):
    """[..., nrec] float64 from slot misfits [..., nmis]: sum_k m_k (l1 inside) or sqrt(sum_k m_k^2) (l2 inside) per receiver"""
    s = np.asarray(smis, np.float64)
    out = np.zeros(s.shape[:-1] + (nrec,))
    for m, r in enumerate(rec):
        out[..., r] += s[..., m] if method == 2 else s[..., m] ** 2
    return out if method == 2 else np.sqrt(out)


# ------------------------------------------------------------------------------------------------ F1: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_kernels_equal_the_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        C, S, J = p.waveform_candidates_floating_shape(K)
        assert C >= 64 and S >= 64 and J >= 4
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy at any shift,
        window(p, sc, 2, 100)                                 # one with a window inside one stage
        window(p, sc, 5, 2 * S + 37)                          # and one with a window of two stages and a part of a third
        w = np.array([0.0, 0.7, 2.5, 1.3, 1.0, 4.0])          # one of weight 0; the weight of the disabled receiver never counts
        enabled = [True] * 5 + [False]
        wz = np.where(enabled, w, 0.0)
        # a pass of J shifts exactly (negative only, the one-component receiver), 5 shifts, an asymmetric range (the three-component
        # receiver), one shift, a pass and one shift of a second
        ranges = [(1 - J, 0), (-2, 2), (-3, 7), (0, 0), (-4, J - 4), (-1, 1)]
        assert [hi - lo + 1 for lo, hi in ranges[:5]] == [J, 5, 11, 1, J + 1] and [len(c) for c in sc.comps[:3]] == [1, 2, 3]
        rec = slot_map(sc, enabled)
        rng = np.random.default_rng(10 * K + ngroup)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C - 1] = cand[2]                                 # equal candidates across a tile boundary
        cand[C] = cand[2]
        p.set_misfit_method("l1norm")
        aq = device_shifted_references(p, sc, enabled, ranges, dt)
        lo = [r[0] for r in ranges]
        for factor in (1.0, 0.75):
            p.set_synthetics_factor(factor)
            for method in ((1, 2) if factor == 1.0 else (2,)):
                p.set_misfit_method(NAMES[method])            # the kept traces of the plain evaluation
                p.set_floating_shiftrange(0, 0.0, 0.0)
                p.waveform_candidates(0, ngroup, K, cand[:1])
                syn, ref, _ = device_traces(p, sc.comps, enabled, 0, ngroup, K, 2)
                assert all(np.array_equal(a[-lo[rec[m]]], ref[m]) for m, a in enumerate(aq) if lo[rec[m]] <= 0)      # shift 0: the tapered reference
                wlens = [len(r) for r in ref]
                assert min(wlens) < S and max(wlens) == 2 * S + 37, (wlens, S)
                p.set_misfit_method("floating_" + NAMES[method])
                set_ranges(p, dt, ranges)
                full = p.waveform_candidates_floating(0, ngroup, K, cand, outer_norm="l2norm", receiver_weights=w, slot_misfit=True)
                assert np.array_equal(full.slot_norm, np.array([p.get_misfits(g * K, 1)[1][0] for g in range(ngroup)]))
                mkq = [[fr.slot_misfits_per_shift(syn[m][g], aq[m], cand, method, dt, factor) for m in range(len(syn))] for g in range(ngroup)]
                for norm in ("l1norm", "l2norm"):
                    for anarchy in (False, True):
                        for ncand in (1, C - 1, C, C + 1, 2 * C + 3):
                            what = "K=%d ngroup=%d factor=%g %s %s anarchy=%s ncand=%d" % (K, ngroup, factor, NAMES[method], norm, anarchy, ncand)
                            rs = fr.evaluate(syn, aq, lo, full.slot_norm, rec, wz, anarchy, cand[:ncand], method, norm, dt, factor, mkq=mkq)
                            scan = p.waveform_candidates_floating(0, ngroup, K, cand[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                                  cand_shift=True, slot_misfit=True)
                            for name in OUTPUTS:
                                same(getattr(scan, name), rs[name], what + " " + name)
                            same(scan.slot_norm, full.slot_norm, what + " slot_norm")
                        assert np.all(scan.status == 0) and np.all(scan.best_index >= 0)
                        assert np.all(scan.misfit[:, C - 1] == scan.misfit[:, 2]) and np.all(scan.misfit[:, C] == scan.misfit[:, 2])
                        assert np.all(scan.cand_shift[:, C - 1] == scan.cand_shift[:, 2]) and np.all(scan.cand_shift[:, C] == scan.cand_shift[:, 2])
                        assert np.all(scan.slot_norm[:, [s for s, r in enumerate(rec) if r == 3]] == 0)
                        assert np.all(scan.cand_shift[:, :, 5] == 0) and np.all(scan.best_shift[:, 5] == 0)
                        for r in range(5):
                            assert np.all((scan.cand_shift[:, :, r] >= ranges[r][0]) & (scan.cand_shift[:, :, r] <= ranges[r][1]))
                ms = p.waveform_candidates_floating_ms()
                assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
        p.set_synthetics_factor(1.0)
        # no receiver counts: status 1, NaN, no winner, no shifts; the arrays that are not asked for are not made
        scan = p.waveform_candidates_floating(0, ngroup, K, cand[:3], receiver_weights=np.zeros(6))
        assert np.all(scan.status == 1) and np.all(scan.best_index == -1) and np.all(np.isnan(scan.misfit)) and np.all(np.isnan(scan.best_misfit))
        assert not np.any(scan.best_shift)
        scan = p.waveform_candidates_floating(0, ngroup, K, cand[:3], misfit=False)
        assert scan.misfit is None and scan.cand_shift is None and scan.slot_misfit is None and scan.slot_norm is None
        assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F2: every range (0, 0)
@pytest.mark.parametrize("method", [1, 2])
def test_ranges_of_one_shift_equal_waveform_candidates_bit_for_bit(method):
    sc, p = build(COMPS)
    try:
        K, ngroup = 6, 3
        S = p.waveform_candidates_floating_shape(K)[1]
        p.switch_receiver(6, False)
        zero_reference(p, sc, 4)
        window(p, sc, 2, 100)
        window(p, sc, 5, 2 * S + 37)
        w = np.array([0.0, 0.7, 2.5, 1.3, 1.0, 4.0])
        rng = np.random.default_rng(21)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        p.set_floating_shiftrange(0, 0.0, 0.0)
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                kw = dict(outer_norm=norm, receiver_weights=w, anarchy=anarchy, slot_misfit=True)
                p.set_misfit_method(NAMES[method])
                plain = p.waveform_candidates(0, ngroup, K, cand, **kw)
                p.set_misfit_method("floating_" + NAMES[method])
                fl = p.waveform_candidates_floating(0, ngroup, K, cand, cand_shift=True, **kw)
                for name in ("best_index", "best_misfit", "status", "misfit", "slot_misfit", "slot_norm"):
                    same(getattr(fl, name), getattr(plain, name), "%s %s anarchy=%s %s" % (NAMES[method], norm, anarchy, name))
                assert not np.any(fl.cand_shift) and not np.any(fl.best_shift)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F3: unit candidates
DELAYS = [1, -2, 3, 0, -3, 2]                               # samples by which each station's references are moved
UNIT_RANGES = [(-2, 2), (-1, 3), (-4, 2), (-1, 3), (-4, 4), (-2, 3)]       # 5 to 9 shifts; each holds -delay


@pytest.mark.parametrize("method", [1, 2])
def test_unit_candidates_against_the_basis_sources_own_floating_evaluation(method):
    """x = e_a gives v = s_a[i] exactly, so m_kq is basis source a's own at every shift up to the order of the fp64 sum (a tree
    there, ascending here) and the rounding of the fp32 result.  Per receiver F = sum_k m_k (l1 inside) or sqrt(sum_k m_k^2) (l2
    inside) at the winning shift is the minimum over the shifts of a function that is 1-Lipschitz in the m_kq, so it is compared
    within the suite's rule for two comparators summed over the receiver's slots, sum_k MISFIT_RTOL max(m_k, n_k), whichever of two
    nearly equal shifts either side took.  The shifts themselves: the planted source as a group of one on noise-free data moved
    by DELAYS returns get_floating_shifts' own, the shifts -DELAYS."""
    sc, p = build(COMPS)
    try:
        dt, K, ngroup, nrec = sc.gf["dt"], 6, 3, sc.nrec
        for ir in range(nrec):
            p.shift_ref_seismogram(ir + 1, DELAYS[ir] * dt)
        p.set_misfit_method("floating_" + NAMES[method])
        set_ranges(p, dt, UNIT_RANGES)
        rec = slot_map(sc, [True] * 6)
        p.set_source_params("moment_tensor", colocated_groups(np.random.default_rng(3), ngroup, K))
        p.eval()
        m, n, g = p.get_misfits()
        shifts = p.get_floating_shifts()
        scan = p.waveform_candidates_floating(0, ngroup, K, np.eye(K), outer_norm="l2norm", slot_misfit=True, cand_shift=True)
        m2, n2, g2 = p.get_misfits()
        assert np.array_equal(m, m2) and np.array_equal(n, n2) and np.array_equal(g, g2)       # the evaluation it leaves is eval's
        assert np.array_equal(shifts, p.get_floating_shifts())
        assert np.array_equal(scan.slot_norm, n[::K])
        mine = receiver_sums(scan.slot_misfit.reshape(ngroup * K, -1), rec, nrec, method)
        theirs = receiver_sums(m, rec, nrec, method)
        bound = np.zeros_like(theirs)
        for k, r in enumerate(rec):
            bound[:, r] += MISFIT_RTOL * np.maximum(m[:, k], n[:, k])
        print("%s: unit candidates against get_misfits, largest |dF| / bound %.3g; %d of %d shifts equal get_floating_shifts'" % (
            NAMES[method], np.max(np.abs(mine - theirs) / bound), int(np.sum(scan.cand_shift.reshape(ngroup * K, nrec) == np.rint(shifts / dt))), shifts.size))
        assert np.all(np.abs(mine - theirs) <= bound)
        # the planted source itself, a group of one
        p.set_source_params("moment_tensor", mt_row(PLANTED)[None, :])
        p.eval()
        want = np.rint(p.get_floating_shifts()[0] / dt).astype(np.int32)
        assert list(want) == [-d for d in DELAYS]
        one = p.waveform_candidates_floating(0, 1, 1, [[1.0]], cand_shift=True, slot_misfit=True)
        assert np.array_equal(one.best_shift[0], want) and np.array_equal(one.cand_shift[0, 0], want.astype(np.int16)) and one.best_index[0] == 0
        assert one.best_misfit[0] <= 1e-3                     # (the planted source on its own noise-free data)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F4: against syntheses
GRID_RANGES = [(-2, 2), (-3, 1), (-2, 4), (-1, 3), (-4, 4), (-2, 3)]       # 5 to 9 shifts


def test_the_mechanism_grid_against_its_syntheses_under_floating_l1norm(monkeypatch):
    """12 x 4 x 12 double couples at 30 degrees against `misfits_for_params` of the same rows under floating_l1norm on the same
    context, l1norm outside.  Per (mechanism, receiver) F = sum_k m_k at the winning shift is a minimum over the shifts,
    1-Lipschitz in the per-shift slot misfits, so it is held to `slot_bound` (tests/test_waveform_candidates_gpu.py) summed over the
    receiver's slots, whichever of two nearly equal shifts either side took.  The best mechanism: both global misfits lie within
    the suite's rule for a global misfit, tol = MISFIT_RTOL sqrt(g^2 + 1), of the exact one, so the same mechanism wins where the
    evaluation's runner-up lies more than 2 tol above its minimum."""
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt, K, moment, nrec = sc.gf["dt"], 6, 7e18, sc.nrec
        for ir in range(nrec):                                # every station late or early by a few samples
            p.shift_ref_seismogram(ir + 1, DELAYS[ir] * dt)
        p.set_misfit_method("floating_l1norm")
        set_ranges(p, dt, GRID_RANGES)
        row = mt_row(np.zeros(6))
        rec = slot_map(sc, [True] * 6)
        cand, sdr = mtfit.double_couple_candidates(*GRID, moment / UNIT)
        res = mtfit.scan_double_couples_waveform_floating(p, "moment_tensor", row, *GRID, moment=moment, outer_norm="l1norm", cube=True,
                                                          slot_misfit=True)
        scan = res["scan"]
        assert p.nsrc == 6 and scan.status[0] == 0 and scan.slot_misfit.shape[:2] == (1, 576) and res["cube"].shape == (1, 12, 4, 12)
        assert res["cube_shifts"].shape == (1, 12, 4, 12, nrec)
        syn, ref, _ = device_traces(p, sc.comps, [True] * 6, 0, 1, K, 2)
        grid = np.array([mt_row(np.asarray(t * UNIT, np.float32), row[:4], row[10]) for t in cand], np.float32)
        m, n, _, status = p.misfits_for_params("moment_tensor", grid)
        assert len(m) == 576 and not np.any(status) and np.array_equal(n[0], scan.slot_norm[0])
        shifts = np.rint(p.get_floating_shifts() / dt).astype(int)
        g = p.outer_misfits_slots(m, n, rec, nrec, outer_norm="l1norm", which_draw=0)[2]
        m, n = m.astype(np.float64), n.astype(np.float64)
        per_slot = slot_bound("l1norm", dt, [s[0] for s in syn], ref, cand, m, n)
        bound = np.zeros((576, nrec))
        for k, r in enumerate(rec):
            bound[:, r] += per_slot[:, k]
        dF = np.abs(receiver_sums(scan.slot_misfit[0], rec, nrec, 2) - receiver_sums(m, rec, nrec, 2))
        ibest, imin = int(scan.best_index[0]), int(np.argmin(g))
        two = np.sort(g)[:2]
        tol = MISFIT_RTOL * np.sqrt(two[0] ** 2 + 1.0)
        print("floating_l1norm inside, l1norm outside: 576 double couples, largest |dF| / bound %.3g, worst |predicted - evaluated| %.3g; %d of %d "
              "shifts differ from the evaluation's; best predicted %.9f at (%g, %g, %g), evaluated there %.9f, evaluated minimum %.9f, runner-up "
              "%.9f" % (np.max(dF / bound), np.max(np.abs(scan.misfit[0] - g)), int(np.sum(scan.cand_shift[0] != shifts)), shifts.size,
                        scan.best_misfit[0], sdr[ibest, 0], sdr[ibest, 1], sdr[ibest, 2], g[ibest], two[0], two[1]))
        assert np.all(dF <= bound)
        assert abs(g[ibest] - two[0]) <= 2 * tol
        if two[1] - two[0] > 2 * tol:
            assert ibest == imin
        assert [res["strike"][0], res["dip"][0], res["rake"][0]] == list(sdr[ibest]) and res["moment"][0] == moment
        assert np.array_equal(res["shifts"][0], scan.cand_shift[0, ibest] * dt) and np.array_equal(scan.best_shift[0], scan.cand_shift[0, ibest])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F5: the fold is outer_misfits'
@pytest.mark.parametrize("method", [1, 2])
def test_outer_fold_is_kiwi_hip_outer_misfits_on_the_calls_own_slots(method):
    sc, p = build(COMPS)
    try:
        dt, K, ngroup = sc.gf["dt"], 6, 2
        p.switch_receiver(6, False)
        zero_reference(p, sc, 4)
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        rec = slot_map(sc, [True] * 5 + [False])
        p.set_misfit_method("floating_" + NAMES[method])
        set_ranges(p, dt, GRID_RANGES)
        rng = np.random.default_rng(61)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                scan = p.waveform_candidates_floating(0, ngroup, K, cand, outer_norm=norm, receiver_weights=w, anarchy=anarchy, slot_misfit=True)
                for g in range(ngroup):
                    bv, bi, gl = p.outer_misfits_slots(scan.slot_misfit[g], np.tile(scan.slot_norm[g], (len(cand), 1)), rec, sc.nrec,
                                                       outer_norm=norm, receiver_weights=w, anarchy=anarchy, draw_weights=np.ones((1, sc.nrec)),
                                                       which_draw=0)
                    same(scan.misfit[g], gl, "%s %s anarchy=%s group %d" % (NAMES[method], norm, anarchy, g))
                    assert scan.best_index[g] == bi[0] and scan.best_misfit[g] == bv[0]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F6: the same bits however it is cut
def assert_same_scan(a, b, slack, what):
    """two scans of the same groups through different chunkings / pieces / contexts.  exact contract: the same bits.  fused: the
    batch shape chooses the accumulate kernel instantiation, so the kept traces agree within 64 SYN_RTOL of their norm; carried
    through the combination a slot misfit moves by at most 64 SYN_RTOL sum_a |x_a| norm(s_a) at EVERY shift, and so does the
    minimum over the shifts; the global misfit by slack[g, c], those over the norm factors folded the same way."""
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        for name in ("best_index", "best_misfit", "best_shift", "misfit", "cand_shift", "slot_misfit", "slot_norm"):
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
    kw = dict(outer_norm=norm, slot_misfit=True, cand_shift=True)

    def prepared(**more):
        sc, q = build(COMPS, **more)
        q.set_misfit_method("floating_" + NAMES[method])
        set_ranges(q, sc.gf["dt"], GRID_RANGES)
        return sc, q

    sc, p = prepared()
    try:
        dt = sc.gf["dt"]
        p.set_source_params("moment_tensor", rows)
        base = p.waveform_candidates_floating(0, ngroup, K, cand, **kw)
        assert np.all(base.status == 0)
        slack = np.zeros((ngroup, len(cand)))
        if common.arith() != "exact":
            p.set_misfit_method(NAMES[method])
            p.waveform_candidates(0, ngroup, K, cand[:1])
            syn, _, _ = device_traces(p, sc.comps, [True] * 6, 0, ngroup, K, 2)
            p.set_misfit_method("floating_" + NAMES[method])
            for g in range(ngroup):
                if method == 2:
                    nb = np.array([dt * np.sum(np.abs(s[g].astype(np.float64)), axis=1) for s in syn])
                else:
                    nb = np.array([np.sqrt(dt * np.sum(s[g].astype(np.float64) ** 2, axis=1)) for s in syn])
                per_slot = 64 * SYN_RTOL * (np.abs(cand) @ nb.T)
                n = base.slot_norm[g].astype(np.float64)
                slack[g] = np.sqrt(np.sum(per_slot ** 2, axis=1)) / np.sqrt(np.sum(n * n)) if norm == "l2norm" else np.sum(per_slot, axis=1) / np.sum(n)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_scan(base, p.waveform_candidates_floating(5, ngroup, K, cand, **kw), slack, "isrc0 = 5")
        for piece in (1, 5):
            assert_same_scan(base, p.waveform_candidates_floating_params("moment_tensor", rows, K, cand, piece=piece, **kw), slack, "piece %d" % piece)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups: read at kiwi_hip_init
    sc, q = prepared()
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_scan(base, q.waveform_candidates_floating(0, ngroup, K, cand, **kw), slack, "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = prepared(engine=multi_engine(2))                  # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        assert_same_scan(base, m.waveform_candidates_floating_params("moment_tensor", rows, K, cand, **kw), slack, "two contexts")
        assert_same_scan(base, m.waveform_candidates_floating_params("moment_tensor", rows, K, cand, piece=2 * K, **kw), slack, "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ F7: a failed basis source
def test_a_failed_basis_source_gives_status_two():
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        p.set_misfit_method("floating_l1norm")
        set_ranges(p, dt, GRID_RANGES)
        # a basis source that fails to discretise ("Empty rupture area": above the constraining planes)
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (4, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((4, 6)) * 1e18
        eik[3, 3] = 500.0
        for piece in (0, 2):
            for norm in ("l1norm", "l2norm"):
                scan = p.waveform_candidates_floating_params("mt_eikonal", eik, 2, cand, outer_norm=norm, cand_shift=True, slot_misfit=True, piece=piece)
                assert scan.status[0] == 0 and scan.best_index[0] >= 0 and np.all(np.isfinite(scan.misfit[0]))
                assert scan.status[1] == 2 and scan.best_index[1] == -1 and np.isnan(scan.best_misfit[1]) and np.all(np.isnan(scan.misfit[1]))
                assert not np.any(scan.best_shift[1]) and not np.any(scan.cand_shift[1]) and not np.any(scan.slot_misfit[1]) and not np.any(scan.slot_norm[1])
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F8: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        dt = sc.gf["dt"]
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        p.set_misfit_method("floating_l1norm")
        set_ranges(p, dt, GRID_RANGES)
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

        def entry(match, K=6, ncand=5, x=cand, outer=2, slots=(False, False), isrc0=0, ngroup=2, params_form=True, null=None, cshift=False):
            """both C entries with these arguments: refused, with the reason in a message that starts with the call's name"""
            import ctypes
            bi, bm, st, bs = np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32), np.zeros(64, np.int32)
            sm = np.zeros(2 * 5 * 32, np.float32) if slots[0] else None
            sn = np.zeros(2 * 32, np.float32) if slots[1] else None
            cs = np.zeros(2 * 5 * 8, np.int16) if cshift else None
            x = None if null == "candidates" else np.ascontiguousarray(x, np.float64)
            tail = (ncand, dp(x), outer, None, 0, ip(None if null == "best_index" else bi), dp(None if null == "best_misfit" else bm),
                    ip(None if null == "status" else st), ip(None if null == "best_shift" else bs), None,
                    None if cs is None else cs.ctypes.data_as(ctypes.POINTER(ctypes.c_short)), fp(sm), fp(sn))
            rc = p.L.kiwi_hip_waveform_candidates_floating(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="waveform_candidates_floating: .*" + match):
                p._ck(rc, "waveform_candidates_floating")
            if params_form:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_waveform_candidates_floating_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="waveform_candidates_floating: .*" + match):
                    p._ck(rc, "waveform_candidates_floating")
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
        entry("a cand_shift array without a misfit array", cshift=True)
        for null in ("candidates", "best_index", "best_misfit", "status", "best_shift"):
            entry("null candidates, best_index, best_misfit, status or best_shift array", null=null)
        for K in (0, 9):
            entry("basis sources per group", K=K)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, params_form=False)
        # a shift range beyond 16 bits does not fit cand_shift; without cand_shift the call answers
        p.set_floating_shiftrange(2, 40000 * dt, 40004 * dt)
        with pytest.raises(KiwiHipError, match="waveform_candidates_floating: a shift range beyond 16 bits"):
            p.waveform_candidates_floating(0, 2, 6, cand, cand_shift=True)
        with pytest.raises(KiwiHipError, match="waveform_candidates_floating: a shift range beyond 16 bits"):
            p.waveform_candidates_floating_params("moment_tensor", rows, 6, cand, cand_shift=True)
        p.set_source_params("moment_tensor", rows)
        scan = p.waveform_candidates_floating(0, 2, 6, cand)
        assert np.all(scan.status == 0) and np.all((scan.best_shift[:, 1] >= 40000) & (scan.best_shift[:, 1] <= 40004))
        set_ranges(p, dt, GRID_RANGES)
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.waveform_candidates_floating(0, 2, 6, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.waveform_candidates_floating(0, 2, 6, cand[:, :5])
        with pytest.raises(KiwiHipError, match="no closed form"):
            mtfit.scan_double_couples_waveform_floating(p, "moment_tensor", rows[0], [0.], [45.], [90.], moment=None)
        # a method other than the floating ones: the message says where l1norm and l2norm go
        for method in ("l1norm", "l2norm", "ampspec_l1norm", "peak"):
            p.set_misfit_method(method)
            with pytest.raises(KiwiHipError, match="waveform_candidates_floating: the misfit method must be floating_l1norm or floating_l2norm .*"
                                                   "l1norm and l2norm go through kiwi_hip_waveform_candidates"):
                p.waveform_candidates_floating(0, 2, 6, cand)
            with pytest.raises(KiwiHipError, match="waveform_candidates_floating: the misfit method must be floating_l1norm or floating_l2norm"):
                p.waveform_candidates_floating_params("moment_tensor", rows, 6, cand)
            p.set_source_params("moment_tensor", rows)
        p.set_misfit_method("floating_l1norm")
        still_usable()
        assert np.all(p.waveform_candidates_floating(0, 2, 6, cand).status == 0)
        still_usable()
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
        q.set_misfit_method("floating_l1norm")
        q.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="waveform_candidates_floating: .*needs a reference seismogram"):
            q.waveform_candidates_floating(0, 2, 6, cand)
        with pytest.raises(KiwiHipError, match="waveform_candidates_floating: .*needs a reference seismogram"):
            q.waveform_candidates_floating_params("moment_tensor", rows, 6, cand)
        q.set_ref_seismogram(3, 2, *sc.refs[(3, 2)])
        q.set_source_params("moment_tensor", rows)
        scan = q.waveform_candidates_floating(0, 2, 6, cand)
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
        p.set_misfit_method("floating_l1norm")
        p.set_source_params("moment_tensor", rows)
        with pytest.raises(KiwiHipError, match="waveform_candidates_floating: an enabled receiver has no misfit taper"):
            p.waveform_candidates_floating(0, 2, 6, cand)
        p.switch_receiver(3, False)
        assert np.all(p.waveform_candidates_floating(0, 2, 6, cand).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ F9: helper, bootstrap, example
PLANTED_SDR = (60.0, 60.0, 90.0, 5e18)
PAD = 6


def test_helper_recovers_the_planted_mechanism_and_delays_with_one_glitched_station():
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted))
    e = sc.oracle()
    sc.make_references(e)
    rng = np.random.default_rng(12)
    for (ir, k), (lo, d) in list(sc.refs.items()):            # every station's data late by its delay, padded so that they cover the taper
        padded = np.zeros(len(d) + 2 * PAD)
        padded[PAD + DELAYS[ir - 1]:PAD + DELAYS[ir - 1] + len(d)] = d
        obs = (padded + 0.02 * np.std(d) * rng.standard_normal(len(padded))).astype(np.float32)
        if ir == 3:                                           # station 3: its data replaced by a glitch, a step of 20 times their size
            obs = (20.0 * np.max(np.abs(d)) * (np.arange(len(padded)) > len(padded) // 3)).astype(np.float32)
        sc.refs[(ir, k)] = (lo - PAD, obs)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        dt = sc.gf["dt"]
        p.set_misfit_method("floating_l1norm")
        set_ranges(p, dt, [(-4, 4)] * 6)
        row = mt_row(np.zeros(6))
        good = np.arange(6) != 2
        res = mtfit.scan_double_couples_waveform_floating(p, "moment_tensor", row, *GRID, moment=PLANTED_SDR[3], outer_norm="l1norm", cube=True)
        assert res["status"][0] == 0 and res["cube"].shape == (1, 12, 4, 12) and res["moment"][0] == PLANTED_SDR[3]
        assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR), (res["strike"], res["dip"], res["rake"])
        assert res["misfit"][0] == np.nanmin(res["cube"])
        assert list(np.rint(res["shifts"][0] / dt).astype(int)[good]) == [-d for d, g in zip(DELAYS, good) if g], res["shifts"]
        # a moment axis: the planted moment comes out first among three
        moments = (PLANTED_SDR[3], 0.5 * PLANTED_SDR[3], 2.0 * PLANTED_SDR[3])
        axis = mtfit.scan_double_couples_waveform_floating(p, "moment_tensor", row, *GRID, moment=moments, outer_norm="l1norm", cube=True)
        assert axis["cube"].shape == (1, 12, 4, 12, 3) and axis["cube_shifts"].shape == (1, 12, 4, 12, 3, 6)
        assert axis["moment"][0] == PLANTED_SDR[3] and axis["index"][0] == 3 * res["index"][0]
        assert np.array_equal(axis["cube"][..., 0], res["cube"]) and np.array_equal(axis["cube_shifts"][..., 0, :], res["cube_shifts"])
        # the bootstrap over the receivers through kiwi_hip_outer_misfits on the call's own slots: the planted mechanism is the mode
        draws = np.concatenate([np.ones((1, sc.nrec)), rng.multinomial(sc.nrec, np.full(sc.nrec, 1.0 / sc.nrec), 200).astype(np.float64)])
        boot = mtfit.scan_double_couples_waveform_floating(p, "moment_tensor", row, *GRID, moment=PLANTED_SDR[3], outer_norm="l1norm", bootstrap=draws)
        assert boot["boot_index"].shape == (1, 201) and boot["boot_index"][0, 0] == res["index"][0] and boot["boot_misfit"][0, 0] == res["misfit"][0]
        mode = int(np.bincount(boot["boot_index"][0][boot["boot_index"][0] >= 0]).argmax())
        sdr = mtfit.double_couple_candidates(*GRID)[1]
        assert same_mechanism(sdr[mode, 0], sdr[mode, 1], sdr[mode, 2], PLANTED_SDR), sdr[mode]
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_l1_station_shifts.py"), "--small"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism, depth and delays found" in out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
@pytest.mark.parametrize("norm", ["l1norm", "l2norm"])
def test_a_piece_in_which_every_basis_source_fails_to_discretise(norm):
    """three groups of two `mt_eikonal` basis sources in pieces of one group, both sources of the middle group failing to discretise:
    nothing is uploaded for that piece.  Its group reads as a failed group does, its neighbours as the call without it gives them"""
    sc, p = build(COMPS)
    try:
        p.set_misfit_method("floating_l1norm")
        set_ranges(p, sc.gf["dt"], GRID_RANGES)
        eik, good = eikonal_list_with_a_failed_piece(p)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        kw = dict(outer_norm=norm, cand_shift=True, slot_misfit=True, piece=2)
        got = p.waveform_candidates_floating_params("mt_eikonal", eik, 2, cand, **kw)
        assert list(got.status) == [0, 2, 0]
        assert got.best_index[1] == -1 and np.isnan(got.best_misfit[1]) and np.all(np.isnan(got.misfit[1]))
        assert not np.any(got.best_shift[1]) and not np.any(got.cand_shift[1])
        assert not np.any(got.slot_misfit[1]) and not np.any(got.slot_norm[1])
        assert_beside_a_failed_piece(got, p.waveform_candidates_floating_params("mt_eikonal", good, 2, cand, **kw), common.arith(), norm)
    finally:
        p.close()
