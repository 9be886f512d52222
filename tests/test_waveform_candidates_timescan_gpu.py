"""kiwi_hip_waveform_candidates_time_scan on the device: the rows, scan and fold kernels have the same BITS as the numpy
restatement (tests/waveform_candidates_timescan_restatement.py) fed with the call's own rows, whatever K, the number of groups, the
method, the outer norm, anarchy, the synthetics factor, the offsets against the pass and the number of candidates against the tile;
the rows are the parents' rows; unit candidates against kiwi_hip_time_scan; offset 0 against kiwi_hip_waveform_candidates; a
576-mechanism grid at five origin times against its syntheses; the same bits however the call is cut; the slot misfits through
kiwi_hip_outer_misfits; the refusals; the context afterwards; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_timescan_cases as lc
from tests import waveform_candidates_timescan_restatement as wtr
from tests.common import Scenario, misfit_close
from tests.linfit_cases import UNIT, device_traces, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups
from tests.test_waveform_candidates_gpu import GRID, NAMES, band, same, same_mechanism, slot_bound, slot_map, window, zero_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FIELDS = ("best_offset", "best_index", "best_misfit", "status", "cand_misfit", "cand_offset", "misfit", "slot_misfit", "slot_norm")
ALL = dict(misfit=True, slot_misfit=True)


def slots_of(sc, enabled):
    return [(ir + 1, k + 1) for ir, c in enumerate(sc.comps) if enabled[ir] for k in range(len(c))]


def references_and_tapers(p, sc, enabled):
    """(ref[m], taper[m]) float32 [wlen_m] of the enabled receivers' slots as the context holds them: the tapered references, and
    the taper weights read as the tapered reference of ones (fl(1 w) = w); the references are put back"""
    slots = slots_of(sc, enabled)
    plain = [p.get_reference(ir, k, 1, maxn=1 << 14) for ir, k in slots]
    tapered = [p.get_reference(ir, k, 2, maxn=1 << 14) for ir, k in slots]
    for (ir, k), (lo, d) in zip(slots, tapered):
        p.set_ref_seismogram(ir, k, lo - 5, np.ones(len(d) + 10, F32))
    taper = []
    for (ir, k), (lo, d) in zip(slots, tapered):
        lo1, w = p.get_reference(ir, k, 2, maxn=1 << 14)
        assert lo1 == lo and len(w) == len(d)
        taper.append(w)
    for (ir, k), (lo, d) in zip(slots, plain):
        p.set_ref_seismogram(ir, k, lo, d)
    for (ir, k), (lo, d) in zip(slots, tapered):
        assert np.array_equal(p.get_reference(ir, k, 2, maxn=1 << 14)[1], d)
    return [d for lo, d in tapered], taper


def raw_rows(scan, wlens):
    return wtr.raw_of(scan.rows, scan.row_offset, wlens, scan.shift_halo)


def same_scan(a, b, what, fields=FIELDS):
    for name in fields:
        same(getattr(a, name), b[name] if isinstance(b, dict) else getattr(b, name), what + " " + name)


def cut(rs, nk, ncand):
    """the restatement of the first nk offsets and the first ncand candidates from the slot misfits of more of both"""
    return rs[:, :nk, :ncand]


# ------------------------------------------------------------------------------------------------ G1: device == restatement
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_kernels_equal_the_restatement_bit_for_bit(K, ngroup):
    sc, p = build(COMPS, window=60)
    try:
        dt = sc.gf["dt"]
        C, S, J = p.waveform_candidates_time_scan_shape(K)
        assert C >= 64 and S >= 64 and J >= 8
        p.switch_receiver(6, False)                           # a disabled receiver,
        zero_reference(p, sc, 4)                              # one without reference energy,
        window(p, sc, 3, 45)                                  # one with a window inside one stage, the shortest,
        window(p, sc, 2, 2 * S + 37)                          # and one with a window of two stages and a part of a third
        w = np.array([0.0, 0.7, 2.5, 1.3, 1.0, 4.0])          # one of weight 0; the weight of the disabled receiver never counts
        enabled = [True] * 5 + [False]
        wz = np.where(enabled, w, 0.0)
        rec = slot_map(sc, enabled)
        ref, taper = references_and_tapers(p, sc, enabled)
        wlens = [len(r) for r in ref]
        assert min(wlens) == 45 and max(wlens) == 2 * S + 37, wlens
        rng = np.random.default_rng(10 * K + ngroup)
        tabs, moments, rises = lc.scattered_tables(rng, ngroup, K)           # fractional centroid times, rise times 0, 1, 2 s: folded
        p.set_sources(tabs, moments, rises)
        nc_all, nk_all = 2 * C + 3, 2 * J + 3
        cand = rng.uniform(-2.0, 2.0, (nc_all, K))
        cand[C - 1] = cand[2]                                 # equal misfits across a tile boundary
        cand[C] = cand[2]

        def check(method, factor, k0, kstep, nk, ncand, norm, anarchy, smis, raw):
            what = "K=%d ngroup=%d factor=%g %s %s anarchy=%s offsets (%d, %d, %d) ncand=%d" % (K, ngroup, factor, NAMES[method], norm, anarchy, k0, kstep, nk, ncand)
            scan = p.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, nk, cand[:ncand], outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                   rows=True, **ALL)
            for a, b in zip(raw_rows(scan, wlens), raw):
                same(a, b, what + " rows")
            rs = wtr.fold_offsets(cut(smis, nk, ncand), norm_of[0], rec, wz, anarchy, norm)
            same_scan(scan, rs, what)
            return scan

        norm_of = [None]
        for method, factor in ((2, 1.0), (1, 1.0), (2, 0.75)):
            p.set_synthetics_factor(factor)
            p.set_misfit_method(NAMES[method])
            for k0, kstep in {(2, 1.0): ((-3, 1), (0, 1), (-7, 3)), (1, 1.0): ((-7, 3),), (2, 0.75): ((-3, 1),)}[(method, factor)]:
                full = p.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, nk_all, cand, outer_norm="l2norm", receiver_weights=w, rows=True, **ALL)
                assert np.array_equal(full.slot_norm, np.array([p.get_misfits(g * K, 1)[1][0] for g in range(ngroup)]))
                norm_of[0] = full.slot_norm
                raw = raw_rows(full, wlens)
                assert full.shift_halo == max(abs(k0), abs(k0 + (nk_all - 1) * kstep))
                smis = wtr.slot_misfits_of(raw, taper, ref, cand, method, dt, full.shift_halo, wtr.offsets(k0, kstep, nk_all), factor)
                check(method, factor, k0, kstep, nk_all, nc_all, "l2norm", False, smis, raw)
                if (k0, kstep) != (-3, 1):
                    check(method, factor, k0, kstep, nk_all, C + 1, "l1norm", True, smis, raw)
                    continue
                scan = check(method, factor, k0, kstep, nk_all, nc_all, "l1norm", False, smis, raw)
                assert np.all(scan.status == 0) and np.all(scan.best_index >= 0) and np.all(scan.best_offset >= 0)
                assert np.all(scan.misfit[:, :, C - 1] == scan.misfit[:, :, 2]) and np.all(scan.misfit[:, :, C] == scan.misfit[:, :, 2])
                assert np.all(scan.slot_norm[:, [s for s, r in enumerate(rec) if r == 3]] == 0)
                check(method, factor, k0, kstep, nk_all, nc_all, "l1norm", True, smis, raw)
                check(method, factor, k0, kstep, nk_all, nc_all, "l2norm", True, smis, raw)
                if method == 2 and factor == 1.0:             # the offsets against the pass, the candidates against the tile
                    # (a shorter scan has a smaller halo: its rows are compared with the same samples of the longer one's)
                    for nk in (1, J - 1, J, J + 1):
                        Sn = max(abs(k0), abs(k0 + (nk - 1) * kstep))
                        rawn = [r[:, :, full.shift_halo - Sn:r.shape[2] - (full.shift_halo - Sn)] for r in raw]
                        for ncand in (1, C - 1, C, C + 1, nc_all):
                            check(method, factor, k0, kstep, nk, ncand, "l1norm", False, smis, rawn)
                    for ncand in (1, C - 1, C, C + 1):
                        check(method, factor, k0, kstep, nk_all, ncand, "l1norm", False, smis, raw)
                ms = p.waveform_candidates_time_scan_ms()
                assert len(ms) == 4 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0
            # offsets beyond the shortest window: every sample of it read from outside the window, on either side
            for k0 in (min(wlens) + 1, -min(wlens) - 2):
                big = p.waveform_candidates_time_scan(0, ngroup, K, k0, 1, 2, cand[:C + 1], outer_norm="l1norm", receiver_weights=w, rows=True, **ALL)
                rs = wtr.evaluate(raw_rows(big, wlens), taper, ref, norm_of[0], rec, wz, False, cand[:C + 1], method, "l1norm", dt, big.shift_halo,
                                  k0, 1, 2, factor)
                same_scan(big, rs, "K=%d ngroup=%d %s offsets (%d, 1, 2)" % (K, ngroup, NAMES[method], k0))
        p.set_synthetics_factor(1.0)
        # no receiver counts: status 1, NaN, no winner, no best offset; the arrays that are not asked for are not made
        scan = p.waveform_candidates_time_scan(0, ngroup, K, -1, 1, 3, cand[:3], receiver_weights=np.zeros(6), misfit=True)
        assert np.all(scan.status == 1) and np.all(scan.best_index == -1) and np.all(scan.best_offset == -1)
        assert np.all(np.isnan(scan.misfit)) and np.all(np.isnan(scan.best_misfit)) and np.all(scan.cand_offset == -1) and np.all(np.isnan(scan.cand_misfit))
        scan = p.waveform_candidates_time_scan(0, ngroup, K, -1, 1, 3, cand[:3], cand_misfit=False, cand_offset=False)
        assert scan.misfit is None and scan.slot_misfit is None and scan.slot_norm is None and scan.rows is None and scan.cand_misfit is None
        assert np.all(scan.status == 0) and np.all((scan.best_index >= 0) & (scan.best_index < 3)) and np.all((scan.best_offset >= 0) & (scan.best_offset < 3))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G2: the rows are the parents'
def test_rows_are_the_parents_rows():
    """fl(rows[S - k + i] taper[i]) is the kept tapered trace of kiwi_hip_linear_fit: at k = 0 on the same context, at k != 0 on
    the context with references and tapers moved by -k samples (route B of the linear fit's time scan)"""
    sc, p = lc.standard()
    try:
        K, ngroup = 6, 2
        enabled = [True] * 5 + [False]
        ref, taper = references_and_tapers(p, sc, enabled)
        wlens = [len(r) for r in ref]
        tabs, moments, rises = lc.scattered_tables(np.random.default_rng(23), ngroup, K)
        p.set_sources(tabs, moments, rises)
        p.set_misfit_method("l1norm")
        scan = p.waveform_candidates_time_scan(0, ngroup, K, -5, 5, 3, np.eye(K), rows=True)          # offsets -5, 0, 5
        raw, S = raw_rows(scan, wlens), scan.shift_halo
        assert S == 5 and all(r.shape == (ngroup, K, n + 2 * S) for r, n in zip(raw, wlens))
        p.set_misfit_method("l2norm")

        def kept():
            p.linear_fit(0, ngroup, K)
            return device_traces(p, sc.comps, enabled, 0, ngroup, K, 2)[0]
        for k, syn in zip((0, 5), lc.route_b(p, sc, (0, 5), kept)):
            for m, (r, t) in enumerate(zip(raw, taper)):
                same((r[:, :, S - k:S - k + len(t)] * t).astype(F32), syn[m], "offset %d slot %d" % (k, m))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G3: unit candidates
@pytest.mark.parametrize("method", [1, 2])
def test_unit_candidates_against_time_scan(method):
    """x = e_a gives u = row_a exactly, so the slot misfit at offset k is kiwi_hip_time_scan's of basis source a up to the order of
    the fp64 sum over the samples (a tree over 256 threads there, ascending here)"""
    sc, p = lc.standard()
    try:
        K, ngroup, (k0, kstep, nk) = 6, 2, (-7, 3, 6)
        p.set_misfit_method(NAMES[method])
        tabs, moments, rises = lc.scattered_tables(np.random.default_rng(3), ngroup, K)
        p.set_sources(tabs, moments, rises)
        ts_m, ts_n = p.time_scan(0, ngroup * K, k0, kstep, nk)[:2]
        scan = p.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, nk, np.eye(K), **ALL)
        m = ts_m.reshape(ngroup, K, nk, -1)                    # [group, source, offset, slot]
        n = ts_n.reshape(ngroup, K, -1)
        mine = np.moveaxis(scan.slot_misfit, 1, 2)            # [group, candidate = source, offset, slot]
        assert np.array_equal(scan.slot_norm, n[:, 0])
        rel = np.max(np.abs(mine.astype(np.float64) - m) / np.maximum(np.abs(m), 1e-30))
        print("%s: unit candidates against time_scan, largest relative difference %.3g (2^-23 = %.3g)" % (NAMES[method], rel, 2.0 ** -23))
        assert misfit_close(mine, m, norm=np.broadcast_to(n[:, :, None, :], m.shape))
        # K = 1, x = [1]: every source a group of its own
        one = p.waveform_candidates_time_scan(0, ngroup * K, 1, k0, kstep, nk, [[1.0]], **ALL)
        assert misfit_close(one.slot_misfit[:, :, 0], ts_m, norm=np.broadcast_to(ts_n[:, None, :], ts_m.shape))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G4: offset 0 against the plain call
@pytest.mark.parametrize("method", [1, 2])
def test_offset_zero_against_waveform_candidates(method):
    """not the same bits -- the plain call tapers every basis trace before combining, this one combines and tapers once --; both lie
    within slot_bound of the exact combination, so of each other"""
    sc, p = build(COMPS)
    try:
        K, ngroup, dt = 6, 2, sc.gf["dt"]
        p.set_misfit_method(NAMES[method])
        rng = np.random.default_rng(41)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        for norm in ("l1norm", "l2norm"):
            plain = p.waveform_candidates(0, ngroup, K, cand, outer_norm=norm, slot_misfit=True)
            scan = p.waveform_candidates_time_scan(0, ngroup, K, -2, 2, 3, cand, outer_norm=norm, **ALL)       # offsets -2, 0, 2
            syn, ref, _ = device_traces(p, sc.comps, [True] * 6, 0, ngroup, K, 2)
            assert np.array_equal(plain.slot_norm, scan.slot_norm) and np.array_equal(plain.status, scan.status)
            for g in range(ngroup):
                m, n = plain.slot_misfit[g].astype(np.float64), np.tile(plain.slot_norm[g].astype(np.float64), (len(cand), 1))
                bound = slot_bound(NAMES[method], dt, [s[g] for s in syn], ref, cand, m, n)
                dm = np.abs(scan.slot_misfit[g, 1].astype(np.float64) - m)
                print("%s %s group %d: offset 0 against the plain call, largest |dm| / bound %.3g" % (NAMES[method], norm, g, np.max(dm / bound)))
                assert np.all(dm <= bound)
            assert misfit_close(scan.misfit[:, 1], plain.misfit, glob=True)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G5: against syntheses
@pytest.mark.parametrize("method,norm", [(2, "l1norm"), (1, "l2norm")])
def test_the_mechanism_grid_at_five_origin_times_against_its_syntheses(method, norm):
    sc, p = build(None, planted=False)                        # data: the default bilateral rupture; 6 receivers x ned
    try:
        dt, K, moment = sc.gf["dt"], 6, 7e18
        assert dt == 0.5                                      # (time + k dt is exact in fp32)
        p.set_misfit_method(NAMES[method])
        row = mt_row(np.zeros(6))
        k0, kstep, nk = -4, 2, 5
        cand, sdr = mtfit.double_couple_candidates(*GRID, moment / UNIT)
        scan = p.waveform_candidates_time_scan_params("moment_tensor", mtfit.elementary_params("moment_tensor", row[None, :], UNIT), K, k0, kstep,
                                                      nk, cand, outer_norm=norm, rows=True, **ALL)
        assert p.nsrc == 6 and scan.status[0] == 0 and scan.slot_misfit.shape[:3] == (1, nk, 576)
        enabled = [True] * 6
        ref, taper = references_and_tapers(p, sc, enabled)
        raw, S = raw_rows(scan, [len(r) for r in ref]), scan.shift_halo
        rec = slot_map(sc, enabled)
        worst = 0.0
        for j, k in enumerate(wtr.offsets(k0, kstep, nk)):
            grid = np.array([mt_row(np.asarray(t * UNIT, np.float32), [row[0] + k * dt] + list(row[1:4]), row[10]) for t in cand], np.float32)
            m, n, _, status = p.misfits_for_params("moment_tensor", grid)
            assert not np.any(status) and np.array_equal(n[0], scan.slot_norm[0])
            g = p.outer_misfits_slots(m, n, rec, sc.nrec, outer_norm=norm, which_draw=0)[2]
            m, n = m.astype(np.float64), n.astype(np.float64)
            rows_k = [(r[0][:, S - k:S - k + len(t)] * t).astype(F32) for r, t in zip(raw, taper)]
            bound = slot_bound(NAMES[method], dt, rows_k, ref, cand, m, n)
            dm = np.abs(scan.slot_misfit[0, j].astype(np.float64) - m)
            worst = max(worst, float(np.max(dm / bound)))
            assert np.all(dm <= bound), (k, np.max(dm / bound))
            contract = common.arith()
            os.environ["KIWI_HIP_ARITH"] = "fused"            # the rule on the scale of the norm factors, for both contracts
            try:
                assert misfit_close(scan.misfit[0, j], g, glob=True)
            finally:
                os.environ["KIWI_HIP_ARITH"] = contract
        print("%s inside, %s outside: 576 double couples x 5 origin times, largest |dm| / bound %.3g" % (NAMES[method], norm, worst))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G6: the same bits however it is cut
def assert_same_cut(a, b, what):
    assert np.array_equal(a.status, b.status), what
    if common.arith() == "exact":
        same_scan(a, b, what)
        return
    # (fused: the batch shape chooses the accumulate kernel's instantiation, so the synthetics agree to SYN_RTOL only; the claim of
    # the same bits is the exact contract's)
    assert np.allclose(a.misfit, b.misfit, rtol=1e-3, atol=0, equal_nan=True), what


@pytest.mark.parametrize("method,norm", [(2, "l1norm"), (1, "l2norm")])
def test_first_source_chunks_pieces_contexts_and_split_offsets(method, norm, monkeypatch):
    ngroup, K, (k0, kstep, nk) = 12, 6, (-7, 3, 11)
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    kw = dict(outer_norm=norm, **ALL)

    def prepared(**more):
        sc, q = build(COMPS, window=150, **more)
        q.set_misfit_method(NAMES[method])
        return sc, q

    sc, p = prepared()
    try:
        p.set_source_params("moment_tensor", rows)
        base = p.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, nk, cand, **kw)
        assert np.all(base.status == 0)
        p.set_source_params("moment_tensor", np.concatenate([head, rows]))
        assert_same_cut(base, p.waveform_candidates_time_scan(5, ngroup, K, k0, kstep, nk, cand, **kw), "isrc0 = 5")
        # the offsets in two calls: the per-offset answers are those of the one call
        p.set_source_params("moment_tensor", rows)
        first = p.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, 4, cand, **kw)
        second = p.waveform_candidates_time_scan(0, ngroup, K, k0 + 4 * kstep, kstep, nk - 4, cand, **kw)
        if common.arith() == "exact":
            for name in ("best_index", "best_misfit", "misfit", "slot_misfit"):
                same(np.concatenate([getattr(first, name), getattr(second, name)], 1), getattr(base, name), "two calls " + name)
        for piece in (1, 5):
            assert_same_cut(base, p.waveform_candidates_time_scan_params("moment_tensor", rows, K, k0, kstep, nk, cand, piece=piece, **kw), "piece %d" % piece)
            assert p.nsrc == K
            p.eval()
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups: read at kiwi_hip_init
    sc, q = prepared()
    try:
        q.set_source_params("moment_tensor", rows)
        assert_same_cut(base, q.waveform_candidates_time_scan(0, ngroup, K, k0, kstep, nk, cand, **kw), "chunks")
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m = prepared(engine=multi_engine(2))                  # two contexts (stacked on device 0 where there is one device)
    try:
        assert m.ndevices() == 2
        assert_same_cut(base, m.waveform_candidates_time_scan_params("moment_tensor", rows, K, k0, kstep, nk, cand, **kw), "two contexts")
        assert_same_cut(base, m.waveform_candidates_time_scan_params("moment_tensor", rows, K, k0, kstep, nk, cand, piece=2 * K, **kw), "two contexts, pieces")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ G7: the fold is outer_misfits'
def test_slot_misfits_through_outer_misfits_reproduce_misfit():
    sc, p = build(COMPS)
    try:
        K, ngroup, nk = 6, 2, 4
        p.switch_receiver(6, False)
        zero_reference(p, sc, 4)
        w = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])
        rec = slot_map(sc, [True] * 5 + [False])
        p.set_misfit_method("l1norm")
        rng = np.random.default_rng(61)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (300, K))
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                scan = p.waveform_candidates_time_scan(0, ngroup, K, -2, 1, nk, cand, outer_norm=norm, receiver_weights=w, anarchy=anarchy, **ALL)
                for g in range(ngroup):
                    sm = scan.slot_misfit[g].reshape(nk * len(cand), -1)      # nk x ncand read as sources
                    bv, bi, gl = p.outer_misfits_slots(sm, np.tile(scan.slot_norm[g], (len(sm), 1)), rec, sc.nrec, outer_norm=norm,
                                                       receiver_weights=w, anarchy=anarchy, draw_weights=np.ones((1, sc.nrec)), which_draw=0)
                    same(scan.misfit[g].reshape(-1), gl, "%s anarchy=%s group %d" % (norm, anarchy, g))
                    jb = scan.best_offset[g]
                    assert bi[0] == jb * len(cand) + scan.best_index[g, jb] and bv[0] == scan.best_misfit[g, jb]
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G7b: a failed basis source
def test_a_failed_basis_source_gives_its_group_status_two():
    """three groups of two `mt_eikonal` basis sources, the middle group with a source that fails to discretise ("Empty rupture area":
    above the constraining planes): in one piece the kernels pass over the group inside a chunk; with pieces of one group and both
    of its sources failing, nothing is uploaded for it.  Either way the group reads as stated and its neighbours as without it"""
    sc, p = build(COMPS)
    try:
        K, (k0, kstep, nk) = 2, (-7, 3, 11)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, K))
        p.set_misfit_method("l1norm")
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (6, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((6, 6)) * 1e18
        kw = dict(rows=True, **ALL)
        for norm in ("l1norm", "l2norm"):
            alone = p.waveform_candidates_time_scan_params("mt_eikonal", eik[[0, 1, 4, 5]], K, k0, kstep, nk, cand, outer_norm=norm, **kw)
            assert np.all(alone.status == 0) and np.all(alone.best_offset >= 0)
            bad = eik.copy()
            for piece in (0, 2):
                bad[3, 3] = 500.0
                if piece == 2:
                    bad[2, 3] = 500.0                         # a piece in which nothing could be discretised: nothing is uploaded for it
                got = p.waveform_candidates_time_scan_params("mt_eikonal", bad, K, k0, kstep, nk, cand, outer_norm=norm, piece=piece, **kw)
                what = "%s piece %d" % (norm, piece)
                assert list(got.status) == [0, 2, 0], what
                assert got.best_offset[1] == -1 and np.all(got.best_index[1] == -1) and np.all(got.cand_offset[1] == -1), what
                assert np.all(np.isnan(got.best_misfit[1])) and np.all(np.isnan(got.misfit[1])) and np.all(np.isnan(got.cand_misfit[1])), what
                assert not np.any(got.slot_misfit[1]) and not np.any(got.slot_norm[1]) and not np.any(got.rows[1]), what
                assert got.shift_halo == alone.shift_halo and np.array_equal(got.row_offset, alone.row_offset)
                good = type(got)(*[f[[0, 2]] if isinstance(f, np.ndarray) and name != "row_offset" else f for name, f in zip(got._fields, got)])
                assert_same_cut(alone, good, what + ": the groups beside the failed one")
                if common.arith() == "exact":
                    same(good.rows, alone.rows, what + " rows")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G8: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
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

        def refused(match, scan=(0, 1, 2), K=6, ngroup=2, isrc0=0, x=cand, listed=True, same_setup=True, **kw):
            with pytest.raises(KiwiHipError, match="waveform_candidates_time_scan: .*" + match):
                p.waveform_candidates_time_scan(isrc0, ngroup, K, *scan, x, **kw)
            if listed:
                with pytest.raises(KiwiHipError, match="waveform_candidates_time_scan: .*" + match):
                    p.waveform_candidates_time_scan_params("moment_tensor", rows, K, *scan, x, **kw)
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)
            if same_setup:
                still_usable()

        # what kiwi_hip_time_scan refuses of the offsets
        refused("need at least one offset", scan=(0, 1, 0))
        refused("at most %d are supported" % p.L.kiwi_hip_time_scan_max_offsets(), scan=(0, 1, p.L.kiwi_hip_time_scan_max_offsets() + 1))
        refused("at least one sample", scan=(0, 0, 3))
        refused("the largest shift is", scan=(-p.L.kiwi_hip_time_scan_max_shift() - 1, 1, 2))
        refused("the largest shift is", scan=(0, 600, 3))
        # what kiwi_hip_waveform_candidates refuses
        x = cand.copy()
        x[3, 2] = np.nan
        refused("entry 2 of candidate 3 is not finite", x=x)
        refused("not inside the uploaded batch", ngroup=3, listed=False)
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand[:, :5])
        # this call's own
        refused("a cand_offset array without cand_misfit", cand_misfit=False, cand_offset=True)
        L = p.L
        bo, bi, bm, st = np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros(4), np.zeros(2, np.int32)
        sm = np.zeros(2 * 2 * 5 * 32, F32)
        xs = np.ascontiguousarray(cand)
        rc = L.kiwi_hip_waveform_candidates_time_scan(p.h, 0, 2, 6, 0, 1, 2, 5, xs.ctypes.data_as(c_double_p), 1, None, 0, bo.ctypes.data_as(c_int_p),
                                                      bi.ctypes.data_as(c_int_p), bm.ctypes.data_as(c_double_p), st.ctypes.data_as(c_int_p), None, None,
                                                      None, sm.ctypes.data_as(c_float_p), None, None)
        assert rc != 0
        with pytest.raises(KiwiHipError, match="waveform_candidates_time_scan: a slot_misfit array without slot_norm"):
            p._ck(rc, "waveform_candidates_time_scan")
        rc = L.kiwi_hip_waveform_candidates_time_scan(p.h, 0, 2, 6, 0, 1, 2, 5, xs.ctypes.data_as(c_double_p), 1, None, 0, None,
                                                      bi.ctypes.data_as(c_int_p), bm.ctypes.data_as(c_double_p), st.ctypes.data_as(c_int_p), None, None,
                                                      None, None, None, None)
        assert rc != 0
        with pytest.raises(KiwiHipError, match="waveform_candidates_time_scan: null best_offset array"):
            p._ck(rc, "waveform_candidates_time_scan")
        still_usable()
        with pytest.raises(KiwiHipError, match="no closed form under"):
            mtfit.scan_double_couples_waveform_time_scan(p, "moment_tensor", rows[0], [0.], [45.], [90.], None, 0, 1, 2)
        # a method other than l1norm or l2norm
        for method in ("ampspec_l1norm", "floating_l1norm", "peak"):
            p.set_misfit_method(method)
            refused("the misfit method must be l1norm or l2norm", same_setup=False)
        p.set_misfit_method("l1norm")
        still_usable()
        # a receiver with a misfit filter: the message says why
        p.set_misfit_filter(3, *band(sc.gf["dt"]))
        refused("has a misfit filter; the taper sits in front of the filter, so every candidate and offset would need a transform of its own",
                same_setup=False)
        p.eval()
        assert np.all(np.isfinite(p.get_misfits()[0]))
        p.switch_receiver(3, False)
        assert np.all(p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand).status == 0)       # (the filter of a disabled receiver does not count)
    finally:
        p.close()
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
        with pytest.raises(KiwiHipError, match="waveform_candidates_time_scan: an enabled receiver has no misfit taper"):
            p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand)
        p.switch_receiver(3, False)
        assert np.all(p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand).status == 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G9: the context afterwards
def test_context_afterwards():
    """after the call an evaluation on the context gives the bits it gave before (the halo and the per-source strip spans are put
    back), and the evaluation the call leaves is offset 0's plain one"""
    sc, p = build(COMPS)
    try:
        K, ngroup = 6, 3
        p.set_misfit_method("l1norm")
        rows = colocated_groups(np.random.default_rng(3), ngroup, K)
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        plain = p.waveform_candidates(0, ngroup, K, np.eye(K), slot_misfit=True)
        p.waveform_candidates_time_scan(0, ngroup, K, -40, 20, 5, np.eye(K))
        for a, b in zip(before, p.get_misfits()):             # what the call left: the plain evaluation of the basis sources
            assert misfit_close(b, a, norm=before[1]) if a.ndim == 2 else misfit_close(b, a, glob=True)
        p.eval()
        for a, b in zip(before, p.get_misfits()):
            assert np.array_equal(a, b)
        again = p.waveform_candidates(0, ngroup, K, np.eye(K), slot_misfit=True)
        for name in ("best_index", "best_misfit", "misfit", "slot_misfit", "slot_norm", "status"):
            same(getattr(again, name), getattr(plain, name), name)
        # a refused call and a call that threw put the halo back as well
        with pytest.raises(KiwiHipError):
            p.waveform_candidates_time_scan(0, ngroup + 1, K, -40, 20, 5, np.eye(K))
        p.eval()
        for a, b in zip(before, p.get_misfits()):
            assert np.array_equal(a, b)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ G10: helper and example
PLANTED_SDR = (60.0, 60.0, 90.0, 5e18)


def test_helper_recovers_the_planted_mechanism_and_offset_under_a_glitch():
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted, location=[1.5, 0., 0., 10000.]))       # three samples later
    e = sc.oracle()
    sc.make_references(e)
    assert sc.gf["dt"] == 0.5
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
        res = mtfit.scan_double_couples_waveform_time_scan(p, "moment_tensor", row, *GRID, PLANTED_SDR[3], -4, 1, 9, outer_norm="l1norm", cube=True)
        assert res["status"][0] == 0 and res["cube"].shape == (1, 9, 12, 4, 12) and res["moment"][0] == PLANTED_SDR[3]
        assert res["offset"][0] == 7 and res["time_shift"][0] == 1.5, (res["offset"], res["offsets_misfit"])
        assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR), (res["strike"], res["dip"], res["rake"])
        assert res["misfit"][0] == np.nanmin(res["cube"]) == res["offsets_misfit"][0, 7]
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_l1_timescan.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "planted mechanism, depth and origin time found" in out.stdout
