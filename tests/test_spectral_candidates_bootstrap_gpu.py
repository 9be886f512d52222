"""kiwi_hip_spectral_candidates_bootstrap on the device.  The yardstick is the host route that defines the call, on the same
context and the same uploaded batch: `spectral_candidates(..., slot_misfit=True)`, then `Engine.outer_misfits_slots` on its float
arrays read as ngroup x ncand sources of nmis slots -- once for all groups (best_*), once per group (group_*).  Bit for bit,
whatever the number of candidates against the kernels' tile, of draws against the draw tile, of kept bins against the LDS stage, of
receivers against the LDS layout, and however the call is cut into chunks, draw passes, pieces and devices; also against the numpy
restatement fed with the parent's spectra; failed basis sources; refusals; the parent call untouched; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_bootstrap_cases as bc
from tests import spectral_candidates_bootstrap_restatement as sbr
from tests import spectral_candidates_restatement as sr
from tests.common import Scenario
from tests.linfit_cases import PLANTED, eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups
from tests.test_spectral_candidates_gpu import GRID, NAMES, PLANTED_SDR, band, long_reference, same_mechanism, short_taper, slot_map, zero_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts
ENABLED = [True] * 5 + [False]
FILTERED = (1, 3, 5)                                          # receivers (1-based) with a pass band; the others have none


def standard(method=3, engine=None, two_lengths=True):
    """tests/test_spectral_candidates_gpu.py's set-up: six receivers of 1 to 5 components, receiver 6 disabled, receiver 4 with
    references of zeros, a pass band on three of them, receiver 5 with longer transforms and a short window; WEIGHTS gives
    receiver 2 the weight 0"""
    sc, p = build(COMPS, engine=engine)
    p.switch_receiver(6, False)
    zero_reference(p, sc, 4)
    if two_lengths:
        long_reference(p, sc, 5)
        short_taper(p, sc, 5)
    for ir in FILTERED:
        p.set_misfit_filter(ir, *band(sc.gf["dt"]))
    p.set_misfit_method(NAMES[method])
    return sc, p


def draws_of(nrec, ndraw, counted, skipped, seed=0):
    """bc.draw_rows (ones, zeros, non-zero only on skipped receivers, then resampled) with one one-hot row per receiver behind the
    first three: they pin every receiver's sums over its slots"""
    dw = bc.draw_rows(nrec, max(ndraw, 3 + nrec), counted, skipped, seed=seed)
    dw[3:3 + nrec] = np.eye(nrec)
    return dw[:ndraw]


def host_route(p, rec, nrec, isrc0, ngroup, K, cand, dw, outer_norm, w, anarchy):
    """what the library offered before: the parent call's slot arrays downloaded, then kiwi_hip_outer_misfits on them"""
    scan = p.spectral_candidates(isrc0, ngroup, K, cand, outer_norm=outer_norm, receiver_weights=w, anarchy=anarchy, misfit=False, slot_misfit=True)

    def outer(mis, nor, slots, nrec_, norm, w_, an, draws):
        return p.outer_misfits_slots(mis, nor, slots, nrec_, outer_norm=norm, receiver_weights=w_, anarchy=an, draw_weights=draws)
    return sbr.from_slots(scan.slot_misfit, scan.slot_norm, rec, nrec, scan.status, dw, outer_norm, w, anarchy, outer=outer), scan


# ------------------------------------------------------------------------------------------------ 1: device == host route
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_device_equals_host_route_bit_for_bit(K, ngroup):
    sc, p = standard()
    try:
        C, T, Rmax = p.spectral_candidates_bootstrap_shape(K)
        assert (C, T, Rmax) == (256, 16, 70)
        rec = slot_map(sc, ENABLED)
        assert sorted(set(np.bincount(rec))) == [1, 2, 3, 4, 5]      # receivers of 1 to 5 slots: the slot fold
        rng = np.random.default_rng(50 * K + ngroup)
        rows = colocated_groups(rng, ngroup, K)
        if ngroup == 3:
            rows[2 * K:] = rows[:K]                           # two groups with identical rows: a tie across groups
        p.set_source_params("moment_tensor", rows)
        cand = rng.uniform(-2.0, 2.0, (600, K))
        cand[C - 1] = cand[2]                                 # a tie across a tile boundary... (C - 1 is the last lane of tile 0)
        cand[C] = cand[2]                                     # ... and with the first lane of tile 1
        dw = draws_of(sc.nrec, 40, [0, 2, 4], [3, 5], seed=K)
        ncalls = 0
        for method, factor in ((3, 1.0), (4, 1.0), (3, 0.75), (4, 0.75)):
            p.set_synthetics_factor(factor)
            p.set_misfit_method(NAMES[method])
            whole = factor == 1.0                             # every cut of the work at factor 1; the other factor at the largest shape
            for ncand in (1, C - 1, C, C + 1, 600) if whole else (600,):
                for norm in ("l1norm", "l2norm"):
                    for anarchy in (False, True):
                        for w in (WEIGHTS, None):
                            kw = dict(outer_norm=norm, receiver_weights=w, anarchy=anarchy)
                            want, scan = host_route(p, rec, sc.nrec, 0, ngroup, K, cand[:ncand], dw, norm, w, anarchy)
                            for ndraw in ((1, T - 1, T, T + 1, 40) if w is not None and whole and method == 3 else (40,)):
                                got = p.spectral_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw[:ndraw], per_group=True, **kw)
                                what = "K=%d ngroup=%d %s x %g ncand=%d %s anarchy=%s weights=%s ndraw=%d" % (
                                    K, ngroup, NAMES[method], factor, ncand, norm, anarchy, w is not None, ndraw)
                                bc.assert_boot(got, want, what, ndraw, same_batch=True)
                                ncalls += 1
                                assert np.array_equal(got.status, scan.status) and np.all(got.status == 0), what      # the parent's status
                                assert not np.isnan(got.best_value[0]) and got.best_cand[0] >= 0, what        # the row of ones
                                if ndraw >= 3:                # all zeros; non-zero only on skipped receivers
                                    assert np.all(np.isnan(got.best_value[1:3])) and np.all(got.best_group[1:3] == -1), what
                                    assert np.all(got.best_cand[1:3] == -1), what
                                    assert np.all(np.isnan(got.group_value[:, 1:3])) and np.all(got.group_cand[:, 1:3] == -1), what
                                if ndraw >= 9:                # the one-hot rows: a counted receiver alone gives a value
                                    assert not np.isnan(got.best_value[3]) and not np.isnan(got.best_value[5]), what
                                assert np.all(got.best_cand != C - 1) and np.all(got.best_cand != C), what      # the lowest index of a tie
                                assert np.all(got.best_group != 2), what                                        # the lower group of a tie
                                if ngroup == 3:
                                    assert np.array_equal(got.group_value[0], got.group_value[2], equal_nan=True), what
                            got = p.spectral_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw, **kw)
                            assert got.group_value is None and got.group_offset is None and got.group_cand is None
                            bc.assert_boot(got, want, "no group arrays", same_batch=True)
        # no receiver counts: the parent's status 1, and no best in any draw
        p.set_synthetics_factor(1.0)
        none = p.spectral_candidates_bootstrap(0, ngroup, K, cand[:3], dw, receiver_weights=np.zeros(6), per_group=True)
        assert np.all(none.status == 1) and np.all(np.isnan(none.best_value)) and np.all(none.best_cand == -1) and np.all(none.group_cand == -1)
        assert np.array_equal(none.status, p.spectral_candidates(0, ngroup, K, cand[:3], receiver_weights=np.zeros(6)).status)
        ms = p.spectral_candidates_bootstrap_ms()
        assert len(ms) == 5 and all(t > 0 for t in ms[:4]) and ms[4] >= 0
        print("K=%d ngroup=%d: %d device calls against the host route" % (K, ngroup, ncalls))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: kept bins around the LDS stage
def test_kept_bins_around_the_lds_stage():
    """Green's functions of 120 samples: transforms of 256 samples, 129 bins without a filter -- one more than a stage of 128 holds.
    Receiver 1 keeps a handful of bins, receiver 3 none at all (its pass band lies between two bins), receiver 5 a band of some
    tens."""
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(PLANTED), L=120)
    sc.make_references(sc.oracle())
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        dt, K, ngroup = sc.gf["dt"], 6, 2
        C, B, _ = p.spectral_candidates_shape(K, context=False)
        assert B == 128
        nyq = 0.5 / dt
        p.set_misfit_filter(1, [c * nyq for c in (0.20, 0.21, 0.22, 0.23)], [0., 1., 1., 0.])
        p.set_misfit_filter(3, [c * nyq for c in (0.2005, 0.2010, 0.2015, 0.2020)], [0., 1., 1., 0.])
        p.set_misfit_filter(5, *band(dt))
        rec = slot_map(sc, [True] * 6)
        rng = np.random.default_rng(2)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = draws_of(sc.nrec, 20, range(6), [], seed=2)
        for method in (3, 4):
            p.set_misfit_method(NAMES[method])
            full = p.spectral_candidates(0, ngroup, K, cand[:2], outer_norm="l2norm", spectra=True)
            kept = full.spectra_range[0, :, 1] - full.spectra_range[0, :, 0] + 1
            assert np.all(full.spectra_range[..., 2] == 2 * B), full.spectra_range[0]
            per_rec = {r: set(int(k) for k, rr in zip(kept, rec) if rr == r) for r in range(6)}
            print(NAMES[method], "kept bins per receiver:", per_rec)
            assert per_rec[1] == per_rec[3] == per_rec[5] == {B + 1}             # no filter: one bin more than a stage
            assert all(1 <= k <= 8 for k in per_rec[0]) and per_rec[2] == {0} and all(8 < k < B for k in per_rec[4])
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    want, scan = host_route(p, rec, sc.nrec, 0, ngroup, K, cand, dw, norm, None, anarchy)
                    got = p.spectral_candidates_bootstrap(0, ngroup, K, cand, dw, outer_norm=norm, anarchy=anarchy, per_group=True)
                    bc.assert_boot(got, want, "stage %s %s anarchy=%s" % (NAMES[method], norm, anarchy), same_batch=True)
                    assert np.array_equal(got.status, scan.status)
                    assert not np.any(scan.slot_misfit[:, :, [m for m, r in enumerate(rec) if r == 2]])      # no kept bins: slot misfit 0
                    assert not np.isnan(got.best_value[3 + 1])                                                # the one-hot row of receiver 2
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: index plumbing
def test_the_planted_candidate_wins_wherever_it_stands():
    sc, p = build(COMPS)                                      # (every reference is the planted tensor's: its misfit is rounding)
    try:
        p.switch_receiver(6, False)
        for ir in FILTERED:
            p.set_misfit_filter(ir, *band(sc.gf["dt"]))
        K, ncand = 6, 600
        rng = np.random.default_rng(3)
        rows = colocated_groups(rng, 2, K)
        p.set_source_params("moment_tensor", rows)
        good = np.linalg.solve(rows[:K, 4:10].astype(np.float64).T, mt_row(PLANTED)[4:10].astype(np.float64))      # the planted tensor in group 0's basis
        poor = rng.uniform(-2.0, 2.0, (ncand, K))
        dw = draws_of(sc.nrec, 12, [0, 2, 4], [3, 5], seed=3)
        for method in (3, 4):
            p.set_misfit_method(NAMES[method])
            for at in (0, 63, 64, 255, 256, ncand - 1):
                cand = poor.copy()
                cand[at] = good
                got = p.spectral_candidates_bootstrap(0, 2, K, cand, dw, outer_norm="l1norm", receiver_weights=WEIGHTS, per_group=True)
                assert got.best_group[0] == 0 and got.best_cand[0] == at and got.group_cand[0, 0] == at, (NAMES[method], at, got.best_cand[0])
                assert got.best_value[0] < 1e-3 and np.all(got.best_cand[got.best_cand >= 0] == at)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: device == restatement
def test_device_equals_restatement_fed_with_the_parents_spectra():
    K, ngroup = 6, 2
    sc, p = standard()
    try:
        dt = sc.gf["dt"]
        rec = slot_map(sc, ENABLED)
        has_filter = [r + 1 in FILTERED for r in rec]
        wz = np.where(ENABLED, WEIGHTS, 0.0)
        rng = np.random.default_rng(78)
        p.set_source_params("moment_tensor", colocated_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (40, K))
        dw = draws_of(sc.nrec, 20, [0, 2, 4], [3, 5], seed=9)
        for method, factor in ((3, 1.0), (4, 0.75)):
            p.set_misfit_method(NAMES[method])
            p.set_synthetics_factor(factor)
            full = p.spectral_candidates(0, ngroup, K, cand[:1], outer_norm="l2norm", receiver_weights=WEIGHTS, slot_misfit=True, spectra=True)
            groups = sr.groups_from_scan(full, has_filter)
            cache = {}
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    rs = sbr.from_spectra(groups, rec, sc.nrec, wz, anarchy, cand, method, norm, dt, dw, syn_factor=factor, cache=cache)
                    got = p.spectral_candidates_bootstrap(0, ngroup, K, cand, dw, outer_norm=norm, receiver_weights=WEIGHTS, anarchy=anarchy,
                                                          per_group=True)
                    bc.assert_boot(got, rs, "restatement %s x %g, %s anarchy=%s" % (NAMES[method], factor, norm, anarchy), same_batch=True)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 5: the LDS layout
def test_the_most_receivers_are_accepted_and_one_more_is_refused():
    from tests.test_waveform_candidates_bootstrap_gpu import wide_scenario
    for nrec in (70, 71):
        sc = wide_scenario(nrec)
        p = sc.product()
        sc.apply_setup(p, False)
        try:
            assert p.spectral_candidates_bootstrap_shape(6)[2] == 70 and p.outer_max_receivers() > 71
            p.set_misfit_method("ampspec_l1norm")
            p.set_misfit_filter(nrec, *band(sc.gf["dt"]))
            p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(nrec), 2, 6))
            cand = np.random.default_rng(2).uniform(-2.0, 2.0, (70, 6))
            if nrec == 71:
                with pytest.raises(KiwiHipError, match=r"nok > spectral_candidates_bootstrap: 71 receivers.*at most 70"):
                    p.spectral_candidates_bootstrap(0, 1, 6, cand[:3], np.ones((2, 71)))
                p.eval()
                assert np.all(p.get_misfits()[0] > 0)
                continue
            p.switch_receiver(3, False)
            rec = slot_map(sc, [r != 2 for r in range(nrec)])
            w = np.random.default_rng(1).uniform(0.5, 2.0, nrec)
            w[nrec - 2] = 0.0
            dw = bc.draw_rows(nrec, 33, [r for r in range(nrec) if r not in (2, nrec - 2)], [2, nrec - 2], seed=1)
            dw[3] = 0.0
            dw[3, nrec - 1] = 1.0                             # the last receiver alone decides
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    want, scan = host_route(p, rec, nrec, 0, 2, 6, cand, dw, norm, w, anarchy)
                    got = p.spectral_candidates_bootstrap(0, 2, 6, cand, dw, outer_norm=norm, receiver_weights=w, anarchy=anarchy, per_group=True)
                    bc.assert_boot(got, want, "%d receivers %s anarchy=%s" % (nrec, norm, anarchy), same_batch=True)
                    assert not np.any(np.isnan(got.best_value[3:])) and np.all(np.isnan(got.best_value[1:3]))
                    last = scan.slot_misfit[..., -1].astype(np.float64) / scan.slot_norm[:, None, -1].astype(np.float64)
                    assert np.isclose(got.best_value[3], np.min(last), rtol=1e-12)
        finally:
            p.close()


# ------------------------------------------------------------------------------------------------ 6: however it is cut
PASS_NDRAW = 30000                                            # 3 tiles x 30000 draws x 12 bytes: one group's slab above 1 MiB


def test_first_source_pieces_chunks_draw_passes_and_contexts(monkeypatch):
    ngroup, K = 12, 6
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    as_dict = lambda s: {name: getattr(s, name) for name in s._fields}      # noqa: E731
    exact = common.arith() == "exact"
    base, passes = {}, {}
    sc, p = standard(two_lengths=False)
    try:
        C, T, _ = p.spectral_candidates_bootstrap_shape(K)
        rec = slot_map(sc, ENABLED)
        dw = draws_of(sc.nrec, 40, range(5), [5], seed=3)
        pdw = bc.draw_rows(sc.nrec, PASS_NDRAW, range(5), [5], seed=4)
        pc = bc.pass_candidates(C)
        assert ((len(pc) + C - 1) // C) * 12 * PASS_NDRAW > 1 << 20
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            p.set_source_params("moment_tensor", rows)
            b = base[norm] = p.spectral_candidates_bootstrap(0, ngroup, K, cand, dw, **kw)
            bc.assert_boot(b, host_route(p, rec, sc.nrec, 0, ngroup, K, cand, dw, norm, None, True)[0], "base " + norm, same_batch=True)
            print(norm, "winners of the draws (group, candidate):", sorted(set(zip(b.best_group[3:], b.best_cand[3:]))))
            p.set_source_params("moment_tensor", np.concatenate([head, rows]))
            got = p.spectral_candidates_bootstrap(5, ngroup, K, cand, dw, **kw)
            if exact:
                bc.assert_boot(got, as_dict(b), "isrc0 = 5")
            for piece in (K, 5 * K, 0):
                got = p.spectral_candidates_bootstrap_params("moment_tensor", rows, K, cand, dw, piece=piece, **kw)
                assert np.array_equal(got.status, b.status)
                if exact:
                    bc.assert_boot(got, as_dict(b), "piece %d" % piece)
                assert p.nsrc == (piece or p.nsrc)
                p.eval()                                      # the engine holds the head of the list and knows how long it is
            # the case whose draws go in passes below, here in one pass, against the host route
            p.set_source_params("moment_tensor", bc.pass_rows())
            passes[norm] = p.spectral_candidates_bootstrap(0, bc.PASS_GROUPS, 6, pc, pdw, **kw)
            bc.assert_boot(passes[norm], host_route(p, rec, sc.nrec, 0, bc.PASS_GROUPS, 6, pc, pdw, norm, None, True)[0], "one pass " + norm,
                           same_batch=True)
    finally:
        p.close()
    # several chunks, several draw passes: KIWI_HIP_CHUNK_MB is read when a context is made
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")
    sc, q = standard(two_lengths=False)
    try:
        for norm, b in base.items():
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            q.set_source_params("moment_tensor", rows)
            got = q.spectral_candidates_bootstrap(0, ngroup, K, cand, dw, **kw)
            assert np.array_equal(got.status, b.status)
            if exact:
                bc.assert_boot(got, as_dict(b), "chunks " + norm)
            q.set_source_params("moment_tensor", bc.pass_rows())
            got = q.spectral_candidates_bootstrap(0, bc.PASS_GROUPS, 6, pc, pdw, **kw)
            if exact:
                bc.assert_boot(got, as_dict(passes[norm]), "draw passes " + norm)
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = standard(two_lengths=False, engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        for norm, b in base.items():
            for piece in (0, 2 * K):
                got = m2.spectral_candidates_bootstrap_params("moment_tensor", rows, K, cand, dw, piece=piece, outer_norm=norm, anarchy=True,
                                                              per_group=True)
                assert np.array_equal(got.status, b.status)
                if exact:
                    bc.assert_boot(got, as_dict(b), "two contexts, piece %d" % piece)
    finally:
        m2.close()


# ------------------------------------------------------------------------------------------------ 7: failed basis sources
@pytest.mark.parametrize("method", [3, 4])
def test_a_group_with_a_failed_basis_source_never_wins(method):
    """three groups of two `mt_eikonal` sources, the middle group failing to discretise: in pieces of one group nothing is uploaded
    for it; in one piece (and with one source failing only) it is a failed group inside an uploaded batch"""
    sc, p = build(COMPS)
    try:
        p.set_misfit_method(NAMES[method])
        p.set_misfit_filter(1, *band(sc.gf["dt"]))
        eik, good = eikonal_list_with_a_failed_piece(p)
        one = eik.copy()
        one[2, 3] = eik[0, 3]                                 # source 2 (the first of the middle group) discretises, source 3 does not
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        dw = draws_of(sc.nrec, 12, range(6), [], seed=6)
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, per_group=True)
            alone = p.spectral_candidates_bootstrap_params("mt_eikonal", good, 2, cand, dw, **kw)
            assert np.all(alone.status == 0)
            for piece, lst in ((2, eik), (0, eik), (0, one)):
                got = p.spectral_candidates_bootstrap_params("mt_eikonal", lst, 2, cand, dw, piece=piece, **kw)
                what = "%s %s piece %d" % (NAMES[method], norm, piece)
                assert list(got.status) == [0, 2, 0], what
                assert np.all(np.isnan(got.group_value[1])) and np.all(got.group_cand[1] == -1), what
                assert np.all(got.best_group != 1), what
                for g, ga in ((0, 0), (2, 1)):                # the neighbours answer as without it
                    assert np.array_equal(np.isnan(got.group_value[g]), np.isnan(alone.group_value[ga])), what
                    if common.arith() == "exact":
                        assert np.array_equal(got.group_value[g], alone.group_value[ga], equal_nan=True), what
                        assert np.array_equal(got.group_cand[g], alone.group_cand[ga]), what
                two = np.where(got.group_value[2] < got.group_value[0], 2, 0)
                has = ~np.isnan(got.best_value)
                assert np.array_equal(got.best_group[has], two[has]), what
                assert np.array_equal(got.best_value, np.fmin(got.group_value[0], got.group_value[2]), equal_nan=True), what
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 8: refusals; the parent untouched
def test_refusals_name_the_reason_and_leave_the_context_and_the_parent_call_as_they_were():
    sc, p = standard(two_lengths=False)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        dw = draws_of(sc.nrec, 10, range(5), [5])
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        parent_kw = dict(outer_norm="l2norm", receiver_weights=WEIGHTS, slot_misfit=True, spectra=True)
        parent_before = p.spectral_candidates(0, 2, 6, cand, **parent_kw)
        left = p.get_misfits()
        boot_before = p.spectral_candidates_bootstrap(0, 2, 6, cand, dw, per_group=True)
        for x, y in zip(left, p.get_misfits()):               # afterwards the context is what the parent call leaves
            assert np.array_equal(x, y)
        parent_after = p.spectral_candidates(0, 2, 6, cand, **parent_kw)
        for name in parent_before._fields:                    # the parent call on the same context: identical arrays
            x, y = getattr(parent_before, name), getattr(parent_after, name)
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)
            again = p.spectral_candidates_bootstrap(0, 2, 6, cand, dw, per_group=True)
            for name in again._fields:
                assert np.array_equal(getattr(again, name), getattr(boot_before, name), equal_nan=True), name

        still_usable()
        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)               # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=1, isrc0=0, ngroup=2, listed=True, ndraw=10, draws=dw, weights=None, groups=(True, True),
                  null=None):
            """both C entries with these arguments: refused, with the call's name in front and the reason in the message"""
            bv, bg, bcd, st = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(8, np.int32)
            gv, gc = np.zeros(512), np.zeros(512, np.int32)
            x = np.ascontiguousarray(x, np.float64)
            d = None if draws is None else np.ascontiguousarray(draws, np.float64)
            w = None if weights is None else np.ascontiguousarray(weights, np.float64)
            outs = dict(best_value=dp(bv), best_group=ip(bg), best_cand=ip(bcd), status=ip(st))
            if null:
                outs[null] = None
            tail = (ncand, dp(x), outer, dp(w), 0, ndraw, dp(d), outs["best_value"], outs["best_group"], outs["best_cand"], outs["status"],
                    dp(gv) if groups[0] else None, ip(gc) if groups[1] else None)
            rc = p.L.kiwi_hip_spectral_candidates_bootstrap(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > spectral_candidates_bootstrap: .*" + match):
                p._ck(rc, "spectral_candidates_bootstrap")
            if listed:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_spectral_candidates_bootstrap_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > spectral_candidates_bootstrap: .*" + match):
                    p._ck(rc, "spectral_candidates_bootstrap")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)

        # what this call adds
        entry("ndraw = 0; at least one draw", ndraw=0)
        entry("at least one draw", ndraw=-2)
        entry("null draw_weights", draws=None)
        for name in ("best_value", "best_group", "best_cand", "status"):
            entry("null draw_weights, best_value, best_group, best_cand or status", null=name)
        bad = dw.copy()
        bad[2, 1] = np.nan
        entry("draw_weights of draw 2, receiver 2 is not finite", draws=bad)
        bad[2, 1] = np.inf
        entry("draw_weights of draw 2, receiver 2 is not finite", draws=bad)
        w = np.ones(sc.nrec)
        w[4] = np.inf
        entry("receiver_weight of receiver 5 is not finite", weights=w)
        w[4] = np.nan
        entry("receiver_weight of receiver 5 is not finite", weights=w)
        for groups in ((True, False), (False, True)):
            entry("both or not at all", groups=groups)
        still_usable()
        # what the parent call refuses of the set-up
        for K in (0, 9):
            entry("basis sources per group", K=K)
        entry("at least one candidate", ncand=0)
        x = cand.copy()
        x[3, 2] = np.nan
        entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, listed=False)
        still_usable()
        for method in ("l2norm", "l1norm", "floating_l2norm"):
            p.set_misfit_method(method)
            entry("the misfit method must be ampspec_l2norm or ampspec_l1norm")
        p.set_misfit_method("ampspec_l2norm")
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.spectral_candidates_bootstrap(0, 2, 6, cand, dw, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"spectral_candidates_bootstrap: candidates must be \[ncand, K = 6\]"):
            p.spectral_candidates_bootstrap(0, 2, 6, cand[:, :5], dw)
        with pytest.raises(KiwiHipError, match=r"spectral_candidates_bootstrap: draw_weights must be \[ndraw, 6\]"):
            p.spectral_candidates_bootstrap(0, 2, 6, cand, dw[:, :5])
        still_usable()
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 9: the helper and the example
def test_helper_agrees_with_the_host_route_and_finds_the_planted_mechanism_and_depth():
    """3 depths x the 576 double couples of GRID x 2 moments; the data are the planted double couple at 10 km under noise, a pass
    band on every receiver"""
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted, location=[0., 0., 0., 10000.]))
    sc.make_references(sc.oracle())
    rng = np.random.default_rng(12)
    for key, (lo, d) in list(sc.refs.items()):
        sc.refs[key] = (lo, (d + 0.02 * np.std(d) * rng.standard_normal(len(d))).astype(np.float32))
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        for ir in range(1, sc.nrec + 1):
            p.set_misfit_filter(ir, *band(sc.gf["dt"]))
        p.set_misfit_method("ampspec_l2norm")
        rows = np.stack([mt_row(np.zeros(6), location=[0., 0., 0., depth]) for depth in (8000., 10000., 12000.)])
        moments = [PLANTED_SDR[3], 2 * PLANTED_SDR[3]]
        dw = bc.draw_rows(sc.nrec, 200, range(sc.nrec), [], seed=8)
        res = mtfit.bootstrap_double_couples_spectral(p, "moment_tensor", rows, *GRID, moments, dw, outer_norm="l2norm", per_group=True)
        assert np.all(res["status"] == 0) and p.nsrc == 18
        assert res["row"][0] == 1 and res["moment"][0] == PLANTED_SDR[3]
        assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR)
        assert np.isnan(res["misfit"][1]) and res["row"][1] == -1 and np.isnan(res["strike"][1]) and np.isnan(res["moment"][1])      # the row of zeros
        assert res["index"][1] == -1
        assert res["rows_misfit"].shape == res["rows_strike"].shape == res["rows_moment"].shape == res["rows_index"].shape == (3, 200)
        # the planted depth and mechanism are the mode of the resampled draws
        has = res["row"][3:] >= 0
        assert np.all(has) and np.bincount(res["row"][3:]).argmax() == 1
        mode = int(np.bincount(res["index"][3:]).argmax())
        sdr = mtfit.double_couple_candidates(*GRID)[1][mode // 2]
        assert same_mechanism(sdr[0], sdr[1], sdr[2], PLANTED_SDR), sdr
        # its arrays are the host route's
        mech = mtfit.double_couple_candidates(*GRID, 1.0)[0]
        cand = (mech[:, None, :] * (np.array(moments) / 1e18)[None, :, None]).reshape(-1, 6)
        want, _ = host_route(p, slot_map(sc, [True] * sc.nrec), sc.nrec, 0, 3, 6, cand, dw, "l2norm", None, False)
        bc.assert_boot(res["boot"], want, "helper", same_batch=True)
        with pytest.raises(KiwiHipError, match="is not resampled"):
            mtfit.bootstrap_double_couples_spectral(p, "moment_tensor", rows, [0.], [45.], [90.], None, dw)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_ampspec_bootstrap.py"), "--small"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted mechanism and depth found by the draw of ones" in out.stdout and "planted depth wins" in out.stdout, out.stdout
    assert "polarity" in out.stdout
