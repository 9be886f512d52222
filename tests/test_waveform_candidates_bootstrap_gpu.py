"""kiwi_hip_waveform_candidates_bootstrap on the device.  The yardstick is the host route that defines the call, on the same
context and the same uploaded batch: `waveform_candidates_time_scan(..., slot_misfit=True)`, then `Engine.outer_misfits_slots` on
its float arrays read as ngroup x nk x ncand sources of nmis slots -- once for all groups (best_*), once per group (group_*).  Bit
for bit, whatever the number of candidates against the kernel's tile, of draws against its draw tile, of receivers against its LDS
layout, and however the call is cut into chunks, draw passes, pieces and devices; also against the numpy restatement fed with the
parent's slot arrays; a failed basis source; refusals; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_bootstrap_cases as bc
from tests import linfit_timescan_cases as lc
from tests import waveform_candidates_bootstrap_restatement as wbr
from tests.common import Scenario
from tests.linfit_cases import PLANTED, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups
from tests.test_waveform_candidates_gpu import GRID, band, same_mechanism, slot_map, zero_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts
ENABLED = [True] * 5 + [False]


def offsets_of(nk):
    """(k0, kstep, nk): the plain case for one offset, else offsets on both sides of zero"""
    return (0, 1, 1) if nk == 1 else (-2, 2, nk)


def standard(method="l1norm", **more):
    """tests/test_linfit_gpu.py's six receivers of 1 to 5 components under a window of 60 samples, as the time scan's GPU test has
    them: receiver 6 disabled, receiver 4 with references of zeros; WEIGHTS gives receiver 2 the weight 0"""
    sc, p = build(COMPS, window=60, **more)
    p.switch_receiver(6, False)
    zero_reference(p, sc, 4)
    p.set_misfit_method(method)
    return sc, p


def host_route(p, rec, nrec, isrc0, ngroup, K, cand, dw, k0, kstep, nk, outer_norm, w, anarchy):
    """what the library offered before: the scan's slot arrays downloaded, then kiwi_hip_outer_misfits on them"""
    scan = p.waveform_candidates_time_scan(isrc0, ngroup, K, k0, kstep, nk, cand, outer_norm=outer_norm, receiver_weights=w, anarchy=anarchy,
                                           cand_misfit=False, cand_offset=False, slot_misfit=True)

    def outer(mis, nor, slots, nrec_, norm, w_, an, draws):
        return p.outer_misfits_slots(mis, nor, slots, nrec_, outer_norm=norm, receiver_weights=w_, anarchy=an, draw_weights=draws)
    return wbr.from_scan(scan.slot_misfit, scan.slot_norm, rec, nrec, scan.status, dw, outer_norm, w, anarchy, outer=outer), scan


# ------------------------------------------------------------------------------------------------ 1: device == host route
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_device_equals_host_route_bit_for_bit(K, ngroup):
    sc, p = standard()
    try:
        C, T, Rmax = p.waveform_candidates_bootstrap_shape(K)
        assert C >= 64 and Rmax >= 64
        rec = slot_map(sc, ENABLED)
        assert sorted(set(np.bincount(rec))) == [1, 2, 3, 4, 5]      # receivers of 1 to 5 slots: the slot fold
        rng = np.random.default_rng(40 * K + ngroup)
        rows = scattered_groups(rng, ngroup, K)
        if ngroup == 3:
            rows[2 * K:] = rows[:K]                           # two groups with identical rows: a tie across groups
        p.set_source_params("moment_tensor", rows)
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C - 1] = cand[2]                                 # a tie across a tile boundary... (C - 1 is the last lane of tile 0)
        cand[C] = cand[2]                                     # ... and with the first lane of tile 1
        dw = bc.draw_rows(sc.nrec, 2 * T + 1, [0, 2, 4], [3, 5], seed=K)
        ncalls = 0
        for method, factor in (("l1norm", 1.0), ("l2norm", 1.0), ("l1norm", 0.75)):
            p.set_synthetics_factor(factor)
            p.set_misfit_method(method)
            whole = method == "l1norm" and factor == 1.0      # every cut of the work once; the other insides at the largest shape
            for nk in (1, 3) if whole else (3,):
                for ncand in (1, C - 1, C + 1, 2 * C + 3) if whole else (2 * C + 3,):
                    for norm in ("l1norm", "l2norm"):
                        for anarchy in (False, True):
                            for w in (WEIGHTS, None):
                                kw = dict(outer_norm=norm, receiver_weights=w, anarchy=anarchy)
                                want, _ = host_route(p, rec, sc.nrec, 0, ngroup, K, cand[:ncand], dw, *offsets_of(nk), norm, w, anarchy)
                                for ndraw in ((1, T - 1, T, T + 1, 2 * T + 1) if w is not None and whole else (2 * T + 1,)):
                                    got = p.waveform_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw[:ndraw], *offsets_of(nk), per_group=True, **kw)
                                    what = "K=%d ngroup=%d %s x %g nk=%d ncand=%d %s anarchy=%s weights=%s ndraw=%d" % (
                                        K, ngroup, method, factor, nk, ncand, norm, anarchy, w is not None, ndraw)
                                    bc.assert_boot(got, want, what, ndraw, same_batch=True)
                                    ncalls += 1
                                    assert np.all(got.status == 0), what
                                    assert not np.isnan(got.best_value[0]) and got.best_cand[0] >= 0, what        # the row of ones
                                    if ndraw >= 3:            # all zeros; non-zero only on skipped receivers
                                        assert np.all(np.isnan(got.best_value[1:3])) and np.all(got.best_group[1:3] == -1), what
                                        assert np.all(got.best_offset[1:3] == -1) and np.all(got.best_cand[1:3] == -1), what
                                        assert np.all(np.isnan(got.group_value[:, 1:3])) and np.all(got.group_cand[:, 1:3] == -1), what
                                    assert np.all(got.best_cand != C - 1) and np.all(got.best_cand != C), what      # the lowest index of a tie
                                    assert np.all(got.best_group != 2), what                                        # the lower group of a tie
                                    if ngroup == 3:
                                        assert np.array_equal(got.group_value[0], got.group_value[2], equal_nan=True), what
                                got = p.waveform_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw, *offsets_of(nk), **kw)
                                assert got.group_value is None and got.group_offset is None and got.group_cand is None
                                bc.assert_boot(got, want, "no group arrays", same_batch=True)
        ms = p.waveform_candidates_bootstrap_ms()
        assert len(ms) == 5 and all(t > 0 for t in ms[:4]) and ms[4] >= 0
        print("K=%d ngroup=%d: %d device calls against the host route" % (K, ngroup, ncalls))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: device == restatement
def test_device_equals_restatement_fed_with_the_parents_slot_arrays():
    K, ngroup, nk = 6, 2, 3
    sc, p = standard()
    try:
        C, T, _ = p.waveform_candidates_bootstrap_shape(K)
        rec = slot_map(sc, ENABLED)
        rng = np.random.default_rng(77)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = bc.draw_rows(sc.nrec, 2 * T + 1, [0, 2, 4], [3, 5], seed=9)
        for method in ("l1norm", "l2norm"):
            p.set_misfit_method(method)
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    scan = p.waveform_candidates_time_scan(0, ngroup, K, *offsets_of(nk), cand, outer_norm=norm, receiver_weights=WEIGHTS,
                                                           anarchy=anarchy, slot_misfit=True)
                    rs = wbr.from_scan(scan.slot_misfit, scan.slot_norm, rec, sc.nrec, scan.status, dw, norm, WEIGHTS, anarchy)
                    got = p.waveform_candidates_bootstrap(0, ngroup, K, cand, dw, *offsets_of(nk), outer_norm=norm, receiver_weights=WEIGHTS,
                                                          anarchy=anarchy, per_group=True)
                    bc.assert_boot(got, rs, "restatement %s inside, %s anarchy=%s" % (method, norm, anarchy), same_batch=True)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: the LDS layout
_WIDE = {}


def wide_scenario(nrec):
    if nrec not in _WIDE:
        sc = Scenario(nrec=nrec, comps_list=["d"] * nrec, true_type=6, true_params=mt_row(PLANTED))
        sc.make_references(sc.oracle())
        _WIDE[nrec] = sc
    return _WIDE[nrec]


def _max_receivers():
    from kiwi_amd import lib as klib
    import ctypes
    c, t, r = (ctypes.c_int() for _ in range(3))
    assert klib.load().kiwi_hip_waveform_candidates_bootstrap_shape(6, ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)) == 0
    return r.value


def test_the_most_receivers_the_lds_layout_holds():
    """max_receivers receivers of one component: two groups, 70 candidates, 2 T + 1 draws, one of them decided by the last receiver
    alone; bits as in case 1"""
    nrec = _max_receivers()
    sc = wide_scenario(nrec)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        C, T, Rmax = p.waveform_candidates_bootstrap_shape(6)
        assert nrec == Rmax <= 511
        p.set_misfit_method("l1norm")
        p.switch_receiver(3, False)
        enabled = [r != 2 for r in range(nrec)]
        rec = slot_map(sc, enabled)
        rng = np.random.default_rng(nrec)
        p.set_source_params("moment_tensor", scattered_groups(rng, 2, 6))
        w = rng.uniform(0.5, 2.0, nrec)
        w[nrec - 2] = 0.0
        cand = rng.uniform(-2.0, 2.0, (70, 6))
        counted = [r for r in range(nrec) if r not in (2, nrec - 2)]
        dw = bc.draw_rows(nrec, 2 * T + 1, counted, [2, nrec - 2], seed=1)
        dw[3] = 0.0
        dw[3, nrec - 1] = 1.0                                 # the last receiver alone decides
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                want, scan = host_route(p, rec, nrec, 0, 2, 6, cand, dw, -2, 3, 2, norm, w, anarchy)
                got = p.waveform_candidates_bootstrap(0, 2, 6, cand, dw, -2, 3, 2, outer_norm=norm, receiver_weights=w, anarchy=anarchy, per_group=True)
                bc.assert_boot(got, want, "%d receivers %s anarchy=%s" % (nrec, norm, anarchy), same_batch=True)
                assert not np.any(np.isnan(got.best_value[3:])) and np.all(np.isnan(got.best_value[1:3]))
                # draw 3 by hand: the last receiver's single slot against its norm, the weight cancelling
                last = scan.slot_misfit[..., -1].astype(np.float64) / scan.slot_norm[:, None, None, -1].astype(np.float64)
                assert np.isclose(got.best_value[3], np.min(last), rtol=1e-12)
    finally:
        p.close()


def test_one_receiver_more_than_the_layout_holds_is_refused():
    Rmax = _max_receivers()
    sc = wide_scenario(Rmax + 1)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        assert p.outer_max_receivers() > Rmax                 # (the yardstick's own limit is not the one met)
        p.set_misfit_method("l1norm")
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(1), 1, 6))
        cand = np.random.default_rng(2).uniform(-1.0, 1.0, (3, 6))
        with pytest.raises(KiwiHipError, match=r"nok > waveform_candidates_bootstrap: %d receivers.*at most %d" % (Rmax + 1, Rmax)):
            p.waveform_candidates_bootstrap(0, 1, 6, cand, np.ones((2, Rmax + 1)))
        p.eval()
        assert np.all(p.get_misfits()[0] > 0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: however it is cut
def test_first_source_pieces_chunks_draw_passes_and_contexts(monkeypatch):
    ngroup, K = lc.CHUNK_GROUPS, lc.CHUNK_K
    rows = lc.chunk_rows()
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = bc.pack_candidates()
    as_dict = lambda s: {name: getattr(s, name) for name in s._fields}      # noqa: E731
    exact = common.arith() == "exact"
    base, passes = {}, {}

    def prepared(**more):
        sc, q = lc.standard(**more)
        q.set_misfit_method("l1norm")
        return sc, q

    sc, p = prepared()
    try:
        C, T, _ = p.waveform_candidates_bootstrap_shape(K)
        rec = slot_map(sc, ENABLED)
        dw = bc.pack_draws(sc.nrec)
        pdw = bc.draw_rows(sc.nrec, bc.PASS_NDRAW, range(5), [5], seed=4)
        pc = bc.pass_candidates(C)
        assert bc.PASS_SCAN[2] * ((len(pc) + C - 1) // C) * 12 * bc.PASS_NDRAW > 1 << 20       # one group's slab against 1 MiB
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            p.set_source_params("moment_tensor", rows)
            b = base[norm] = p.waveform_candidates_bootstrap(0, ngroup, K, cand, dw, *lc.CHUNK_SCAN, **kw)
            bc.assert_boot(b, host_route(p, rec, sc.nrec, 0, ngroup, K, cand, dw, *lc.CHUNK_SCAN, norm, None, True)[0], "base " + norm, same_batch=True)
            print(norm, "winners of the draws (group, offset, candidate):", sorted(set(zip(b.best_group[3:], b.best_offset[3:], b.best_cand[3:]))))
            p.set_source_params("moment_tensor", np.concatenate([head, rows]))
            got = p.waveform_candidates_bootstrap(5, ngroup, K, cand, dw, *lc.CHUNK_SCAN, **kw)
            if exact:
                bc.assert_boot(got, as_dict(b), "isrc0 = 5")
            for piece in (K, 2 * K, 0):
                got = p.waveform_candidates_bootstrap_params("moment_tensor", rows, K, cand, dw, *lc.CHUNK_SCAN, piece=piece, **kw)
                assert np.array_equal(got.status, b.status)
                if exact:
                    bc.assert_boot(got, as_dict(b), "piece %d" % piece)
                assert p.nsrc == (piece or p.nsrc)
                p.eval()                                      # the engine holds the head of the list and knows how long it is
            # the case whose draws go in passes below, here in one pass, against the host route
            p.set_source_params("moment_tensor", bc.pass_rows())
            passes[norm] = p.waveform_candidates_bootstrap(0, bc.PASS_GROUPS, 6, pc, pdw, *bc.PASS_SCAN, **kw)
            bc.assert_boot(passes[norm], host_route(p, rec, sc.nrec, 0, bc.PASS_GROUPS, 6, pc, pdw, *bc.PASS_SCAN, norm, None, True)[0],
                           "one pass " + norm, same_batch=True)
    finally:
        p.close()
    # several chunks, several draw passes: KIWI_HIP_CHUNK_MB is read when a context is made
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")
    sc, q = prepared()
    try:
        for norm, b in base.items():
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            q.set_source_params("moment_tensor", rows)
            q.kernel_ms()
            got = q.waveform_candidates_bootstrap(0, ngroup, K, cand, dw, *lc.CHUNK_SCAN, **kw)
            assert q.kernel_ms()[1][1] >= 2                   # a chunk boundary between groups
            assert np.array_equal(got.status, b.status)
            if exact:
                bc.assert_boot(got, as_dict(b), "chunks " + norm)
            q.set_source_params("moment_tensor", bc.pass_rows())
            got = q.waveform_candidates_bootstrap(0, bc.PASS_GROUPS, 6, pc, pdw, *bc.PASS_SCAN, **kw)
            if exact:
                bc.assert_boot(got, as_dict(passes[norm]), "draw passes " + norm)
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = prepared(engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        for norm, b in base.items():
            for piece in (0, 2 * K):
                got = m2.waveform_candidates_bootstrap_params("moment_tensor", rows, K, cand, dw, *lc.CHUNK_SCAN, piece=piece, outer_norm=norm,
                                                              anarchy=True, per_group=True)
                assert np.array_equal(got.status, b.status)
                if exact:
                    bc.assert_boot(got, as_dict(b), "two contexts, piece %d" % piece)
    finally:
        m2.close()


# ------------------------------------------------------------------------------------------------ 5: a failed basis source
def test_a_group_with_a_failed_basis_source_never_wins():
    sc, p = build(COMPS)
    try:
        p.set_misfit_method("l1norm")
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (6, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((6, 6)) * 1e18
        dw = bc.draw_rows(sc.nrec, 12, range(6), [], seed=6)
        good = eik.copy()
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, per_group=True)
            whole = p.waveform_candidates_bootstrap_params("mt_eikonal", good, 2, cand, dw, -1, 1, 3, **kw)
            assert np.all(whole.status == 0)
            for piece, bad in ((0, [3]), (2, [2, 3])):        # piece 2 with both sources bad: a piece of which nothing is uploaded
                eik = good.copy()
                eik[bad, 3] = 500.0                           # "Empty rupture area": above the constraining planes
                got = p.waveform_candidates_bootstrap_params("mt_eikonal", eik, 2, cand, dw, -1, 1, 3, piece=piece, **kw)
                what = "%s piece %d" % (norm, piece)
                assert list(got.status) == [0, 2, 0], what
                assert np.all(np.isnan(got.group_value[1])) and np.all(got.group_offset[1] == -1) and np.all(got.group_cand[1] == -1), what
                assert np.all(got.best_group != 1), what
                for g in (0, 2):                              # the other groups' bits are unchanged
                    assert np.array_equal(np.isnan(got.group_value[g]), np.isnan(whole.group_value[g])), what
                    if common.arith() == "exact":
                        assert np.array_equal(got.group_value[g], whole.group_value[g], equal_nan=True), what
                        assert np.array_equal(got.group_offset[g], whole.group_offset[g]) and np.array_equal(got.group_cand[g], whole.group_cand[g]), what
                # the call's best is the best of the two groups that are left
                two = np.where(got.group_value[2] < got.group_value[0], 2, 0)
                has = ~np.isnan(got.best_value)
                assert np.array_equal(got.best_group[has], two[has]), what
                assert np.array_equal(got.best_value, np.fmin(got.group_value[0], got.group_value[2]), equal_nan=True), what
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = lc.standard()
    try:
        p.set_misfit_method("l1norm")
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        dw = bc.draw_rows(sc.nrec, 4, range(5), [5])
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        boot_before = p.waveform_candidates_bootstrap(0, 2, 6, cand, dw, 0, 1, 2, per_group=True)
        scan_left = None

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)
            again = p.waveform_candidates_bootstrap(0, 2, 6, cand, dw, 0, 1, 2, per_group=True)
            for name in again._fields:
                assert np.array_equal(getattr(again, name), getattr(boot_before, name), equal_nan=True), name
            return p.get_misfits()

        # afterwards the context is what the time scan leaves
        mine = still_usable()
        p.waveform_candidates_time_scan(0, 2, 6, 0, 1, 2, cand)
        scan_left = p.get_misfits()
        for x, y in zip(mine, scan_left):
            assert np.array_equal(x, y)
        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)               # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=1, scan=(0, 1, 2), isrc0=0, ngroup=2, listed=True, ndraw=4, draws=dw, weights=None,
                  groups=(True, True, True), null=None):
            """both C entries with these arguments: refused, with the call's name in front and the reason in the message"""
            bv, bg, bo, bcd, st = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(8, np.int32)
            gv, gj, gc = np.zeros(512), np.zeros(512, np.int32), np.zeros(512, np.int32)
            x = np.ascontiguousarray(x, np.float64)
            d = None if draws is None else np.ascontiguousarray(draws, np.float64)
            w = None if weights is None else np.ascontiguousarray(weights, np.float64)
            outs = dict(best_value=dp(bv), best_group=ip(bg), best_offset=ip(bo), best_cand=ip(bcd), status=ip(st))
            if null:
                outs[null] = None
            tail = (scan[0], scan[1], scan[2], ncand, dp(x), outer, dp(w), 0, ndraw, dp(d), outs["best_value"], outs["best_group"],
                    outs["best_offset"], outs["best_cand"], outs["status"], dp(gv) if groups[0] else None, ip(gj) if groups[1] else None,
                    ip(gc) if groups[2] else None)
            rc = p.L.kiwi_hip_waveform_candidates_bootstrap(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > waveform_candidates_bootstrap: .*" + match):
                p._ck(rc, "waveform_candidates_bootstrap")
            if listed:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_waveform_candidates_bootstrap_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > waveform_candidates_bootstrap: .*" + match):
                    p._ck(rc, "waveform_candidates_bootstrap")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)

        # what this call adds
        entry("ndraw = 0; at least one draw", ndraw=0)
        entry("at least one draw", ndraw=-2)
        entry("null draw_weights", draws=None)
        for name in ("best_value", "best_group", "best_offset", "best_cand", "status"):
            entry("null draw_weights, best_value, best_group, best_offset, best_cand or status", null=name)
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
        for groups in ((True, True, False), (True, False, True), (False, True, True), (True, False, False)):
            entry("all three or not at all", groups=groups)
        still_usable()
        # what the time scan refuses of K, the candidates and the offsets
        for K in (0, 9):
            entry("basis sources per group", K=K)
        entry("at least one candidate", ncand=0)
        x = cand.copy()
        x[3, 2] = np.nan
        entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        entry("need at least one offset", scan=(0, 1, 0))
        entry("at most %d are supported" % p.L.kiwi_hip_time_scan_max_offsets(), scan=(0, 1, p.L.kiwi_hip_time_scan_max_offsets() + 1))
        entry("at least one sample", scan=(0, 0, 3))
        entry("the largest shift is", scan=(-p.L.kiwi_hip_time_scan_max_shift() - 1, 1, 2))
        for isrc0, ngroup in ((0, 3), (7, 1), (-1, 1)):
            entry("not inside the uploaded batch", isrc0=isrc0, ngroup=ngroup, listed=False)
        still_usable()
        p.set_misfit_filter(2, *band(sc.gf["dt"]))
        entry("has a misfit filter")
        p.set_misfit_filter(2, [], [])
        still_usable()
        for method in ("ampspec_l1norm", "floating_l1norm", "peak"):
            p.set_misfit_method(method)
            entry("the misfit method must be l1norm or l2norm")
        p.set_misfit_method("l1norm")
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.waveform_candidates_bootstrap(0, 2, 6, cand, dw, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"waveform_candidates_bootstrap: candidates must be \[ncand, K = 6\]"):
            p.waveform_candidates_bootstrap(0, 2, 6, cand[:, :5], dw)
        with pytest.raises(KiwiHipError, match=r"waveform_candidates_bootstrap: draw_weights must be \[ndraw, 6\]"):
            p.waveform_candidates_bootstrap(0, 2, 6, cand, dw[:, :5])
        still_usable()
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7: the helper and the example
PLANTED_SDR = (60.0, 60.0, 90.0, 5e18)


def test_helper_agrees_with_the_host_route_and_finds_the_planted_node_under_a_glitch():
    """3 depths x 5 offsets x the 576 double couples of GRID x 2 moments; the data are the planted double couple at 10 km, three
    samples later than the rows, under noise, station 3 a glitch (the time scan's helper test)"""
    planted = np.array(synthetic.mt_from_sdr(*PLANTED_SDR), np.float32)
    sc = Scenario(comps_list=list(COMPS), true_type=6, true_params=mt_row(planted, location=[1.5, 0., 0., 10000.]))
    sc.make_references(sc.oracle())
    assert sc.gf["dt"] == 0.5
    rng = np.random.default_rng(12)
    for key, (lo, d) in list(sc.refs.items()):
        sc.refs[key] = (lo, (d + 0.02 * np.std(d) * rng.standard_normal(len(d))).astype(np.float32))
    for k in range(len(sc.comps[2])):
        lo, d = sc.refs[(3, k + 1)]
        sc.refs[(3, k + 1)] = (lo, (20.0 * np.max(np.abs(d)) * (np.arange(len(d)) > len(d) // 3)).astype(np.float32))
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_misfit_method("l1norm")
        rows = np.stack([mt_row(np.zeros(6), location=[0., 0., 0., depth]) for depth in (8000., 10000., 12000.)])
        moments = [PLANTED_SDR[3], 2 * PLANTED_SDR[3]]
        dw = bc.draw_rows(sc.nrec, 24, range(sc.nrec), [], seed=8)
        res = mtfit.bootstrap_double_couples_waveform(p, "moment_tensor", rows, *GRID, moments, dw, k0=1, kstep=1, nk=5, outer_norm="l1norm",
                                                      per_group=True)
        assert np.all(res["status"] == 0) and p.nsrc == 18
        assert res["row"][0] == 1 and res["offset"][0] == 2 and res["time_shift"][0] == 1.5 and res["moment"][0] == PLANTED_SDR[3]
        assert same_mechanism(res["strike"][0], res["dip"][0], res["rake"][0], PLANTED_SDR)
        assert np.isnan(res["misfit"][1]) and res["row"][1] == -1 and np.isnan(res["strike"][1]) and np.isnan(res["moment"][1])      # the row of zeros
        assert np.isnan(res["time_shift"][1]) and res["offset"][1] == -1 and res["index"][1] == -1
        assert res["rows_misfit"].shape == res["rows_strike"].shape == res["rows_offset"].shape == res["rows_moment"].shape == (3, 24)
        # its arrays are the host route's
        mech = mtfit.double_couple_candidates(*GRID, 1.0)[0]
        cand = (mech[:, None, :] * (np.array(moments) / 1e18)[None, :, None]).reshape(-1, 6)
        rec = slot_map(sc, [True] * sc.nrec)
        want, _ = host_route(p, rec, sc.nrec, 0, 3, 6, cand, dw, 1, 1, 5, "l1norm", None, False)
        bc.assert_boot(res["boot"], want, "helper", same_batch=True)
        with pytest.raises(KiwiHipError, match="no closed form under"):
            mtfit.bootstrap_double_couples_waveform(p, "moment_tensor", rows, [0.], [45.], [90.], None, dw)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith())
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_l1_bootstrap.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted mechanism, depth and origin time found by the draw of ones" in out.stdout and "planted depth wins" in out.stdout, out.stdout
