"""kiwi_hip_linear_fit_candidates_floating_bootstrap on the device.  The yardstick is the host route that defines the call, on the
same context: `linear_fit_candidates_floating(..., cand_shift=True, receiver_misfit=True)`, then `Engine.outer_misfits` on its
float arrays read as ngroup x ncand sources of one slot per receiver -- once for all groups (best_*), once per group (group_*) --
and the winner's row of cand_shift (tests/linfit_candidates_floating_bootstrap_cases.py host_route).  Bit for bit under the `exact`
arithmetic contract, whatever the number of candidates against the kernel's tile, of draws against its draw tile, of shifts
against the LDS stage, and however the call is cut into chunks, draw passes, pieces and contexts; also against the numpy restatement fed with the
parent's sums; ranges of one shift against the Gram sibling; a failed basis source; refusals; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit, synthetic
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_floating_bootstrap_cases as fc
from tests import linfit_candidates_floating_bootstrap_restatement as fbr
from tests import linfit_candidates_floating_restatement as fr
from tests.linfit_candidates_floating_cases import RANGES_A, RANGES_B, brute_sums, slack_of
from tests.linfit_cases import eikonal_list_with_a_failed_piece, mt_row
from tests.test_linfit_gpu import COMPS, build, colocated_groups, multi_engine, scattered_groups

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = fc.WEIGHTS


# ------------------------------------------------------------------------------------------------ 1: device == host route
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_device_equals_host_route_bit_for_bit(K, ngroup):
    """RANGES_A: the receivers that count have ranges of one shift (0, 0), of J shifts on one side only (1, 4) and of 33 shifts, one
    more than an LDS stage; without weights the receiver of range (-2, -1) counts too.  Receiver 4 has references of zeros,
    receiver 6 is disabled, WEIGHTS gives receiver 2 the weight 0"""
    sc, p = fc.standard_with_skipped_receivers()
    try:
        C, T, Rmax = p.linear_fit_candidates_floating_bootstrap_shape(K)
        S = p.linear_fit_candidates_floating_shape(K)[2]
        assert C == 256 and Rmax >= sc.nrec and max(hi - lo + 1 for lo, hi in RANGES_A) == S + 1
        rng = np.random.default_rng(50 * K + ngroup)
        rows = scattered_groups(rng, ngroup, K)
        if ngroup == 3:
            rows[2 * K:] = rows[:K]                           # two groups with identical rows: a tie across groups
        p.set_source_params("moment_tensor", rows)
        cand = rng.uniform(-2.0, 2.0, (2 * C + 3, K))
        cand[C - 1] = cand[2]                                 # a tie across a tile boundary... (C - 1 is the last lane of tile 0)
        cand[C] = cand[2]                                     # ... and with the first lane of tile 1
        dw = fc.draw_rows(sc.nrec, 2 * T + 1, fc.COUNTED, fc.SKIPPED, seed=K)
        fc.floating(p, sc, RANGES_A)
        ncalls = 0
        for ncand in (1, C - 1, C + 1, 2 * C + 3):
            for norm in ("l1norm", "l2norm"):
                for anarchy in (False, True):
                    for w in (WEIGHTS, None):
                        kw = dict(outer_norm=norm, receiver_weights=w, anarchy=anarchy)
                        what = "K=%d ngroup=%d ncand=%d %s anarchy=%s weights=%s" % (K, ngroup, ncand, norm, anarchy, w is not None)
                        want = fc.host_route(p, 0, ngroup, K, cand[:ncand], dw, norm, w, anarchy)
                        # on the host route first: the row of ones has a finite winner, the rows of zeros and of skipped
                        # receivers only, and no others, are excluded -- NaN == NaN hides nothing below
                        excluded = np.isnan(want["best_value"])
                        assert np.array_equal(np.nonzero(excluded)[0], [1, 2]), what
                        assert np.all(np.isnan(want["group_value"]) == excluded[None, :]), what
                        assert np.all(want["best_cand"][~excluded] >= 0) and np.all(want["status"] == 0), what
                        counted = fc.COUNTED if w is not None else [0, 1, 2, 4]
                        assert np.any(want["best_shift"][:, counted[1:]] != 0), what
                        for ndraw in ((1, T - 1, T, T + 1, 2 * T + 1) if w is not None else (2 * T + 1,)):
                            got = p.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand[:ncand], dw[:ndraw], per_group=True, **kw)
                            fc.assert_boot(got, want, "%s ndraw=%d" % (what, ndraw), ndraw, same_batch=True)
                            ncalls += 1
                            assert got.best_shift.shape == (ndraw, sc.nrec) and got.group_shift.shape == (ngroup, ndraw, sc.nrec), what
                            skipped = [r for r in range(sc.nrec) if r not in counted]
                            assert not np.any(got.best_shift[:, skipped]) and not np.any(got.group_shift[:, :, skipped]), what
                            if ndraw >= 3:                    # all zeros; non-zero only on skipped receivers
                                assert np.all(np.isnan(got.best_value[1:3])) and np.all(got.best_group[1:3] == -1), what
                                assert np.all(got.best_cand[1:3] == -1) and not np.any(got.best_shift[1:3]), what
                                assert np.all(got.group_cand[:, 1:3] == -1) and not np.any(got.group_shift[:, 1:3]), what
                            if common.arith() == "exact":
                                assert np.all(got.best_cand != C - 1) and np.all(got.best_cand != C), what      # the lowest index of a tie
                                assert np.all(got.best_group != 2), what                                        # the lower group of a tie
                                if ngroup == 3:
                                    assert np.array_equal(got.group_value[0], got.group_value[2], equal_nan=True), what
                                    assert np.array_equal(got.group_shift[0], got.group_shift[2]), what
                        got = p.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand[:ncand], dw, **kw)
                        assert got.group_value is None and got.group_cand is None and got.group_shift is None
                        fc.assert_boot(got, want, what + ", no group arrays", same_batch=True)
        ms = p.linear_fit_candidates_floating_bootstrap_ms()
        assert len(ms) == 4 and all(t > 0 for t in ms[:3]) and ms[3] >= 0
        print("K=%d ngroup=%d: %d device calls against the host route" % (K, ngroup, ncalls))
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: device == restatement
def test_device_equals_restatement_fed_with_the_parents_sums():
    """the sums of every shift by the brute route of tests/linfit_candidates_floating_cases.py (the references moved,
    `linear_fit(..., by_receiver=True)` each time), the composition of the two restatements on them.  The slack (fused contract
    only) is the parent test's, tests/linfit_candidates_floating_cases.py slack_of"""
    K, ngroup = 6, 2
    sc, p = fc.standard_with_skipped_receivers()
    try:
        dt = sc.gf["dt"]
        C, T, _ = p.linear_fit_candidates_floating_bootstrap_shape(K)
        rng = np.random.default_rng(78)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = fc.draw_rows(sc.nrec, 2 * T + 1, fc.COUNTED, fc.SKIPPED, seed=9)
        wz = np.where([True] * 5 + [False], WEIGHTS, 0.0)
        for anarchy, ranges in ((False, RANGES_A), (True, RANGES_B)):
            nbr, sb, sR = brute_sums(p, dt, ranges, ngroup, K)
            fc.floating(p, sc, ranges)
            for norm in ("l1norm", "l2norm"):
                scan = fr.evaluate(nbr, sb, sR, [lo for lo, _ in ranges], wz, anarchy, cand, norm)
                rs = fbr.from_scan(scan["receiver_misfit"], scan["receiver_norm"], scan["cand_shift"], scan["status"], dw, norm, wz, anarchy)
                slack = float(np.max(slack_of(nbr, scan, cand)))
                got = p.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand, dw, outer_norm=norm, receiver_weights=WEIGHTS,
                                                                 anarchy=anarchy, per_group=True)
                assert np.array_equal(np.nonzero(np.isnan(rs["best_value"]))[0], [1, 2])
                fc.assert_boot(got, rs, "restatement %s anarchy=%s" % (norm, anarchy), slack=slack)
            p.set_floating_shiftrange(0, 0.0, 0.0)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 3: every range (0, 0)
@pytest.mark.parametrize("anarchy", [False, True])
def test_ranges_of_one_shift_equal_the_gram_siblings_bootstrap(anarchy):
    """every range (0, 0), outer l1norm: kiwi_hip_linear_fit_candidates_bootstrap with nk = 1 at offset 0 on the same context under
    l2norm, bit for bit (n_r = sqrt(R_r) / 1, and the parent pair's receiver misfits are the same bits), and every shift 0"""
    K, ngroup = 6, 3
    sc, p = fc.standard_with_skipped_receivers()
    try:
        C, T, _ = p.linear_fit_candidates_floating_bootstrap_shape(K)
        rng = np.random.default_rng(6)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = fc.draw_rows(sc.nrec, T + 1, fc.COUNTED, fc.SKIPPED, seed=2)
        kw = dict(outer_norm="l1norm", receiver_weights=WEIGHTS, anarchy=anarchy, per_group=True)
        gram = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand, dw, 0, 1, 1, **kw)
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(0, 0.0, 0.0)
        got = p.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand, dw, **kw)
        assert np.array_equal(np.nonzero(np.isnan(gram.best_value))[0], [1, 2]) and np.all(gram.status == 0)
        for name in ("best_value", "best_group", "best_cand", "status", "group_value", "group_cand"):
            assert np.array_equal(getattr(got, name), getattr(gram, name), equal_nan=name.endswith("value")), name
        assert not np.any(got.best_shift) and not np.any(got.group_shift)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 4: however it is cut
PASS_GROUPS, PASS_NDRAW = 2, 10000                            # 9 tiles x 10000 draws x 12 bytes: one group's slab above 1 MiB


def test_first_source_pieces_chunks_draw_passes_and_contexts(monkeypatch):
    ngroup, K = 40, 6
    rows = colocated_groups(np.random.default_rng(8), ngroup)
    head = scattered_groups(np.random.default_rng(9), 1, 5)
    cand = np.random.default_rng(10).uniform(-2.0, 2.0, (300, K))
    as_dict = lambda s: {name: getattr(s, name) for name in s._fields}      # noqa: E731
    base, passes, pass_slack = {}, {}, {}
    sc, p = build(COMPS)
    try:
        dw = fc.draw_rows(sc.nrec, 40, range(sc.nrec), [], seed=3)
        p.set_source_params("moment_tensor", rows)
        nbr, sb, sR = brute_sums(p, sc.gf["dt"], RANGES_A, ngroup, K)
        fc.floating(p, sc, RANGES_A)
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            p.set_source_params("moment_tensor", rows)
            b = base[norm] = p.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand, dw, **kw)
            fc.assert_boot(b, fc.host_route(p, 0, ngroup, K, cand, dw, norm, None, True), "base " + norm, same_batch=True)
            print(norm, "winners of the draws (group, candidate):", sorted(set(zip(b.best_group[3:], b.best_cand[3:]))))
            scan = fr.evaluate(nbr, sb, sR, [lo for lo, _ in RANGES_A], None, True, cand, norm)
            slack = float(np.max(slack_of(nbr, scan, cand)))
            p.set_source_params("moment_tensor", np.concatenate([head, rows]))
            fc.assert_boot(p.linear_fit_candidates_floating_bootstrap(5, ngroup, K, cand, dw, **kw), as_dict(b), "isrc0 = 5", slack=slack)
            for piece in (K, 3 * K, 0):                       # pieces of one group, of three groups, the default
                got = p.linear_fit_candidates_floating_bootstrap_params("moment_tensor", rows, K, cand, dw, piece=piece, **kw)
                fc.assert_boot(got, as_dict(b), "%s piece %d" % (norm, piece), slack=slack)
                assert p.nsrc == (piece or p.nsrc)
                p.eval()                                      # the engine holds the head of the list and knows how long it is
            # the case whose draws go in passes under the bound below, here in one pass, against the host route
            C = p.linear_fit_candidates_floating_bootstrap_shape(K)[0]
            pc = np.random.default_rng(12).uniform(-2.0, 2.0, (9 * C - 5, K))
            pdw = fc.draw_rows(sc.nrec, PASS_NDRAW, range(sc.nrec), [], seed=4)
            assert ((len(pc) + C - 1) // C) * 12 * PASS_NDRAW > 1 << 20
            p.set_source_params("moment_tensor", rows[:PASS_GROUPS * K])
            passes[norm] = p.linear_fit_candidates_floating_bootstrap(0, PASS_GROUPS, K, pc, pdw, **kw)
            fc.assert_boot(passes[norm], fc.host_route(p, 0, PASS_GROUPS, K, pc, pdw, norm, None, True), "one pass " + norm, same_batch=True)
            two = slice(0, PASS_GROUPS)
            scan = fr.evaluate(nbr[two], [x[two] for x in sb], [x[two] for x in sR], [lo for lo, _ in RANGES_A], None, True, pc, norm)
            pass_slack[norm] = float(np.max(slack_of(nbr[two], scan, pc)))
    finally:
        p.close()
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")              # several chunks of groups: read at kiwi_hip_init
    sc, q = build(COMPS)
    try:
        fc.floating(q, sc, RANGES_A)
        q.set_source_params("moment_tensor", rows)
        for norm, b in base.items():
            q.kernel_ms()
            got = q.linear_fit_candidates_floating_bootstrap(0, ngroup, K, cand, dw, outer_norm=norm, anarchy=True, per_group=True)
            assert q.kernel_ms()[1][1] >= 2                   # a chunk boundary between groups
            fc.assert_boot(got, as_dict(b), "chunks " + norm, slack=slack)
        q.set_source_params("moment_tensor", rows[:PASS_GROUPS * K])
        for norm, b in passes.items():                        # one group's slab of all draws exceeds the bound: two passes of draws
            got = q.linear_fit_candidates_floating_bootstrap(0, PASS_GROUPS, K, pc, pdw, outer_norm=norm, anarchy=True, per_group=True)
            fc.assert_boot(got, as_dict(b), "draw passes " + norm, slack=pass_slack[norm])
    finally:
        q.close()
    monkeypatch.delenv("KIWI_HIP_CHUNK_MB")
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = build(COMPS, engine=multi_engine(2))             # two contexts (stacked on device 0 where there is one device)
    try:
        assert m2.ndevices() == 2
        fc.floating(m2, sc, RANGES_A)
        for norm, b in base.items():
            for piece in (0, 2 * K):
                got = m2.linear_fit_candidates_floating_bootstrap_params("moment_tensor", rows, K, cand, dw, piece=piece, outer_norm=norm,
                                                                         anarchy=True, per_group=True)
                fc.assert_boot(got, as_dict(b), "two contexts, piece %d" % piece, slack=slack)
    finally:
        m2.close()


def test_a_group_with_a_failed_basis_source_never_wins():
    sc, p = build(COMPS)
    try:
        fc.floating(p, sc, RANGES_A)
        _, good3 = eikonal_list_with_a_failed_piece(p)        # (sets the crust and the constraints; its lists are made below)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        good = np.tile(good3[:1], (6, 1))
        good[:, 13:19] = np.random.default_rng(6).standard_normal((6, 6)) * 1e18
        dw = fc.draw_rows(sc.nrec, 12, range(sc.nrec), [], seed=6)
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, per_group=True)
            whole = p.linear_fit_candidates_floating_bootstrap_params("mt_eikonal", good, 2, cand, dw, **kw)
            assert np.all(whole.status == 0) and np.any(whole.group_shift)
            for piece, bad in ((0, [3]), (2, [2, 3])):        # piece 2 with both sources bad: a piece of which nothing is uploaded
                eik = good.copy()
                eik[bad, 3] = 500.0                           # "Empty rupture area": above the constraining planes
                got = p.linear_fit_candidates_floating_bootstrap_params("mt_eikonal", eik, 2, cand, dw, piece=piece, **kw)
                what = "%s piece %d" % (norm, piece)
                assert list(got.status) == [0, 2, 0], what
                assert np.all(np.isnan(got.group_value[1])) and np.all(got.group_cand[1] == -1) and not np.any(got.group_shift[1]), what
                assert np.all(got.best_group != 1), what
                for g in (0, 2):                              # the other groups' bits are unchanged
                    assert np.array_equal(np.isnan(got.group_value[g]), np.isnan(whole.group_value[g])), what
                    if common.arith() == "exact":
                        assert np.array_equal(got.group_value[g], whole.group_value[g], equal_nan=True), what
                        assert np.array_equal(got.group_cand[g], whole.group_cand[g]) and np.array_equal(got.group_shift[g], whole.group_shift[g]), what
                # the call's best is the best of the two groups that are left, its shifts that group's
                two = np.where(got.group_value[2] < got.group_value[0], 2, 0)
                has = ~np.isnan(got.best_value)
                assert np.array_equal(np.nonzero(~has)[0], [1, 2]), what
                assert np.array_equal(got.best_group[has], two[has]), what
                assert np.array_equal(got.best_value, np.fmin(got.group_value[0], got.group_value[2]), equal_nan=True), what
                assert np.array_equal(got.best_shift[has], got.group_shift[two[has], np.nonzero(has)[0]]), what
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_name_the_reason_and_leave_the_context_usable():
    sc, p = build(COMPS)
    try:
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        dw = fc.draw_rows(sc.nrec, 4, range(sc.nrec), [])
        p.set_source_params("moment_tensor", rows)
        fc.floating(p, sc, RANGES_A)
        boot_before = p.linear_fit_candidates_floating_bootstrap(0, 2, 6, cand, dw, per_group=True)

        def still_usable():
            again = p.linear_fit_candidates_floating_bootstrap(0, 2, 6, cand, dw, per_group=True)
            for name in again._fields:
                assert np.array_equal(getattr(again, name), getattr(boot_before, name), equal_nan=True), name

        still_usable()
        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)               # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, isrc0=0, ngroup=2, listed=True, ndraw=4, draws=dw, weights=None,
                  groups=(True, True, True), null=None):
            """both C entries with these arguments: refused, with the call's name in front and the reason in the message"""
            bv, bg, bcd, bs, st = np.zeros(64), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(512, np.int32), np.zeros(8, np.int32)
            gv, gc, gs = np.zeros(512), np.zeros(512, np.int32), np.zeros(4096, np.int32)
            x = np.ascontiguousarray(x, np.float64)
            d = None if draws is None else np.ascontiguousarray(draws, np.float64)
            w = None if weights is None else np.ascontiguousarray(weights, np.float64)
            outs = dict(best_value=dp(bv), best_group=ip(bg), best_cand=ip(bcd), best_shift=ip(bs), status=ip(st))
            if null:
                outs[null] = None
            tail = (ncand, dp(x), outer, dp(w), 0, ndraw, dp(d), outs["best_value"], outs["best_group"], outs["best_cand"], outs["best_shift"],
                    outs["status"], dp(gv) if groups[0] else None, ip(gc) if groups[1] else None, ip(gs) if groups[2] else None)
            rc = p.L.kiwi_hip_linear_fit_candidates_floating_bootstrap(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating_bootstrap: .*" + match):
                p._ck(rc, "linear_fit_candidates_floating_bootstrap")
            if listed:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_linear_fit_candidates_floating_bootstrap_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_floating_bootstrap: .*" + match):
                    p._ck(rc, "linear_fit_candidates_floating_bootstrap")
                p.set_source_params("moment_tensor", rows)    # (a failed list call leaves no batch the engine may index)

        # what this call adds
        entry("ndraw = 0; at least one draw", ndraw=0)
        entry("at least one draw", ndraw=-2)
        entry("null draw_weights", draws=None)
        for name in ("best_value", "best_group", "best_cand", "best_shift", "status"):
            entry("null draw_weights, best_value, best_group, best_cand, best_shift or status", null=name)
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
        # what the parent refuses of K, ncand, the candidates and the outer norm
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
        # the method: floating_l1norm by its name, everything else sent to floating_l2norm
        p.set_misfit_method("floating_l1norm")
        entry("floating_l1norm.*not quadratic")
        for method in ("l2norm", "l1norm", "ampspec_l2norm"):
            p.set_misfit_method(method)
            entry("must be floating_l2norm")
        p.set_misfit_method("floating_l2norm")
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_candidates_floating_bootstrap(0, 2, 6, cand, dw, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.linear_fit_candidates_floating_bootstrap(0, 2, 6, cand[:, :5], dw)
        with pytest.raises(KiwiHipError, match=r"draw_weights must be \[ndraw, 6\]"):
            p.linear_fit_candidates_floating_bootstrap(0, 2, 6, cand, dw[:, :5])
        still_usable()
    finally:
        p.close()


def test_one_receiver_more_than_the_layout_holds_is_refused():
    from tests.test_linfit_candidates_bootstrap_gpu import wide_scenario
    import ctypes
    from kiwi_amd import lib as klib
    c, t, r = (ctypes.c_int() for _ in range(3))
    assert klib.load().kiwi_hip_linear_fit_candidates_floating_bootstrap_shape(6, ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)) == 0
    Rmax = r.value
    sc = wide_scenario(Rmax + 1)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(1), 1, 6))
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(0, 0.0, 0.0)
        cand = np.random.default_rng(2).uniform(-1.0, 1.0, (3, 6))
        with pytest.raises(KiwiHipError, match=r"nok > linear_fit_candidates_floating_bootstrap: %d receivers.*at most %d" % (Rmax + 1, Rmax)):
            p.linear_fit_candidates_floating_bootstrap(0, 1, 6, cand, np.ones((2, Rmax + 1)))
        assert np.all(p.linear_fit_candidates_floating(0, 1, 6, cand).status == 0)        # the context is still usable
    finally:
        p.close()


def test_most_receivers_the_lds_layout_holds():
    """as many receivers of one component as the candidate kernel's LDS layout holds (the Gram sibling's
    test_receivers_against_the_lds_layout): ranges of one shift (every receiver but three), of shifts on one side only and of S + 1
    shifts, one more than an LDS stage -- on the LAST receiver, which alone decides draw 3; two groups, 70 candidates, 2 T + 1 draws,
    bits as in case 1"""
    from tests.test_linfit_candidates_bootstrap_gpu import wide_scenario
    import ctypes
    from kiwi_amd import lib as klib
    K = 6
    c, t, r = (ctypes.c_int() for _ in range(3))
    assert klib.load().kiwi_hip_linear_fit_candidates_floating_bootstrap_shape(K, ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)) == 0
    nrec = r.value
    sc = wide_scenario(nrec)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        C, T, Rmax = p.linear_fit_candidates_floating_bootstrap_shape(K)
        S = p.linear_fit_candidates_floating_shape(K)[2]
        assert nrec == Rmax == 131
        ranges = {1: (1, 4), 4: (-2, 2), nrec - 1: (-(S // 2), S // 2)}
        assert ranges[nrec - 1][1] - ranges[nrec - 1][0] + 1 == S + 1
        p.switch_receiver(3, False)
        rng = np.random.default_rng(nrec)
        p.set_source_params("moment_tensor", scattered_groups(rng, 2, K))
        p.set_misfit_method("floating_l2norm")
        p.set_floating_shiftrange(0, 0.0, 0.0)
        for ir, (lo, hi) in ranges.items():
            p.set_floating_shiftrange(ir + 1, lo * sc.gf["dt"], hi * sc.gf["dt"])
        w = rng.uniform(0.5, 2.0, nrec)
        w[nrec - 2] = 0.0
        cand = rng.uniform(-2.0, 2.0, (70, K))
        counted = [i for i in range(nrec) if i not in (2, nrec - 2)]
        dw = fc.draw_rows(nrec, 2 * T + 1, counted, [2, nrec - 2], seed=1)
        dw[3] = 0.0
        dw[3, nrec - 1] = 1.0                                 # the last receiver alone decides
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                what = "%d receivers %s anarchy=%s" % (nrec, norm, anarchy)
                want = fc.host_route(p, 0, 2, K, cand, dw, norm, w, anarchy)
                excluded = np.isnan(want["best_value"])
                assert np.array_equal(np.nonzero(excluded)[0], [1, 2]) and np.all(want["status"] == 0), what
                assert np.all(want["best_shift"][~excluded, 1] >= 1) and np.all(want["best_shift"][~excluded, 1] <= 4), what
                assert not np.any(want["best_shift"][:, [2, nrec - 2]]), what
                got = p.linear_fit_candidates_floating_bootstrap(0, 2, K, cand, dw, outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                                 per_group=True)
                assert got.best_shift.shape == (2 * T + 1, nrec) and got.group_shift.shape == (2, 2 * T + 1, nrec), what
                fc.assert_boot(got, want, what, same_batch=True)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 6: the helper and the example
def test_planted_double_couple_depth_and_delays_through_the_helper():
    """data of a planted double couple at 11 km, every station late by its own whole number of samples, noise-free: every draw that
    is not excluded finds the planted depth and mechanism, and the planted delays; the helper's rows agree with the host route"""
    sdr, moment = (40.0, 60.0, 100.0), 5e18
    planted = np.array(synthetic.mt_from_sdr(*sdr, moment), np.float32)
    from tests.common import Scenario
    sc = Scenario(comps_list=COMPS, true_type=6, true_params=mt_row(planted, location=[0., 0., 0., 11000.]))
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
        rows = np.stack([mt_row(np.zeros(6), location=[0., 0., 0., depth]) for depth in (10000., 11000., 12000.)])
        dw = fc.draw_rows(nrec, 24, range(nrec), [], seed=8)
        for norm in ("l1norm", "l2norm"):
            res = mtfit.bootstrap_double_couples_floating(p, "moment_tensor", rows, *grid, dw, moment=moment, outer_norm=norm, per_group=True)
            assert np.all(res["status"] == 0) and p.nsrc == 18
            has = ~np.isnan(res["misfit"])
            assert np.array_equal(np.nonzero(~has)[0], [1, 2])                      # the rows of zeros
            assert res["row"][1] == -1 and np.isnan(res["strike"][1]) and np.isnan(res["moment"][1]) and not np.any(res["shifts"][1])
            assert np.all(res["row"][has] == 1) and res["misfit"][0] < 1e-3
            assert np.all(res["strike"][has] == sdr[0]) and np.all(res["dip"][has] == sdr[1]) and np.all(res["rake"][has] == sdr[2])
            assert np.all(res["moment"][has] == moment)
            assert np.array_equal(res["shifts"][has], np.tile(-np.array(delays) * dt, (int(has.sum()), 1)))
            assert res["rows_misfit"].shape == res["rows_strike"].shape == (3, 24) and res["rows_shifts"].shape == (3, 24, nrec)
            assert np.all(res["rows_misfit"][1][has] <= res["rows_misfit"][0][has])
            cand = mtfit.double_couple_candidates(*grid, moment / 1e18)[0]
            want = fc.host_route(p, 0, 3, 6, cand, dw, norm, None, False)
            fc.assert_boot(res["boot"], want, "helper " + norm, same_batch=True)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith(), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_station_shifts_bootstrap.py"), "--small"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted depth and mechanism win most draws, planted delays are the modes" in out.stdout, out.stdout
    assert "wins" in out.stdout and "spread" in out.stdout, out.stdout
