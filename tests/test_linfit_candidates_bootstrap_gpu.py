"""kiwi_hip_linear_fit_candidates_bootstrap on the device.  The yardstick is the host route that defines the call, on the same
context: `linear_fit_candidates_time_scan(..., receiver_misfit=True)`, then `Engine.outer_misfits` on its float arrays read as
ngroup x nk x ncand sources of one slot per receiver -- once for all groups (best_*), once per group (group_*)
(tests/linfit_candidates_bootstrap_cases.py host_route).  Bit for bit under the `exact` arithmetic contract, whatever the number of
candidates against the kernel's tile, of draws against its draw tile, of receivers against its LDS layout, and however the call is
cut into chunks, draw passes, pieces and devices; also against the numpy restatement fed with the parent's sums; a failed basis
source; refusals; the helper and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd import mtfit
from kiwi_amd.engine import CandidateBootstrap
from kiwi_amd.lib import KiwiHipError, c_double_p, c_float_p, c_int_p
from tests import common
from tests import linfit_candidates_bootstrap_cases as bc
from tests import linfit_candidates_bootstrap_restatement as br
from tests import linfit_candidates_timescan_cases as cc
from tests import linfit_timescan_cases as lc
from tests.common import Scenario
from tests.linfit_cases import PLANTED, mt_row
from tests.test_linfit_candidates_gpu import zero_reference
from tests.test_linfit_gpu import FILTER, colocated_groups, multi_engine, scattered_groups
from tests.timescan_cases import offsets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts
SCAN = (-2, 2)                                                # k0, kstep


def standard_with_skipped_receivers():
    """tests/test_linfit_gpu.py's six receivers: receiver 6 disabled, receiver 4 with references of zeros; WEIGHTS gives receiver 2
    the weight 0.  Receivers 4 and 6 (indices 3, 5) are skipped whatever the weights"""
    sc, p = lc.standard()
    zero_reference(p, sc, 4)
    return sc, p


# ------------------------------------------------------------------------------------------------ 1: device == host route
@pytest.mark.parametrize("K,ngroup", [(1, 1), (1, 3), (6, 1), (6, 3), (8, 1), (8, 3)])
def test_device_equals_host_route_bit_for_bit(K, ngroup):
    sc, p = standard_with_skipped_receivers()
    try:
        C, T, Rmax = p.linear_fit_candidates_bootstrap_shape(K)
        assert C == 256 and Rmax >= sc.nrec
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
        for nk in (1, 3):
            for ncand in (1, C - 1, C + 1, 2 * C + 3):
                for norm in ("l1norm", "l2norm"):
                    for anarchy in (False, True):
                        for w in (WEIGHTS, None):
                            kw = dict(outer_norm=norm, receiver_weights=w, anarchy=anarchy)
                            want = bc.host_route(p, 0, ngroup, K, cand[:ncand], dw, *SCAN, nk, norm, w, anarchy)
                            for ndraw in ((1, T - 1, T, T + 1, 2 * T + 1) if w is not None else (2 * T + 1,)):
                                got = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw[:ndraw], *SCAN, nk, per_group=True, **kw)
                                what = "K=%d ngroup=%d nk=%d ncand=%d %s anarchy=%s weights=%s ndraw=%d" % (
                                    K, ngroup, nk, ncand, norm, anarchy, w is not None, ndraw)
                                bc.assert_boot(got, want, what, ndraw, same_batch=True)
                                ncalls += 1
                                assert np.all(got.status == 0), what
                                assert not np.isnan(got.best_value[0]) and got.best_cand[0] >= 0, what        # the row of ones
                                if ndraw >= 3:                # all zeros; non-zero only on skipped receivers
                                    assert np.all(np.isnan(got.best_value[1:3])) and np.all(got.best_group[1:3] == -1), what
                                    assert np.all(got.best_offset[1:3] == -1) and np.all(got.best_cand[1:3] == -1), what
                                    assert np.all(np.isnan(got.group_value[:, 1:3])) and np.all(got.group_cand[:, 1:3] == -1), what
                                if common.arith() == "exact":
                                    assert np.all(got.best_cand != C - 1) and np.all(got.best_cand != C), what      # the lowest index of a tie
                                    assert np.all(got.best_group != 2), what                                        # the lower group of a tie
                                    if ngroup == 3:
                                        assert np.array_equal(got.group_value[0], got.group_value[2], equal_nan=True), what
                            got = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand[:ncand], dw, *SCAN, nk, **kw)
                            assert got.group_value is None and got.group_offset is None and got.group_cand is None
                            bc.assert_boot(got, want, "no group arrays", same_batch=True)
        ms = p.linear_fit_candidates_bootstrap_ms()
        assert len(ms) == 5 and all(t > 0 for t in ms[:4]) and ms[4] >= 0
        print("K=%d ngroup=%d: %d device calls against the host route" % (K, ngroup, ncalls))
    finally:
        p.close()


def test_device_equals_restatement_fed_with_the_parents_sums():
    """the sums of every (group, offset) from the parent's linear_fit on the moved context (route B of
    tests/linfit_timescan_cases.py: the bits linear_fit_time_scan forms), the composition of the two restatements on them"""
    K, ngroup, nk = 6, 2, 3
    sc, p = standard_with_skipped_receivers()
    try:
        C, T, _ = p.linear_fit_candidates_bootstrap_shape(K)
        rng = np.random.default_rng(77)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = bc.draw_rows(sc.nrec, 2 * T + 1, [0, 2, 4], [3, 5], seed=9)
        wz = np.where([True] * 5 + [False], WEIGHTS, 0.0)
        for anarchy in (False, True):
            nbr, normal, fits = cc.route_b_sums(p, sc, offsets(*SCAN, nk), ngroup, K, WEIGHTS, anarchy)
            slack = float(np.max(cc.slack_of(nbr, wz, cand)))
            for norm in ("l1norm", "l2norm"):
                rs = br.evaluate(nbr, normal, wz, anarchy, cand, norm, dw)
                got = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand, dw, *SCAN, nk, outer_norm=norm, receiver_weights=WEIGHTS,
                                                        anarchy=anarchy, per_group=True)
                bc.assert_boot(got, rs, "restatement %s anarchy=%s" % (norm, anarchy), slack=slack)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 2: the plain case
def test_one_offset_at_zero_equals_the_route_through_linear_fit_candidates():
    K, ngroup = 6, 3
    sc, p = standard_with_skipped_receivers()
    try:
        C, T, _ = p.linear_fit_candidates_bootstrap_shape(K)
        rng = np.random.default_rng(5)
        p.set_source_params("moment_tensor", scattered_groups(rng, ngroup, K))
        cand = rng.uniform(-2.0, 2.0, (C + 1, K))
        dw = bc.draw_rows(sc.nrec, T + 1, [0, 2, 4], [3, 5], seed=2)
        fit = p.linear_fit(0, ngroup, K, receiver_weights=WEIGHTS, by_receiver=True)
        slack = float(np.max(cc.slack_of(fit.by_receiver[:, None], np.where([True] * 5 + [False], WEIGHTS, 0.0), cand)))
        for norm in ("l1norm", "l2norm"):
            for anarchy in (False, True):
                plain = p.linear_fit_candidates(0, ngroup, K, cand, outer_norm=norm, receiver_weights=WEIGHTS, anarchy=anarchy, receiver_misfit=True)
                want = br.from_scan(plain.receiver_misfit[:, None], plain.receiver_norm, plain.status, dw, norm, WEIGHTS, anarchy,
                                    outer=lambda m, n, s, nrec, nm, w, an, d: p.outer_misfits(
                                        m[:, :, None], n[:, :, None], outer_norm=nm, receiver_weights=w, anarchy=an, draw_weights=d,
                                        ncomponents=[1] * nrec))
                got = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand, dw, outer_norm=norm, receiver_weights=WEIGHTS, anarchy=anarchy,
                                                        per_group=True)
                bc.assert_boot(got, want, "plain %s anarchy=%s" % (norm, anarchy), slack=slack)
                assert np.all(got.best_offset[[0] + list(range(3, T + 1))] == 0)
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


def _receiver_counts():
    from kiwi_amd import lib as klib
    import ctypes
    L = klib.load()
    c, s, t, r = (ctypes.c_int() for _ in range(4))
    assert L.kiwi_hip_linear_fit_candidates_shape(6, ctypes.byref(c), ctypes.byref(s)) == 0
    assert L.kiwi_hip_linear_fit_candidates_bootstrap_shape(6, ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)) == 0
    return sorted(set([s.value + 1, r.value])), r.value


@pytest.mark.parametrize("nrec", _receiver_counts()[0])
def test_receivers_against_the_lds_layout(nrec):
    """S + 1 receivers of one component (one more than the parents' LDS stage) and the most the layout holds: two groups, 70
    candidates, 2 T + 1 draws, bits as in case 1"""
    sc = wide_scenario(nrec)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        C, T, Rmax = p.linear_fit_candidates_bootstrap_shape(6)
        assert nrec <= Rmax <= 511
        p.switch_receiver(3, False)
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
                want = bc.host_route(p, 0, 2, 6, cand, dw, -2, 3, 2, norm, w, anarchy)
                got = p.linear_fit_candidates_bootstrap(0, 2, 6, cand, dw, -2, 3, 2, outer_norm=norm, receiver_weights=w, anarchy=anarchy,
                                                        per_group=True)
                bc.assert_boot(got, want, "%d receivers %s anarchy=%s" % (nrec, norm, anarchy), same_batch=True)
                assert not np.any(np.isnan(got.best_value[3:])) and np.all(np.isnan(got.best_value[1:3]))
    finally:
        p.close()


def test_one_receiver_more_than_the_layout_holds_is_refused():
    Rmax = _receiver_counts()[1]
    assert Rmax <= 511                                        # (the yardstick's own limit, kiwi_hip_outer_max_receivers(), is not the one met)
    sc = wide_scenario(Rmax + 1)
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        assert p.outer_max_receivers() > Rmax
        p.set_source_params("moment_tensor", scattered_groups(np.random.default_rng(1), 1, 6))
        cand = np.random.default_rng(2).uniform(-1.0, 1.0, (3, 6))
        with pytest.raises(KiwiHipError, match=r"nok > linear_fit_candidates_bootstrap: %d receivers.*at most %d" % (Rmax + 1, Rmax)):
            p.linear_fit_candidates_bootstrap(0, 1, 6, cand, np.ones((2, Rmax + 1)))
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
    base, passes = {}, {}
    sc, p = lc.standard()
    try:
        C, T, _ = p.linear_fit_candidates_bootstrap_shape(K)
        dw = bc.pack_draws(sc.nrec)
        p.set_source_params("moment_tensor", rows)
        nbr = p.linear_fit(0, ngroup, K, by_receiver=True).by_receiver
        slack = float(np.max(cc.slack_of(nbr[:, None], np.where([True] * 5 + [False], 1.0, 0.0), cand))) * 4     # (offsets: other windows of the same traces)
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, anarchy=True, per_group=True)
            p.set_source_params("moment_tensor", rows)
            b = base[norm] = p.linear_fit_candidates_bootstrap(0, ngroup, K, cand, dw, *lc.CHUNK_SCAN, **kw)
            bc.assert_boot(b, bc.host_route(p, 0, ngroup, K, cand, dw, *lc.CHUNK_SCAN, norm, None, True), "base " + norm, same_batch=True)
            print(norm, "winners of the draws (group, offset, candidate):", sorted(set(zip(b.best_group[3:], b.best_offset[3:], b.best_cand[3:]))))
            p.set_source_params("moment_tensor", np.concatenate([head, rows]))
            bc.assert_boot(p.linear_fit_candidates_bootstrap(5, ngroup, K, cand, dw, *lc.CHUNK_SCAN, **kw), as_dict(b), "isrc0 = 5", slack=slack)
            for piece in (K, 2 * K, 0):
                got = p.linear_fit_candidates_bootstrap_params("moment_tensor", rows, K, cand, dw, *lc.CHUNK_SCAN, piece=piece, **kw)
                bc.assert_boot(got, as_dict(b), "piece %d" % piece, slack=slack)
                assert p.nsrc == (piece or p.nsrc)
                p.eval()                                      # the engine holds the head of the list and knows how long it is
            # the case whose draws go in passes in the child below, here in one pass, against the host route
            p.set_source_params("moment_tensor", bc.pass_rows())
            pdw = bc.draw_rows(sc.nrec, bc.PASS_NDRAW, range(5), [5], seed=4)
            pc = bc.pass_candidates(C)
            assert bc.PASS_SCAN[2] * ((len(pc) + C - 1) // C) * 12 * bc.PASS_NDRAW > 1 << 20       # one group's slab against 1 MiB
            passes[norm] = p.linear_fit_candidates_bootstrap(0, bc.PASS_GROUPS, 6, pc, pdw, *bc.PASS_SCAN, **kw)
            bc.assert_boot(passes[norm], bc.host_route(p, 0, bc.PASS_GROUPS, 6, pc, pdw, *bc.PASS_SCAN, norm, None, True), "one pass " + norm, same_batch=True)
    finally:
        p.close()
    # several chunks, several draw passes: KIWI_HIP_CHUNK_MB is read when a context is made -- a process of its own
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_linfit_candidates_bootstrap_child_%d.npz" % os.getpid())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "linfit_candidates_bootstrap_cases.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, KIWI_HIP_CHUNK_MB="1"), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = dict(np.load(out))
    os.remove(out)
    for norm, b in base.items():
        assert z[norm + "_launches"][1] >= 2, z[norm + "_launches"]       # a chunk boundary between groups
        chunked = CandidateBootstrap(*[z[norm + "_" + name] for name in CandidateBootstrap._fields])
        bc.assert_boot(chunked, as_dict(b), "chunks " + norm, slack=slack)
        cut = CandidateBootstrap(*[z[norm + "_pass_" + name] for name in CandidateBootstrap._fields])
        bc.assert_boot(cut, as_dict(passes[norm]), "draw passes " + norm, slack=slack)
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = lc.standard(engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        for norm, b in base.items():
            for piece in (0, 2 * K):
                got = m2.linear_fit_candidates_bootstrap_params("moment_tensor", rows, K, cand, bc.pack_draws(sc.nrec), *lc.CHUNK_SCAN, piece=piece,
                                                                outer_norm=norm, anarchy=True, per_group=True)
                bc.assert_boot(got, as_dict(b), "two contexts, piece %d" % piece, slack=slack)
    finally:
        m2.close()


# ------------------------------------------------------------------------------------------------ 5: a failed basis source
def test_a_group_with_a_failed_basis_source_never_wins():
    sc, p = lc.standard()
    try:
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 2))
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (6, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((6, 6)) * 1e18
        dw = bc.draw_rows(sc.nrec, 12, range(5), [5], seed=6)
        good = eik.copy()
        for norm in ("l1norm", "l2norm"):
            kw = dict(outer_norm=norm, per_group=True)
            whole = p.linear_fit_candidates_bootstrap_params("mt_eikonal", good, 2, cand, dw, -1, 1, 3, **kw)
            assert np.all(whole.status == 0)
            for piece, bad in ((0, [3]), (2, [2, 3])):        # piece 2 with both sources bad: a piece of which nothing is uploaded
                eik = good.copy()
                eik[bad, 3] = 500.0                           # "Empty rupture area": above the constraining planes
                got = p.linear_fit_candidates_bootstrap_params("mt_eikonal", eik, 2, cand, dw, -1, 1, 3, piece=piece, **kw)
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
        rows = colocated_groups(np.random.default_rng(4), 2)
        cand = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 6))
        dw = bc.draw_rows(sc.nrec, 4, range(5), [5])
        p.set_source_params("moment_tensor", rows)
        p.eval()
        before = p.get_misfits()
        boot_before = p.linear_fit_candidates_bootstrap(0, 2, 6, cand, dw, 0, 1, 2, per_group=True)

        def still_usable():
            p.eval()
            for x, y in zip(before, p.get_misfits()):
                assert common.same_bits(x, y)
            again = p.linear_fit_candidates_bootstrap(0, 2, 6, cand, dw, 0, 1, 2, per_group=True)
            for name in again._fields:
                assert np.array_equal(getattr(again, name), getattr(boot_before, name), equal_nan=True), name
            for x, y in zip(before, p.get_misfits()):         # after a success too: what a plain eval leaves
                assert common.same_bits(x, y)

        still_usable()
        dp = lambda a: None if a is None else a.ctypes.data_as(c_double_p)           # noqa: E731
        ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)               # noqa: E731

        def entry(match, K=6, ncand=5, x=cand, outer=2, scan=(0, 1, 2), isrc0=0, ngroup=2, listed=True, ndraw=4, draws=dw, weights=None,
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
            rc = p.L.kiwi_hip_linear_fit_candidates_bootstrap(p.h, isrc0, ngroup, K, *tail)
            assert rc != 0
            with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_bootstrap: .*" + match):
                p._ck(rc, "linear_fit_candidates_bootstrap")
            if listed:
                basis = np.ascontiguousarray(np.tile(rows[:1], (2 * max(K, 1), 1)), np.float32)
                rc = p.L.kiwi_hip_linear_fit_candidates_bootstrap_params(p.h, 6, 2, K, basis.ctypes.data_as(c_float_p), 0, *tail)
                assert rc != 0
                with pytest.raises(KiwiHipError, match="nok > linear_fit_candidates_bootstrap: .*" + match):
                    p._ck(rc, "linear_fit_candidates_bootstrap")
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
        # what the parents refuse of K, ncand, nk and the offsets
        for K in (0, 9):
            entry("basis sources per group", K=K)
        entry("at least one candidate", ncand=0)
        x = cand.copy()
        x[3, 2] = np.nan
        entry("entry 2 of candidate 3 is not finite", x=x)
        entry("outer_norm must be 1", outer=3)
        entry("need at least one offset", scan=(0, 1, 0))
        entry("257 offsets; at most 256", scan=(-128, 1, 257))
        entry("kstep = 0", scan=(0, 0, 3))
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
        p.set_misfit_method("l2norm")
        still_usable()
        # the Python methods name theirs
        with pytest.raises(KiwiHipError, match="unknown norm"):
            p.linear_fit_candidates_bootstrap(0, 2, 6, cand, dw, outer_norm="l3norm")
        with pytest.raises(KiwiHipError, match=r"\[ncand, K = 6\]"):
            p.linear_fit_candidates_bootstrap(0, 2, 6, cand[:, :5], dw)
        with pytest.raises(KiwiHipError, match=r"draw_weights must be \[ndraw, 6\]"):
            p.linear_fit_candidates_bootstrap(0, 2, 6, cand, dw[:, :5])
        still_usable()
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 7: the helper and the example
DC = (60.0, 60.0, -90.0, 3.0e18)
MECH = (range(0, 360, 30), range(0, 91, 30), range(-180, 180, 30))


def test_bootstrap_double_couples_finds_the_planted_node_and_agrees_with_the_host_route():
    """3 depths x 3 offsets x 12 x 4 x 12 double couples at 30 degrees; the references are the double couple DC at 11 km, one
    sample later than the rows"""
    dt = Scenario().gf["dt"]
    tensor = mtfit.double_couple_candidates([DC[0]], [DC[1]], [DC[2]], DC[3])[0][0].astype(np.float32)
    sc = Scenario(true_type=6, true_params=mt_row(tensor, location=[dt, 0., 0., 11000.]))
    sc.make_references(sc.oracle())
    p = sc.product()
    sc.apply_setup(p, False)
    try:
        rows = np.stack([mt_row(np.zeros(6), location=[0., 0., 0., depth]) for depth in (10000., 11000., 12000.)])
        dw = bc.draw_rows(sc.nrec, 24, range(sc.nrec), [], seed=8)
        planted = mtfit.double_couple_candidates(*[[v] for v in DC[:3]], DC[3])[0][0]
        tensors = mtfit.double_couple_candidates(*MECH, DC[3])[0]
        for norm in ("l1norm", "l2norm"):
            res = mtfit.bootstrap_double_couples(p, "moment_tensor", rows, *MECH, dw, moment=DC[3], k0=-1, kstep=1, nk=3, outer_norm=norm,
                                                 per_group=True)
            assert np.all(res["status"] == 0) and p.nsrc == 18
            assert res["row"][0] == 1 and res["offset"][0] == 2 and res["misfit"][0] <= 1e-4       # draw 0, all ones: the planted node
            assert np.all(np.abs(tensors[res["index"][0]] - planted) <= 1e-4 * DC[3])            # (the mechanism or its auxiliary plane)
            assert [res["strike"][0], res["dip"][0], res["rake"][0]] == list(mtfit.double_couple_candidates(*MECH, 1.0)[1][res["index"][0]])
            assert np.isnan(res["misfit"][1]) and res["row"][1] == -1 and np.isnan(res["strike"][1])      # the row of zeros
            has = ~np.isnan(res["misfit"])
            assert np.all(res["row"][has] == 1) and np.all(res["offset"][has] == 2)                # noise-free data: every draw finds it
            assert res["rows_misfit"].shape == res["rows_strike"].shape == res["rows_offset"].shape == (3, 24)
            assert np.all(res["rows_misfit"][1][has] <= res["rows_misfit"][0][has]) and np.all(res["rows_offset"][1][has] == 2)
            # its rows agree with the route of case 1
            cand = mtfit.double_couple_candidates(*MECH, DC[3] / 1e18)[0]
            want = bc.host_route(p, 0, 3, 6, cand, dw, -1, 1, 3, norm, None, False)
            bc.assert_boot(res["boot"], want, "helper " + norm, same_batch=True)
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, KIWI_HIP_ARITH=common.arith(), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_double_couple_bootstrap.py"), "--small"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "planted depth wins" in out.stdout and "spread of strike" in out.stdout, out.stdout
