"""kiwi_hip_outer_misfits on the device (kiwi_amd/csrc/kiwi_outer.hpp): the outer misfit of every trial source under B
receiver weightings and the best source of each, against the CPU restatement (tests/outer_restatement.py) bit for bit,
against the host path make_global_misfits within the derived bound, through MisfitGrid.postprocess(engine=...), and cut
into shards."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from kiwi_amd import shard
from kiwi_amd.engine import make_global_misfits
from kiwi_amd.lib import KiwiHipError
from tests import outer_cases as K
from tests import outer_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def engine():
    from kiwi_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def components(nrec):
    return [1 + (r % 5) for r in range(nrec)]          # receivers with 1 to 5 components


def same(got, want):
    return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)


def check_against_restatement(e, ns, nrec, ndraw, opt, seed, failing=None):
    outer_norm, anarchy, weighted, masked = opt
    ncomp = components(nrec)
    failing = tuple(s for s in ((0, ns // 2) if failing is None else failing) if s < ns and ns > 2)
    mis, nor = K.make_case(ns, ncomp, seed, failing=failing)
    w, _, dw = K.draws_for(nrec, ndraw, seed + 100, weighted, masked)
    which = ndraw // 2
    mf, nf, sr = R.flatten(mis, nor, ncomp)
    want_v, want_i, want_g = R.outer_misfits(mf, nf, sr, nrec, outer_norm, w, anarchy, dw, which_draw=which)
    got_v, got_i, got_g = e.outer_misfits(mis, nor, outer_norm, w, anarchy, dw, which_draw=which, ncomponents=ncomp)
    assert same(got_g, want_g), "global_of_draw: %d of %d sources differ" % (int(np.sum(~(np.isclose(got_g, want_g, 0, 0, True)))), ns)
    assert same(got_i, want_i), "best_index differs in draws %s" % np.nonzero(got_i != want_i)[0][:10]
    assert same(got_v, want_v), "best_value differs in draws %s" % np.nonzero(~np.isclose(got_v, want_v, 0, 0, True))[0][:10]
    assert got_v.dtype == np.float64 and got_i.dtype == np.int32 and got_g.dtype == np.float64
    for s in failing:
        assert np.isnan(got_g[s])
    return got_v, got_i, got_g


@pytest.mark.parametrize("opt", K.OPTIONS, ids=K.option_id)
def test_device_is_the_restatement_bit_for_bit_over_the_options(engine, opt):
    check_against_restatement(engine, 4097, 50, 7, opt, seed=31)


def _limit():
    from kiwi_amd import lib as klib
    return int(klib.load().kiwi_hip_outer_max_receivers())


# (N_s, N_r or None = the limit, ndraw): every N_s of 1, 63, 4097 with every N_r of 1, 50, the limit, and the draws spread
SIZES = [(1, 1, 1), (1, 50, 7), (1, None, 1000), (63, 1, 1000), (63, 50, 1), (63, None, 7), (4097, 1, 7), (4097, 50, 1000),
         (4097, None, 1)]


@pytest.mark.parametrize("i", range(len(SIZES)), ids=["%dx%sx%d" % (s, r or "limit", d) for s, r, d in SIZES])
def test_device_is_the_restatement_bit_for_bit_over_the_sizes(engine, i):
    ns, nrec, ndraw = SIZES[i]
    if nrec is None:
        nrec = _limit()
        assert nrec >= 512
    for opt in (K.OPTIONS[(5 * i) % 16], K.OPTIONS[(5 * i + 11) % 16]):
        check_against_restatement(engine, ns, nrec, ndraw, opt, seed=50 + i)


@pytest.mark.parametrize("outer_norm", ["l1norm", "l2norm"])
def test_a_list_that_spans_several_chunks(monkeypatch, engine, outer_norm):
    """KIWI_HIP_CHUNK_MB is read at kiwi_hip_init: a context of its own, 1 MiB of workspace, about 500 sources per chunk."""
    from kiwi_amd import Engine
    monkeypatch.setenv("KIWI_HIP_CHUNK_MB", "1")
    small = Engine(0)
    try:
        opt = (outer_norm, True, True, True)
        v, i, g = check_against_restatement(small, 4097, 50, 7, opt, seed=77, failing=(0, 1, 2, 700, 4096))
        v1, i1, g1 = check_against_restatement(engine, 4097, 50, 7, opt, seed=77, failing=(0, 1, 2, 700, 4096))
        assert same(v, v1) and same(i, i1) and same(g, g1)
        check_against_restatement(small, 4097, 50, 1000, (outer_norm, False, False, False), seed=78)
    finally:
        small.close()


def test_ties_answer_the_lower_index_and_empty_draws_index_zero(engine):
    ncomp = components(9)
    ns = 700
    mis, nor = K.make_case(ns, ncomp, seed=5, failing=(0, 300))
    # every source of the second half is a copy of one of the first half: each value occurs twice, 350 apart
    mis[350:], nor[350:] = mis[:350], nor[:350]
    w, _, dw = K.draws_for(9, 33, 9, True, False)
    for outer_norm in ("l1norm", "l2norm"):
        v, i, g = engine.outer_misfits(mis, nor, outer_norm, w, True, dw, which_draw=4, ncomponents=ncomp)
        assert same(g[:350], g[350:])
        assert np.all(i < 350) and np.all(i != 0) and np.all(i != 300)
        assert same(v, np.nanmin(R.draw_misfits(*R.prepare(*R.flatten(mis, nor, ncomp), 9, outer_norm, w, True), dw, outer_norm), 0))
    # a draw whose counts are zero on every receiver with data
    ncomp0 = [3, 0, 2, 0]
    mis, nor = K.make_case(100, ncomp0, seed=6)
    dw = np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 3.0, 0.0, 1.0], [2.0, 0.0, 0.0, 2.0]])
    v, i, g = engine.outer_misfits(mis, nor, "l2norm", None, False, dw, which_draw=1, ncomponents=ncomp0)
    assert np.isnan(v[1]) and i[1] == 0 and np.all(np.isnan(g))
    assert np.isfinite(v[0]) and np.isfinite(v[2])
    mf, nf, sr = R.flatten(mis, nor, ncomp0)
    wv, wi, wg = R.outer_misfits(mf, nf, sr, 4, "l2norm", None, False, dw, which_draw=1)
    assert same(v, wv) and same(i, wi)
    # a list of failings only
    mis, nor = K.make_case(300, ncomp, seed=7, failing=range(300))
    v, i, g = engine.outer_misfits(mis, nor, "l1norm", None, True, K.draws_for(9, 5, 1, False, False)[2], which_draw=0,
                                   ncomponents=ncomp)
    assert np.all(np.isnan(v)) and np.all(i == 0) and np.all(np.isnan(g))


@pytest.mark.parametrize("opt", K.OPTIONS, ids=K.option_id)
def test_the_device_best_source_is_a_host_minimum_within_the_bound(engine, opt):
    """for every draw g_host[best_index_device] <= min(g_host) (1 + (N_r + 16) 2^-52)"""
    outer_norm, anarchy, weighted, masked = opt
    ncomp = components(50)
    mis, nor = K.make_case(3000, ncomp, seed=13, failing=(0, 1500))
    w, mask, dw = K.draws_for(50, 40, 4242, weighted, masked)
    _, bi, _ = engine.outer_misfits(mis, nor, outer_norm, w, anarchy, dw, ncomponents=ncomp)
    rng = np.random.default_rng(4242)
    worst = 0.0
    for d in range(40):
        gh = make_global_misfits(mis, nor, outer_norm, w, mask, anarchy, bootstrap=True, rng=rng)[0]
        worst = max(worst, gh[bi[d]] / np.nanmin(gh) - 1.0)
        assert gh[bi[d]] <= np.nanmin(gh) * (1.0 + K.ulp_bound(50)), d
    print("worst excess over the host minimum: %.2f x 2^-52" % (worst * 2.0 ** 52))


def _example():
    spec = importlib.util.spec_from_file_location("invert_bilateral", os.path.join(ROOT, "examples", "invert_bilateral.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SEED = 20261016


def test_postprocess_with_an_engine_gives_the_host_path_sources(engine):
    """The grid of examples/invert_bilateral.py, misfits from the engine, 200 draws: the same best source and the same
    list of bootstrap sources from equally seeded generators.  (A near-tie could legitimately part the two paths; the
    host's best and second-best are therefore shown to lie further apart than the bound in every draw, host path alone.)"""
    _, grid, _ = _example().main(verbose=False)
    cfg = dict(outer_norm="l2norm")
    # host path alone: the margin of every draw
    rng = np.random.default_rng(SEED)
    margins = []
    for d in range(201):
        g = make_global_misfits(grid.misfits_by_src, grid.norms_by_src, receiver_mask=grid.receiver_mask, bootstrap=d > 0,
                                rng=rng, **cfg)[0]
        two = np.sort(g[~np.isnan(g)])[:2]
        margins.append(two[1] / two[0] - 1.0)
    print("smallest relative gap between the host's best and second best: %.3e (bound %.3e)" % (min(margins), K.ulp_bound(grid.nreceivers)))
    assert min(margins) > 2 * K.ulp_bound(grid.nreceivers), "seed %d has a near-tie in draw %d" % (SEED, int(np.argmin(margins)))
    grid.postprocess(bootstrap_iterations=200, rng=np.random.default_rng(SEED), **cfg)
    host = (grid.ibest, grid.best_source.copy(), np.array(grid.bootstrap_sources), np.array(grid.misfits_by_s),
            np.array(grid.misfits_by_r), np.array(grid.variability_by_r), {k: (s.mean, s.std) for k, s in grid.stats.items()})
    grid.postprocess(bootstrap_iterations=200, rng=np.random.default_rng(SEED), engine=engine, **cfg)
    assert grid.ibest == host[0]
    assert np.array_equal(grid.best_source, host[1])
    assert np.array_equal(np.array(grid.bootstrap_sources), host[2])
    assert len(grid.bootstrap_sources) == 200
    ok = ~np.isnan(host[3])
    assert np.array_equal(np.isnan(grid.misfits_by_s), ~ok)
    assert np.all(np.abs(grid.misfits_by_s[ok] - host[3][ok]) <= K.ulp_bound(grid.nreceivers) * host[3][ok])
    assert np.array_equal(grid.misfits_by_r, host[4]) and np.array_equal(grid.variability_by_r, host[5])
    assert {k: (s.mean, s.std) for k, s in grid.stats.items()} == host[6]


@pytest.mark.parametrize("outer_norm", ["l1norm", "l2norm"])
def test_three_uneven_shards_combine_to_the_unsharded_answer(engine, outer_norm):
    ncomp = components(50)
    ns = 2500
    mis, nor = K.make_case(ns, ncomp, seed=17, failing=tuple(range(900, 1300)) + (0,))
    mis[2000:2400], nor[2000:2400] = mis[100:500], nor[100:500]            # ties across the cuts
    w, _, dw = K.draws_for(50, 64, 3, True, True)
    dw[5] = 0.0
    want_v, want_i, _ = engine.outer_misfits(mis, nor, outer_norm, w, True, dw, ncomponents=ncomp)
    cuts = [0, 901, 1290, ns]                                              # the middle shard holds failings only
    parts = [engine.outer_misfits(mis[lo:hi], nor[lo:hi], outer_norm, w, True, dw, ncomponents=ncomp)
             for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.all(np.isnan(parts[1][0]))
    got_v, got_i = shard.combine_draw_minima([p[0] for p in parts], [p[1] for p in parts], cuts[:-1])
    assert same(got_v, want_v) and same(got_i, want_i)
    assert np.isnan(got_v[5]) and got_i[5] == 0
    # and through the one-process path of sharded_bootstrap
    sv, si = shard.sharded_bootstrap(engine, mis, nor, ns, outer_norm, w, True, dw, ncomponents=ncomp)
    assert same(sv, want_v) and same(si, want_i)


@pytest.mark.exact_only
def test_the_outer_step_does_not_depend_on_the_arithmetic_contract(engine):
    ncomp = components(50)
    mis, nor = K.make_case(1000, ncomp, seed=19, failing=(3,))
    w, _, dw = K.draws_for(50, 100, 23, True, False)
    res = {}
    for mode in ("exact", "fused"):
        engine.set_arithmetic(mode)
        res[mode] = engine.outer_misfits(mis, nor, "l2norm", w, True, dw, which_draw=7, ncomponents=ncomp)
    for a, b in zip(res["exact"], res["fused"]):
        assert same(a, b)
    up, kern, down = engine.outer_ms()
    assert kern > 0.0 and up >= 0.0 and down >= 0.0


def test_errors_come_through_last_error(engine):
    ncomp = [2, 2, 2]
    mis, nor = K.make_case(10, ncomp, seed=1)
    mf, nf, sr = R.flatten(mis, nor, ncomp)
    with pytest.raises(KiwiHipError, match="unknown norm"):
        engine.outer_misfits(mis, nor, "l3norm", ncomponents=ncomp)
    with pytest.raises(KiwiHipError, match="not ascending"):
        engine.outer_misfits_slots(mf, nf, sr[::-1], 3)
    with pytest.raises(KiwiHipError, match="out of range"):
        engine.outer_misfits_slots(mf, nf, sr + 1, 3)
    big = _limit() + 1
    with pytest.raises(KiwiHipError, match="at most %d" % _limit()):
        engine.outer_misfits_slots(mf, nf, sr, big)
    with pytest.raises(KiwiHipError, match="which_draw"):
        engine.outer_misfits_slots(mf, nf, sr, 3, which_draw=1)
    L = engine.L
    bv, bi = np.zeros(1), np.zeros(1, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))           # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))            # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))              # noqa: E731
    for counts in ((-1, 6, 3, 1), (10, -6, 3, 1), (10, 6, -3, 1), (10, 6, 3, -1)):
        rc = L.kiwi_hip_outer_misfits(engine.h, counts[0], counts[1], counts[2], ip(sr), fp(mf), fp(nf), 2, None, 0, counts[3],
                                      dp(np.ones((1, 3))), dp(bv), ip(bi), 0, None)
        assert rc != 0
        buf = C.create_string_buffer(256)
        L.kiwi_hip_last_error(engine.h, buf, 256)
        assert b"negative count" in buf.value
    # nothing above broke the context
    v, i, _ = engine.outer_misfits(mis, nor, "l2norm", ncomponents=ncomp)
    wv, wi, _ = R.outer_misfits(mf, nf, sr, 3)
    assert same(v, wv) and same(i, wi)
