"""The outer misfits under B receiver weightings (kiwi_hip_outer_misfits) without a GPU: the numpy restatement of the
device arithmetic (tests/outer_restatement.py) against the host path make_global_misfits, the draw matrix against
successive host draws, the sharded combine, and the C-ABI's declaration, export and binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from kiwi_amd import shard
from kiwi_amd.engine import bootstrap_draw_weights, make_global_misfits
from tests import outer_cases as K
from tests import outer_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDRAW = 40


@pytest.mark.parametrize("opt", K.OPTIONS, ids=K.option_id)
def test_restatement_is_the_host_path_within_the_derived_bound(opt):
    """Same NaNs, and |g_restated - g_host| <= (N_r + 16) 2^-52 g_host for every source of every one of 40 draws."""
    outer_norm, anarchy, weighted, masked = opt
    ncomp = [1 + (r % 5) for r in range(50)]
    nrec = len(ncomp)
    mis, nor = K.make_case(300, ncomp, seed=11, failing=(0, 137))
    w, mask, dw = K.draws_for(nrec, NDRAW, 2024, weighted, masked)
    mf, nf, sr = R.flatten(mis, nor, ncomp)
    a, b = R.prepare(mf, nf, sr, nrec, outer_norm, w, anarchy)
    g = R.draw_misfits(a, b, np.concatenate([np.ones((1, nrec)), dw]), outer_norm)
    host0, _ = make_global_misfits(mis, nor, outer_norm, w, mask, anarchy)
    rng = np.random.default_rng(2024)
    host = [host0] + [make_global_misfits(mis, nor, outer_norm, w, mask, anarchy, bootstrap=True, rng=rng)[0] for _ in range(NDRAW)]
    worst = 0.0
    for d, gh in enumerate(host):
        assert np.array_equal(np.isnan(g[:, d]), np.isnan(gh)), "draw %d: different sources excluded" % d
        ok = ~np.isnan(gh)
        assert np.isnan(gh[0]) and np.isnan(gh[137])
        assert ok.sum() == 298
        rel = np.abs(g[ok, d] - gh[ok]) / gh[ok]
        worst = max(worst, float(rel.max()))
    print("worst relative difference %.2f x 2^-52 (bound %d)" % (worst * 2.0 ** 52, nrec + 16))
    assert worst <= K.ulp_bound(nrec)
    # and the minima of the restatement are those of its own matrix by numpy's nanargmin
    bv, bi = R.minima(g)
    assert np.array_equal(bi, np.nanargmin(g, 0))
    assert np.array_equal(bv, np.nanmin(g, 0))


@pytest.mark.parametrize("weighted,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_draw_matrix_is_the_counts_of_successive_host_draws(weighted, masked):
    nrec, ndraw = 23, 17
    w = K.weights_with_a_zero(nrec, 5) if weighted else None
    mask = K.mask_with_gaps(nrec) if masked else None
    got = bootstrap_draw_weights(nrec, ndraw, np.random.default_rng(99), mask, w)
    # the host's own draws (engine.py make_global_misfits), from an equally seeded generator
    rng = np.random.default_rng(99)
    m = np.ones(nrec, bool) if mask is None else mask.copy()
    if w is not None:
        m = np.logical_and(m, w != 0)
    enabled = np.arange(nrec)[m]
    for d in range(ndraw):
        draw = enabled[rng.integers(0, len(enabled), len(enabled))]
        assert np.array_equal(got[d], np.bincount(draw, minlength=nrec).astype(np.float64)), d
    assert got.shape == (ndraw, nrec) and got.dtype == np.float64
    assert np.all(got.sum(1) == len(enabled))
    # and both generators have been consumed alike: whatever is drawn next is the same
    check = np.random.default_rng(99)
    bootstrap_draw_weights(nrec, ndraw, check, mask, w)
    rng2 = np.random.default_rng(99)
    for d in range(ndraw):
        rng2.integers(0, len(enabled), len(enabled))
    assert check.bit_generator.state == rng2.bit_generator.state


def test_draws_reach_the_host_path_through_the_draw_matrix():
    """make_global_misfits(bootstrap=True) d times and one bootstrap_draw_weights see the same draws: the host's global
    misfits follow from the matrix's row within the restatement's bound (checked above), here the best sources agree."""
    ncomp = [3] * 12
    mis, nor = K.make_case(200, ncomp, seed=3, decades=2.0)
    dw = bootstrap_draw_weights(12, 25, np.random.default_rng(7))
    mf, nf, sr = R.flatten(mis, nor, ncomp)
    _, bi, _ = R.outer_misfits(mf, nf, sr, 12, "l2norm", None, False, dw)
    rng = np.random.default_rng(7)
    for d in range(25):
        gh = make_global_misfits(mis, nor, "l2norm", bootstrap=True, rng=rng)[0]
        assert gh[bi[d]] <= np.nanmin(gh) * (1 + K.ulp_bound(12))


def test_combine_draw_minima_three_uneven_shards():
    rng = np.random.default_rng(21)
    ns, nd = 101, 64
    g = rng.integers(0, 6, (ns, nd)).astype(np.float64)          # few distinct values: ties everywhere
    g[rng.uniform(size=g.shape) < 0.2] = np.nan
    g[40:58, :] = np.nan                                          # the middle shard has no candidate at all
    g[:, 5] = np.nan                                              # nor has draw 5 anywhere
    g[:40, 9] = np.nan
    g[58:, 9] = np.nan                                            # and draw 9 nowhere
    want_v, want_i = R.minima(g)
    cuts = [0, 40, 58, ns]
    vals, idxs = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v, i = R.minima(g[lo:hi])
        vals.append(v)
        idxs.append(i)
    got_v, got_i = shard.combine_draw_minima(np.array(vals), np.array(idxs), cuts[:-1])
    assert np.array_equal(got_v, want_v, equal_nan=True)
    assert np.array_equal(got_i, want_i)
    assert np.isnan(got_v[5]) and got_i[5] == 0 and np.isnan(got_v[9]) and got_i[9] == 0
    has = ~np.isnan(want_v)
    assert np.array_equal(got_i[has], np.nanargmin(g[:, has], 0))
    # the order of the shards in the fold does not matter
    perm = [2, 0, 1]
    pv, pi = shard.combine_draw_minima(np.array(vals)[perm], np.array(idxs)[perm], np.array(cuts[:-1])[perm])
    assert np.array_equal(pv, want_v, equal_nan=True) and np.array_equal(pi, want_i)


class _RestatedEngine:
    """Engine.outer_misfits by the restatement: what sharded_bootstrap calls on every rank."""

    def outer_misfits(self, mis, nor, outer_norm="l2norm", receiver_weights=None, anarchy=False, draw_weights=None,
                      which_draw=None, ncomponents=None):
        mf, nf, sr = R.flatten(mis, nor, ncomponents)
        return R.outer_misfits(mf, nf, sr, np.asarray(mis).shape[1], outer_norm, receiver_weights, anarchy, draw_weights, which_draw)


def _sharded_case():
    ncomp = [1 + (r % 3) for r in range(8)]
    ns = 41
    mis, nor = K.make_case(ns, ncomp, seed=8, failing=(0, 30))
    mis[25:35], nor[25:35] = mis[5:15], nor[5:15]                 # ties across the cut
    dw = bootstrap_draw_weights(8, 12, np.random.default_rng(2))
    dw[3] = 0.0
    return ncomp, ns, mis, nor, dw


def _bootstrap_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ncomp, ns, mis, nor, dw = _sharded_case()
    lo, hi = shard.shard_range(ns, world, rank)
    mine = dw if rank == 0 else np.zeros_like(dw)                 # the draws come from rank 0
    v, i = shard.sharded_bootstrap(_RestatedEngine(), mis[lo:hi], nor[lo:hi], ns, "l2norm", None, True, mine, dist=dist,
                                   ncomponents=ncomp)
    q.put((rank, v, i))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_bootstrap_over_two_gloo_ranks_is_the_unsharded_answer():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bootstrap_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    ncomp, ns, mis, nor, dw = _sharded_case()
    want_v, want_i, _ = _RestatedEngine().outer_misfits(mis, nor, "l2norm", None, True, dw, ncomponents=ncomp)
    assert sorted(r for r, _, _ in got) == [0, 1]
    for _, v, i in got:
        assert np.array_equal(v, want_v, equal_nan=True) and np.array_equal(i, want_i)
    assert np.isnan(want_v[3]) and want_i[3] == 0
    # one process, no group: the same
    v, i = shard.sharded_bootstrap(_RestatedEngine(), mis, nor, ns, "l2norm", None, True, dw, ncomponents=ncomp)
    assert np.array_equal(v, want_v, equal_nan=True) and np.array_equal(i, want_i)


def test_restatement_ties_and_exclusions():
    ncomp = [2, 1, 3]
    mis, nor = K.make_case(9, ncomp, seed=4, failing=(0,))
    mis[5], nor[5] = mis[2], nor[2]                               # a duplicated source: the lower index answers
    mis[2] *= 0.01
    mis[5] *= 0.01
    mf, nf, sr = R.flatten(mis, nor, ncomp)
    dw = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [2.0, 0.0, 1.0]])
    bv, bi, g = R.outer_misfits(mf, nf, sr, 3, "l1norm", None, False, dw, which_draw=2)
    assert bi[0] == 2 and bi[2] == 2 and g[2] == g[5] and np.isnan(g[0])
    assert np.isnan(bv[1]) and bi[1] == 0
    bv, bi, _ = R.outer_misfits(mf[:1], nf[:1], sr, 3, "l2norm", None, True, dw)
    assert np.all(np.isnan(bv)) and np.all(bi == 0)


def test_outer_misfits_is_declared_exported_and_bound():
    from kiwi_amd import lib as klib
    names = ["kiwi_hip_outer_misfits", "kiwi_hip_outer_max_receivers", "kiwi_hip_get_outer_ms"]
    declared = klib.declared_symbols()
    text = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    bound = set(re.findall(r"name='(kiwi_hip_[a-z_0-9]+)'", text))
    klib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", klib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    L = klib.load()
    for name in names:
        assert name in declared, name
        assert name in bound, name
        assert re.search(r"\bT %s\b" % name, exported), name
        assert getattr(L, name).argtypes is not None
    assert L.kiwi_hip_outer_max_receivers() >= 512
    from kiwi_amd import Engine
    from kiwi_amd.gridsearch import MisfitGrid
    import inspect
    assert hasattr(Engine, "outer_misfits") and "engine" in inspect.signature(MisfitGrid.postprocess).parameters
