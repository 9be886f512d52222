"""numpy restatement of kiwi_hip_linear_fit_candidates_bootstrap (kiwi_amd/csrc/kiwi_linfit_candidates_bootstrap.hpp) as the
COMPOSITION that defines the call: tests/linfit_candidates_timescan_restatement.py `evaluate` (free_scale off) makes receiver_misfit
[ng, nk, ncand, nrec] and receiver_norm [ng, nrec] as float32, tests/outer_restatement.py `outer_misfits` reads them as
ng nk ncand sources of one slot per receiver and finds the best source of every draw; nothing of either is rewritten here.  Not a
test module: tests/test_linfit_candidates_bootstrap.py and tests/test_linfit_candidates_bootstrap_gpu.py use it."""
import numpy as np

from tests import linfit_candidates_timescan_restatement as ctr
from tests import outer_restatement as orr


def take_apart(best_value, best_index, nk, ncand):
    """kiwi_hip_outer_misfits' (best_value, best_index) over ng nk ncand sources as (value, group, offset, candidate): the index
    (g nk + j) ncand + c taken apart; NaN, -1, -1, -1 for a draw with every source excluded (the host route writes index 0)"""
    v = np.asarray(best_value, np.float64)
    i = np.asarray(best_index, np.int64)
    has = v == v
    none = np.int32(-1)
    return (v, np.where(has, i // (nk * ncand), none).astype(np.int32), np.where(has, i // ncand % nk, none).astype(np.int32),
            np.where(has, i % ncand, none).astype(np.int32))


def sources(receiver_misfit, receiver_norm):
    """(misfit, norm [nsrc, nrec] float32) of receiver_misfit [ng, nk, ncand, nrec] and receiver_norm [ng, nrec]: the norm row of
    group g repeated for each of its nk ncand sources"""
    m = np.asarray(receiver_misfit, np.float32)
    ng, nk, ncand, nrec = m.shape
    n = np.broadcast_to(np.asarray(receiver_norm, np.float32)[:, None, None, :], m.shape)
    return m.reshape(ng * nk * ncand, nrec), np.ascontiguousarray(n).reshape(ng * nk * ncand, nrec)


def from_scan(receiver_misfit, receiver_norm, status, draw_weights, outer_norm, receiver_weights=None, anarchy=False, outer=None):
    """the host route on a scan's arrays.  `outer(misfit, norm, slot_receiver, nrec, outer_norm, receiver_weights, anarchy,
    draw_weights)` -> (best_value, best_index, ...): tests/outer_restatement.py's by default.  dict(best_value [nd], best_group,
    best_offset, best_cand [nd] int32, status [ng] int32, group_value [ng, nd], group_offset, group_cand [ng, nd] int32)"""
    outer = orr.outer_misfits if outer is None else outer
    m = np.asarray(receiver_misfit, np.float32)
    ng, nk, ncand, nrec = m.shape
    slots = np.arange(nrec, dtype=np.int32)
    dw = np.asarray(draw_weights, np.float64)
    mis, nor = sources(m, receiver_norm)
    bv, bi = outer(mis, nor, slots, nrec, outer_norm, receiver_weights, anarchy, dw)[:2]
    out = dict(status=np.asarray(status, np.int32))
    out["best_value"], out["best_group"], out["best_offset"], out["best_cand"] = take_apart(bv, bi, nk, ncand)
    out["group_value"] = np.zeros((ng, len(dw)))
    out["group_offset"], out["group_cand"] = np.zeros((ng, len(dw)), np.int32), np.zeros((ng, len(dw)), np.int32)
    per = nk * ncand
    for g in range(ng):
        bv, bi = outer(mis[g * per:(g + 1) * per], nor[g * per:(g + 1) * per], slots, nrec, outer_norm, receiver_weights, anarchy, dw)[:2]
        out["group_value"][g], _, out["group_offset"][g], out["group_cand"][g] = take_apart(bv, bi, nk, ncand)
    return out


def evaluate(by_receiver, normal, weights, anarchy, candidates, outer_norm, draw_weights):
    """by_receiver [ng, nk, nrec, NN] and normal [ng, nk, NN]: the sums of every (group, offset); weights [nrec] with zeros for
    disabled receivers, or None.  What the call answers (from_scan's dict)"""
    rs = ctr.evaluate(by_receiver, normal, weights, anarchy, candidates, outer_norm, False)
    return from_scan(rs["receiver_misfit"], rs["receiver_norm"], rs["status"], draw_weights, outer_norm, weights, anarchy)
