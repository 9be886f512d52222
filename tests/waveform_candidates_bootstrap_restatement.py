"""numpy restatement of kiwi_hip_waveform_candidates_bootstrap (kiwi_amd/csrc/kiwi_waveform_candidates_bootstrap.hpp) as the
COMPOSITION that defines the call: kiwi_hip_waveform_candidates_time_scan's slot_misfit [ng, nk, ncand, nmis] and slot_norm
[ng, nmis] (float32; tests/waveform_candidates_timescan_restatement.py makes them from the rows) are read as ng nk ncand sources of
nmis slots, slot m belonging to receiver slot_receiver[m], the norm row of group g repeated for each of its sources;
tests/outer_restatement.py `outer_misfits` finds the best source of every draw.  Nothing of either is rewritten here; what is added
is the index taken apart and the -1 rule.  Not a test module: tests/test_waveform_candidates_bootstrap.py and
tests/test_waveform_candidates_bootstrap_gpu.py use it."""
import numpy as np

from tests import outer_restatement as orr
from tests.linfit_candidates_bootstrap_restatement import take_apart


def sources(slot_misfit, slot_norm):
    """(misfit, norm [nsrc, nmis] float32) of slot_misfit [ng, nk, ncand, nmis] and slot_norm [ng, nmis]: the norm row of group g
    repeated for each of its nk ncand sources"""
    m = np.asarray(slot_misfit, np.float32)
    ng, nk, ncand, nmis = m.shape
    n = np.broadcast_to(np.asarray(slot_norm, np.float32)[:, None, None, :], m.shape)
    return m.reshape(ng * nk * ncand, nmis), np.ascontiguousarray(n).reshape(ng * nk * ncand, nmis)


def from_scan(slot_misfit, slot_norm, slot_receiver, nrec, status, draw_weights, outer_norm, receiver_weights=None, anarchy=False,
              outer=None):
    """the host route on a scan's slot arrays.  `outer(misfit, norm, slot_receiver, nrec, outer_norm, receiver_weights, anarchy,
    draw_weights)` -> (best_value, best_index, ...): tests/outer_restatement.py's by default.  dict(best_value [nd], best_group,
    best_offset, best_cand [nd] int32, status [ng] int32, group_value [ng, nd], group_offset, group_cand [ng, nd] int32)"""
    outer = orr.outer_misfits if outer is None else outer
    m = np.asarray(slot_misfit, np.float32)
    ng, nk, ncand, nmis = m.shape
    slots = np.asarray(slot_receiver, np.int32)
    assert slots.shape == (nmis,)
    dw = np.asarray(draw_weights, np.float64)
    mis, nor = sources(m, slot_norm)
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
