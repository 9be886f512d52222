"""numpy restatement of kiwi_hip_spectral_candidates_bootstrap (kiwi_amd/csrc/kiwi_spectral_candidates_bootstrap.hpp) as the
COMPOSITION that defines the call: kiwi_hip_spectral_candidates' slot_misfit [ng, ncand, nmis] and slot_norm [ng, nmis] (float32;
tests/spectral_candidates_restatement.py `evaluate` makes them from the spectra) are read as ng ncand sources of nmis slots, slot m
belonging to receiver slot_receiver[m], the norm row of group g repeated for each of its sources; tests/outer_restatement.py
`outer_misfits` finds the best source of every draw.  Nothing of either is rewritten here: the slot arrays go through the waveform
sibling's composition as a scan of ONE offset, which adds the index taken apart as g ncand + c and NaN, -1, -1 for a draw that
excludes everything (best_offset and group_offset are 0 where there is a best, else -1, as `Engine.spectral_candidates_bootstrap`
fills them).  Not a test module: tests/test_spectral_candidates_bootstrap.py and tests/test_spectral_candidates_bootstrap_gpu.py
use it."""
import numpy as np

from tests import waveform_candidates_bootstrap_restatement as wbr


def from_slots(slot_misfit, slot_norm, slot_receiver, nrec, status, draw_weights, outer_norm, receiver_weights=None, anarchy=False,
               outer=None):
    """the host route on the parent call's slot arrays.  `outer` as in tests/waveform_candidates_bootstrap_restatement.py.
    dict(best_value [nd], best_group, best_offset, best_cand [nd] int32, status [ng] int32, group_value [ng, nd], group_offset,
    group_cand [ng, nd] int32)"""
    m = np.asarray(slot_misfit, np.float32)
    assert m.ndim == 3
    return wbr.from_scan(m[:, None], slot_norm, slot_receiver, nrec, status, draw_weights, outer_norm, receiver_weights, anarchy, outer=outer)


def from_spectra(groups, slot_receiver, nrec, weights, anarchy, candidates, method, outer_norm, dt, draw_weights, syn_factor=1.0, cache=None):
    """the same from the parent call's `spectra` outputs (tests/spectral_candidates_restatement.py groups_from_scan): `evaluate`
    makes the slot arrays and the status, `from_slots` the rest.  weights: [nrec], 0 for a disabled receiver"""
    from tests import spectral_candidates_restatement as sr
    rs = sr.evaluate(groups, slot_receiver, weights, anarchy, candidates, method, outer_norm, dt, syn_factor=syn_factor, cache=cache)
    norm = np.array([[np.float32(sl["norm"]) for sl in g] for g in groups], np.float32).reshape(len(groups), -1)
    return from_slots(rs["slot_misfit"], norm, slot_receiver, nrec, rs["status"], draw_weights, outer_norm, weights, anarchy)
