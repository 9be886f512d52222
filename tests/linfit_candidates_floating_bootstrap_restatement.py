"""numpy restatement of kiwi_hip_linear_fit_candidates_floating_bootstrap (kiwi_amd/csrc/kiwi_linfit_candidates_floating_bootstrap.hpp)
as the COMPOSITION that defines the call: tests/linfit_candidates_floating_restatement.py `evaluate` makes receiver_misfit
[ng, ncand, nrec] and receiver_norm [ng, nrec] as float32 and cand_shift [ng, ncand, nrec]; tests/outer_restatement.py
`outer_misfits` reads the first two as ng ncand sources of one slot per receiver and finds the best source of every draw
(through tests/linfit_candidates_bootstrap_restatement.py `from_scan` with one offset); the winner's row of cand_shift is the
draw's shifts.  Nothing of either parent is rewritten here.  Not a test module: tests/test_linfit_candidates_floating_bootstrap.py
and tests/test_linfit_candidates_floating_bootstrap_gpu.py use it."""
import numpy as np

from tests import linfit_candidates_bootstrap_restatement as br
from tests import linfit_candidates_floating_restatement as fr


def winners_shifts(cand_shift, group, cand):
    """rows of cand_shift [ng, ncand, nrec] at (group, cand) [...] as int32 [..., nrec]; zeros where cand < 0"""
    cs = np.asarray(cand_shift)
    has = np.asarray(cand) >= 0
    rows = cs[np.where(has, group, 0), np.where(has, cand, 0)].astype(np.int32)
    return np.where(has[..., None], rows, np.int32(0)).astype(np.int32)


def from_scan(receiver_misfit, receiver_norm, cand_shift, status, draw_weights, outer_norm, receiver_weights=None, anarchy=False, outer=None):
    """the host route on the parent call's arrays (receiver_misfit, cand_shift [ng, ncand, nrec], receiver_norm [ng, nrec]).
    `outer` as in tests/linfit_candidates_bootstrap_restatement.py from_scan.  dict(best_value [nd], best_group, best_cand [nd]
    int32, best_shift [nd, nrec] int32, status [ng] int32, group_value [ng, nd], group_cand [ng, nd] int32, group_shift
    [ng, nd, nrec] int32)"""
    m = np.asarray(receiver_misfit, np.float32)
    ng = m.shape[0]
    b = br.from_scan(m[:, None], receiver_norm, status, draw_weights, outer_norm, receiver_weights, anarchy, outer=outer)
    out = {name: b[name] for name in ("best_value", "best_group", "best_cand", "status", "group_value", "group_cand")}
    out["best_shift"] = winners_shifts(cand_shift, out["best_group"], out["best_cand"])
    out["group_shift"] = winners_shifts(cand_shift, np.arange(ng)[:, None], out["group_cand"])
    return out


def evaluate(by_receiver, shift_b, shift_R, fl_lo, weights, anarchy, candidates, outer_norm, draw_weights):
    """the sums as tests/linfit_candidates_floating_restatement.py `evaluate` takes them; weights [nrec] with zeros for disabled
    receivers, or None.  What the call answers (from_scan's dict)"""
    rs = fr.evaluate(by_receiver, shift_b, shift_R, fl_lo, weights, anarchy, candidates, outer_norm)
    return from_scan(rs["receiver_misfit"], rs["receiver_norm"], rs["cand_shift"], rs["status"], draw_weights, outer_norm, weights, anarchy)
