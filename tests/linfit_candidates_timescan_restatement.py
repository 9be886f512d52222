"""numpy restatement of kiwi_hip_linear_fit_candidates_time_scan (kiwi_amd/csrc/kiwi_linfit_candidates_timescan.hpp): per offset
tests/linfit_candidates_restatement.py `evaluate` on the sums of that offset -- the device evaluates the same expressions on the
same rows --, then the folds over the offsets as scalar loops in the documented order.  Not a test module:
tests/test_linfit_candidates_timescan.py and tests/test_linfit_candidates_timescan_gpu.py use it."""
import numpy as np

from tests import linfit_candidates_restatement as cr


def best_offset(best_index, best_misfit):
    """the j of the smallest best_misfit[j] among the j with best_index[j] >= 0, the lowest j among equal values; -1 if none"""
    oj, ov = -1, 0.0
    for j in range(len(best_index)):
        if best_index[j] >= 0 and (oj < 0 or best_misfit[j] < ov):
            oj, ov = j, best_misfit[j]
    return oj


def marginal(misfit, scale):
    """(cand_misfit [ncand], cand_offset [ncand] int32, cand_scale [ncand]) of misfit, scale [nk, ncand]: j ascending, NaN passed
    over, the smaller value, the first j among equal values; NaN, -1, NaN where every offset is NaN"""
    nk, ncand = misfit.shape
    cm, co, cs = np.full(ncand, np.nan), np.full(ncand, -1, np.int32), np.full(ncand, np.nan)
    for c in range(ncand):
        for j in range(nk):
            v = misfit[j, c]
            if v == v and (co[c] < 0 or v < cm[c]):
                cm[c], co[c], cs[c] = v, j, scale[j, c]
    return cm, co, cs


def evaluate(by_receiver, normal, weights, anarchy, candidates, outer_norm, free_scale=False):
    """by_receiver [ng, nk, nrec, NN] and normal [ng, nk, NN]: the sums of every (group, offset).  dict(best_offset [ng] int32,
    best_index [ng, nk] int32, best_misfit [ng, nk], best_scale [ng, nk] (NaN where there is no winner; ones without free_scale),
    status [ng] int32, cand_misfit, cand_scale [ng, ncand], cand_offset [ng, ncand] int32, misfit, scale [ng, nk, ncand],
    receiver_misfit [ng, nk, ncand, nrec] float32, receiver_norm [ng, nrec] float32)"""
    nbr, nrm = np.asarray(by_receiver, np.float64), np.asarray(normal, np.float64)
    ng, nk = nbr.shape[:2]
    per = [cr.evaluate(nbr[:, j], nrm[:, j], weights, anarchy, candidates, outer_norm, free_scale) for j in range(nk)]
    out = {name: np.stack([p[name] for p in per], 1) for name in ("best_index", "best_misfit", "misfit", "scale", "receiver_misfit")}
    for j in range(1, nk):                                  # R_r does not depend on the offset
        assert np.array_equal(per[j]["status"], per[0]["status"]) and np.array_equal(per[j]["receiver_norm"], per[0]["receiver_norm"])
    out["status"], out["receiver_norm"] = per[0]["status"], per[0]["receiver_norm"]
    ncand = out["misfit"].shape[2]
    out["best_offset"] = np.zeros(ng, np.int32)
    out["best_scale"] = np.full((ng, nk), np.nan)
    out["cand_misfit"], out["cand_scale"] = np.zeros((ng, ncand)), np.zeros((ng, ncand))
    out["cand_offset"] = np.zeros((ng, ncand), np.int32)
    for g in range(ng):
        out["best_offset"][g] = best_offset(out["best_index"][g], out["best_misfit"][g])
        for j in range(nk):
            if out["best_index"][g, j] >= 0:
                out["best_scale"][g, j] = out["scale"][g, j, out["best_index"][g, j]]
        out["cand_misfit"][g], out["cand_offset"][g], out["cand_scale"][g] = marginal(out["misfit"][g], out["scale"][g])
    return out
