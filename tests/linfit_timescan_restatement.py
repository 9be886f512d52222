"""numpy restatement of kiwi_hip_linear_fit_time_scan (kiwi_amd/csrc/kiwi_linfit_timescan.hpp): a thin layer over
tests/linfit_restatement.py -- shift, taper, `fit`, first minimum.  Not a test module.

Rows: per misfit slot `raw[slot]` float32 [ngroup, K, wlen + 2 S] -- the folded, moment-scaled, UNTAPERED synthetic of every basis
source over the slot's window made S samples wider on either side (index e is window sample e - S) --, `taper[slot]` float32
[wlen] the taper weights over the window and `ref[slot]` float32 [wlen] the tapered reference.  `receivers` as in
linfit_restatement."""
import numpy as np

from tests import linfit_restatement as lr


def shifted_traces(raw, taper, S, k):
    """what the comparator holds of every basis source moved k samples later, before the synthetics factor:
    fp32(row[t - k] x taper[t]) over the window"""
    assert abs(k) <= S
    out = []
    for r, w in zip(raw, taper):
        w = np.asarray(w, np.float32)
        out.append(np.asarray(r, np.float32)[:, :, S - k:S - k + len(w)] * w)
    return out


def first_minimum(misfit, status):
    """per group the index of the smallest misfit among the offsets with status 0, the lowest among equal values; -1 if none"""
    best = np.full(len(misfit), -1, np.int32)
    for g in range(len(misfit)):
        b, v = -1, 0.0
        for j in range(misfit.shape[1]):
            if status[g, j] != 0:
                continue
            if b < 0 or misfit[g, j] < v:
                b, v = j, misfit[g, j]
        best[g] = b
    return best


def fit(raw, taper, ref, receivers, dt, S, k0, kstep, nk, weights=None, anarchy=False, syn_factor=1.0):
    """the whole call: dict(coef [ngroup, nk, K], misfit, status, pivot_min [ngroup, nk], normal [ngroup, nk, NN], best [ngroup])"""
    per = [lr.fit(shifted_traces(raw, taper, S, k0 + j * kstep), ref, receivers, dt, weights, anarchy, syn_factor) for j in range(nk)]
    out = {name: np.stack([p[name] for p in per], 1) for name in ("coef", "misfit", "status", "pivot_min", "normal")}
    out["best"] = first_minimum(out["misfit"], out["status"])
    return out
