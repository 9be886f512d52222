"""Shared pieces of the tests of kiwi_hip_linear_fit_candidates_time_scan: the parent's calls per offset on a context whose
references and tapers are moved (route B) put into the restatement's layout, the comparison under the two arithmetic contracts,
and -- run as a script -- the packing case in a process of its own (KIWI_HIP_CHUNK_MB is read when a context is made).  Not a test
module."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = (("l1norm", False), ("l2norm", False), ("l2norm", True))          # (outer norm, free_scale)
PACK_NCAND = 300
FIELDS = ("best_offset", "best_index", "best_misfit", "best_scale", "status", "cand_misfit", "cand_offset", "cand_scale", "misfit", "scale",
          "receiver_misfit", "receiver_norm")


def pack_candidates():
    return np.random.default_rng(10).uniform(-2.0, 2.0, (PACK_NCAND, 6))


def from_parents(scans):
    """CandidateScans of nk separate `linear_fit_candidates` calls (route B, offsets ascending) as the dict
    tests/linfit_candidates_timescan_restatement.py `evaluate` returns: the folds over the offsets are its scalar loops"""
    from tests import linfit_candidates_timescan_restatement as ctr
    st = lambda name: np.stack([getattr(s, name) for s in scans], 1)          # noqa: E731
    out = {name: st(name) for name in ("best_index", "best_misfit", "misfit", "receiver_misfit")}
    out["scale"] = st("scale") if scans[0].scale is not None else np.ones_like(out["misfit"])
    for s in scans[1:]:                                     # R_r does not depend on the offset
        assert np.array_equal(s.status, scans[0].status) and np.array_equal(s.receiver_norm, scans[0].receiver_norm)
    out["status"], out["receiver_norm"] = scans[0].status, scans[0].receiver_norm
    ng, nk, ncand = out["misfit"].shape
    out["best_offset"] = np.array([ctr.best_offset(out["best_index"][g], out["best_misfit"][g]) for g in range(ng)], np.int32)
    out["best_scale"] = np.full((ng, nk), np.nan)
    for g in range(ng):
        for j in range(nk):
            if out["best_index"][g, j] >= 0:
                out["best_scale"][g, j] = out["scale"][g, j, out["best_index"][g, j]]
    m = [ctr.marginal(out["misfit"][g], out["scale"][g]) for g in range(ng)]
    out["cand_misfit"], out["cand_offset"], out["cand_scale"] = (np.stack([x[i] for x in m]) for i in range(3))
    return out


def slack_of(by_receiver, weights, x, scale=None):
    """tests/test_linfit_candidates_gpu.py assert_same_scan's slack per (group, offset, candidate): a relative perturbation
    SYN_RTOL of the kept traces' maximum, 64 SYN_RTOL of their norm, moves a candidate's misfit |sum_i x_i s_i - d| / |d| by at
    most 64 SYN_RTOL sum_i |x_i| |s_i| / |d|, the largest such figure over the receivers that count.  by_receiver
    [ng, nk, nrec, NN]; x [ncand, K]; scale [ng, nk, ncand] (free_scale: x is a direction) or None"""
    from tests import linfit_restatement as lr
    from tests.common import SYN_RTOL
    nbr = np.asarray(by_receiver, np.float64)
    K = x.shape[1]
    R = nbr[..., -1]                                                            # [ng, nk, nrec]
    counts = (R > 0.0) & (np.ones(R.shape[-1]) if weights is None else np.asarray(weights) != 0.0).astype(bool)
    diag = np.stack([nbr[..., lr.tri(K, i, i)] for i in range(K)], -1)          # [ng, nk, nrec, K]
    with np.errstate(all="ignore"):
        ratio = np.where(counts[..., None], np.sqrt(diag / R[..., None]), 0.0)
    per = (np.abs(x)[None, None, None, :, :] * ratio[:, :, :, None, :]).sum(-1).max(2)      # [ng, nk, ncand]
    if scale is not None:
        per = per * np.where(np.isfinite(scale), np.abs(scale), 0.0)
    return 64 * SYN_RTOL * per


def assert_scan(got, want, slack, what):
    """a CandidateTimeScan against the restatement's dict (or from_parents'): every array the call made.  exact contract: the same
    bits.  fused: the sums of the two sides may come from synthetics of different accumulate-kernel instantiations; the statuses
    agree and the misfits within `slack` [ng, nk, ncand] (slack_of)"""
    from tests import common
    assert np.array_equal(got.status, want["status"]), (what, "status")
    if common.arith() == "exact":
        for name in FIELDS:
            a, b = getattr(got, name), want[name]
            if a is None:
                continue
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
            same = np.array_equal(a, b, equal_nan=a.dtype != np.int32)
            if not same:
                bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
                print(what, name, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
            assert same, (what, name)
        return
    with np.errstate(invalid="ignore"):
        close = lambda a, b, s: np.all((np.abs(a - b) <= s) | ((a != a) & (b != b)))      # noqa: E731
        if got.misfit is not None:
            assert close(got.misfit, want["misfit"], slack), (what, "misfit")
        assert close(got.best_misfit, want["best_misfit"], slack.max(2)), (what, "best_misfit")
        if got.cand_misfit is not None:
            assert close(got.cand_misfit, want["cand_misfit"], slack.max(1)), (what, "cand_misfit")


def route_b_sums(p, sc, ks, ngroup, K, weights, anarchy):
    """`linear_fit` with its sums per offset on the moved context: (by_receiver [ng, nk, nrec, NN], normal [ng, nk, NN], the fits)"""
    from tests import linfit_timescan_cases as lc
    fits = lc.route_b(p, sc, ks, lambda: p.linear_fit(0, ngroup, K, receiver_weights=weights, anarchy=anarchy, normal=True, by_receiver=True))
    return np.stack([f.by_receiver for f in fits], 1), np.stack([f.normal for f in fits], 1), fits


def main(out):
    """the scans of linfit_timescan_cases.chunk_rows() as this process's environment cuts them into chunks"""
    from tests import linfit_timescan_cases as lc
    sc, p = lc.standard()
    try:
        p.set_source_params("moment_tensor", lc.chunk_rows())
        z = {}
        for norm, free in MODES:
            p.kernel_ms()
            scan = p.linear_fit_candidates_time_scan(0, lc.CHUNK_GROUPS, lc.CHUNK_K, pack_candidates(), *lc.CHUNK_SCAN, outer_norm=norm,
                                                     anarchy=True, free_scale=free, misfit=True, receiver_misfit=True)
            key = "%s_%d_" % (norm, free)
            z.update({key + name: getattr(scan, name) for name in scan._fields if getattr(scan, name) is not None})
            z[key + "launches"] = np.array(p.kernel_ms()[1])
        np.savez(out, **z)
    finally:
        p.close()


if __name__ == "__main__":
    main(sys.argv[1])
