"""Shared pieces of tests/test_linfit_candidates_floating_gpu.py: shift ranges on a product engine, the per-shift sums by the brute
route (the references moved by every shift of the range, `linear_fit(..., by_receiver=True)` each time), and the comparison of a
`CandidateFloatingScan` with the restatement.  Not a test module."""
import numpy as np

from tests import common
from tests import linfit_candidates_restatement as cr
from tests import linfit_restatement as lr
from tests.common import SYN_RTOL

# per receiver (lo, hi) in samples: lengths 1, 2 (negative only), J = 4 (positive only), J + 1, 33 (longer than an LDS stage of 32
# shifts) and 3
RANGES_A = [(0, 0), (-2, -1), (1, 4), (-2, 2), (-16, 16), (-1, 1)]
RANGES_B = RANGES_A[1:] + RANGES_A[:1]


def set_ranges(p, dt, ranges):
    for ir, (lo, hi) in enumerate(ranges):
        p.set_floating_shiftrange(ir + 1, lo * dt, hi * dt)


def brute_sums(p, dt, ranges, ngroup, K, isrc0=0):
    """(by_receiver [ngroup, nrec, NN] of the unshifted references, shift_b[r] [ngroup, ns_r, K], shift_R[r] [ngroup, ns_r]) of the
    uploaded groups, under l2norm: pass j moves every receiver's references by the j-th shift of its range (the last one again
    where the range is shorter) with `shift_ref_seismogram`, fits, and moves them back.  Leaves the method at l2norm"""
    NG, NN = K * (K + 1) // 2, lr.nn_of(K)
    p.set_misfit_method("l2norm")
    nbr = p.linear_fit(isrc0, ngroup, K, by_receiver=True).by_receiver
    ns = [hi - lo + 1 for lo, hi in ranges]
    shift_b = [np.zeros((ngroup, n, K)) for n in ns]
    shift_R = [np.zeros((ngroup, n)) for n in ns]
    for j in range(max(ns)):
        sh = [ranges[r][0] + min(j, ns[r] - 1) for r in range(len(ranges))]
        for r, s in enumerate(sh):
            p.shift_ref_seismogram(r + 1, s * dt)
        q = p.linear_fit(isrc0, ngroup, K, by_receiver=True).by_receiver
        for r, s in enumerate(sh):
            p.shift_ref_seismogram(r + 1, -s * dt)
            if j < ns[r]:
                shift_b[r][:, j], shift_R[r][:, j] = q[:, r, NG:NG + K], q[:, r, NN - 1]
    return nbr, shift_b, shift_R


def slack_of(nbr, rs, cand):
    """[ngroup, ncand]: what a misfit may move by under the fused contract when the same groups go through another batch shape
    (assert_same_scan of tests/test_linfit_candidates_gpu.py): the kept traces agree within 64 SYN_RTOL of their norm, so
    |sum_i x_i s_i - a_q| moves by at most 64 SYN_RTOL sum_i |x_i| |s_i| at EVERY shift q, and so does its minimum over q; on the
    scale of n_r, the largest such figure over the receivers that count"""
    ng, nrec, NN = nbr.shape
    K = cand.shape[1]
    diag = np.stack([nbr[:, :, lr.tri(K, i, i)] for i in range(K)], 2)                     # [g, r, i]
    n = rs["receiver_norm"].astype(np.float64)
    ratio = np.where(n[:, :, None] > 0, np.sqrt(diag) / np.where(n[:, :, None] > 0, n[:, :, None], 1.0), 0.0)
    return 64 * SYN_RTOL * np.max(np.abs(cand)[None, None, :, :] * ratio[:, :, None, :], axis=1).sum(2)


def assert_floating_bits(scan, rs, ncand, what, slack=None):
    """every output of the call against the restatement's first ncand candidates.  exact contract: the same bits.  fused, where a
    slack is given (the two sides went through different batch shapes): misfits within it"""
    best = [cr.first_minimum(row[:ncand]) for row in rs["misfit"]]
    bi = np.array([b[0] for b in best], np.int32)
    if slack is not None and common.arith() != "exact":
        assert np.array_equal(scan.status, rs["status"]), what
        assert np.all(np.abs(scan.misfit - rs["misfit"][:, :ncand]) <= slack[:, :ncand]), what
        assert np.all(np.abs(scan.best_misfit - np.array([b[1] for b in best])) <= slack[:, :ncand].max(1)), what
        return
    bs = np.stack([rs["cand_shift"][g, max(bi[g], 0)].astype(np.int32) * (1 if bi[g] >= 0 else 0) for g in range(len(bi))])
    pairs = [("misfit", scan.misfit, rs["misfit"][:, :ncand]), ("cand_shift", scan.cand_shift, rs["cand_shift"][:, :ncand]),
             ("receiver_misfit", scan.receiver_misfit, rs["receiver_misfit"][:, :ncand]), ("receiver_norm", scan.receiver_norm, rs["receiver_norm"]),
             ("status", scan.status, rs["status"]), ("best_index", scan.best_index, bi),
             ("best_misfit", scan.best_misfit, np.array([b[1] for b in best])), ("best_shift", scan.best_shift, bs)]
    for name, a, b in pairs:
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        same = np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
        assert same, (what, name)
