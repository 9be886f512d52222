"""numpy restatement of kiwi_hip_linear_fit_candidates (kiwi_amd/csrc/kiwi_linfit_candidates.hpp): the per-receiver sums
`by_receiver` [ngroup, nrec, NN] and their fold `normal` [ngroup, NN] in the layout of tests/linfit_restatement.py in, every
output of the call out, every fp64 operation in the documented order, so that the device can be asked for the same BITS.  The
loops over receivers and over the indices of a sum are scalar loops; the candidates of a group are carried side by side
(elementwise operations only: no `@`, no np.sum, nothing that could re-associate).  Not a test module:
tests/test_linfit_candidates.py and tests/test_linfit_candidates_gpu.py use it."""
import numpy as np

from tests import linfit_restatement as lr


def quad(q, x, K):
    """(x.b, x.G.x) of one row of sums q [NN] for the vectors x (a list of K arrays over the candidates): x.b and the rows of
    G x summed from zero in ascending index order, x.G.x = sum_i x_i (G x)_i -- linfit_solve_kernel's misfit sums"""
    NG = K * (K + 1) // 2
    xb = np.zeros_like(x[0])
    for i in range(K):
        xb = xb + x[i] * q[NG + i]
    xgx = np.zeros_like(x[0])
    for i in range(K):
        row = np.zeros_like(x[0])
        for j in range(K):
            row = row + q[lr.tri(K, min(i, j), max(i, j))] * x[j]
        xgx = xgx + x[i] * row
    return xb, xgx


def first_minimum(misfit):
    """(index, value) of the best entry: NaN passed over, then the smaller value, then the LOWEST index; (-1, NaN) if none"""
    bi, bv = -1, np.nan
    for i in range(len(misfit)):
        v = misfit[i]
        if v == v and (bi < 0 or v < bv):
            bi, bv = i, v
    return bi, bv


def evaluate(by_receiver, normal, weights, anarchy, candidates, outer_norm, free_scale=False):
    """dict(best_index [ng] int32, best_misfit [ng], status [ng] int32, misfit [ng, ncand], scale [ng, ncand] (ones without
    free_scale), receiver_misfit [ng, ncand, nrec] float32, receiver_norm [ng, nrec] float32, receiver_val [ng, ncand, nrec]: the
    clamped quadratic form in front of the root, fp64).  weights: [nrec] with zeros for disabled receivers, or None = ones"""
    nbr, nrm = np.asarray(by_receiver, np.float64), np.asarray(normal, np.float64)
    cand = np.atleast_2d(np.asarray(candidates, np.float64))
    ng, nrec, NN = nbr.shape
    ncand, K = cand.shape
    assert NN == lr.nn_of(K) and outer_norm in ("l1norm", "l2norm") and not (free_scale and outer_norm == "l1norm")
    w = np.ones(nrec) if weights is None else np.asarray(weights, np.float64)
    out = dict(best_index=np.zeros(ng, np.int32), best_misfit=np.zeros(ng), status=np.zeros(ng, np.int32),
               misfit=np.zeros((ng, ncand)), scale=np.ones((ng, ncand)), receiver_misfit=np.zeros((ng, ncand, nrec), np.float32),
               receiver_norm=np.zeros((ng, nrec), np.float32), receiver_val=np.zeros((ng, ncand, nrec)))
    with np.errstate(all="ignore"):
        for g in range(ng):
            x = [cand[:, i].copy() for i in range(K)]
            a = np.ones(ncand)
            mf = np.full(ncand, np.nan)
            status = 1
            if outer_norm == "l2norm":
                N = nrm[g]
                R = N[NN - 1]
                if free_scale:
                    a = np.full(ncand, np.nan)
                if R > 0.0:
                    status = 0
                    xb, xgx = quad(N, x, K)
                    ok = np.ones(ncand, bool)
                    if free_scale:
                        ok = xgx > 0.0
                        a = np.where(ok, xb / np.where(ok, xgx, 1.0), np.nan)
                        x = [a * x[i] for i in range(K)]
                        xb, xgx = quad(N, x, K)
                    val = (R - 2.0 * xb) + xgx
                    val = np.where(val > 0.0, val, 0.0)
                    mf = np.where(ok, np.sqrt(val / R), np.nan)
                elif free_scale:
                    x = [a * x[i] for i in range(K)]
            Ls, Ds, counted = np.zeros(ncand), np.zeros(ncand), False
            for r in range(nrec):
                wr = w[r]
                if wr == 0.0:
                    continue
                q = nbr[g, r]
                Rr = q[NN - 1]
                if not Rr > 0.0:
                    continue
                xb, xgx = quad(q, x, K)
                val = (Rr - 2.0 * xb) + xgx
                val = np.where(val > 0.0, val, 0.0)
                m, n = np.sqrt(val), np.sqrt(Rr)
                v = wr / n if anarchy else wr
                Ls = Ls + v * m
                Ds = Ds + v * n
                counted = True
                out["receiver_val"][g, :, r] = val
                out["receiver_misfit"][g, :, r] = np.where(a == a, m, np.nan).astype(np.float32)
                out["receiver_norm"][g, r] = np.float32(n)
            if outer_norm == "l1norm":
                status = 0 if counted else 1
                if counted:
                    mf = Ls / Ds
            out["misfit"][g], out["scale"][g], out["status"][g] = mf, a, status
            out["best_index"][g], out["best_misfit"][g] = first_minimum(mf)
    return out
