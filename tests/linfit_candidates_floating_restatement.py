"""numpy restatement of kiwi_hip_linear_fit_candidates_floating (kiwi_amd/csrc/kiwi_linfit_candidates_floating.hpp): the
per-receiver sums in -- `by_receiver` [ngroup, nrec, NN] in the layout of tests/linfit_restatement.py (only G_r of it is read) and,
per shift of every receiver's range, b_r[q] and R_r[q] --, every output of the call out, every fp64 operation in the documented
order, so that the device can be asked for the same BITS.  The loops over receivers, shifts and the indices of a sum are scalar
loops; the candidates of a group are carried side by side (elementwise operations only).  Not a test module:
tests/test_linfit_candidates_floating.py and tests/test_linfit_candidates_floating_gpu.py use it."""
import numpy as np

from tests import linfit_candidates_restatement as cr
from tests import linfit_restatement as lr


def receiver_norm(R):
    """n_r = (sum_q sqrt(R_r[q])) / fl_ns, q ascending"""
    s = 0.0
    for q in range(len(R)):
        s = s + np.sqrt(R[q])
    return s / float(len(R))


def evaluate(by_receiver, shift_b, shift_R, fl_lo, weights, anarchy, candidates, outer_norm):
    """shift_b[r]: [ngroup, ns_r, K]; shift_R[r]: [ngroup, ns_r]; fl_lo[r]: the first shift of receiver r in samples.
    dict(best_index [ng] int32, best_misfit [ng], status [ng] int32, best_shift [ng, nrec] int32, misfit [ng, ncand], cand_shift
    [ng, ncand, nrec] int16, receiver_misfit [ng, ncand, nrec] float32, receiver_norm [ng, nrec] float32, receiver_val
    [ng, ncand, nrec]: the smallest clamped quadratic form, fp64).  weights: [nrec] with zeros for disabled receivers, or None"""
    nbr = np.asarray(by_receiver, np.float64)
    cand = np.atleast_2d(np.asarray(candidates, np.float64))
    ng, nrec, NN = nbr.shape
    ncand, K = cand.shape
    assert NN == lr.nn_of(K) and outer_norm in ("l1norm", "l2norm")
    w = np.ones(nrec) if weights is None else np.asarray(weights, np.float64)
    out = dict(best_index=np.zeros(ng, np.int32), best_misfit=np.zeros(ng), status=np.zeros(ng, np.int32),
               best_shift=np.zeros((ng, nrec), np.int32), misfit=np.zeros((ng, ncand)), cand_shift=np.zeros((ng, ncand, nrec), np.int16),
               receiver_misfit=np.zeros((ng, ncand, nrec), np.float32), receiver_norm=np.zeros((ng, nrec), np.float32),
               receiver_val=np.zeros((ng, ncand, nrec)))
    with np.errstate(all="ignore"):
        for g in range(ng):
            x = [cand[:, i].copy() for i in range(K)]
            Ls, Ds, counted = np.zeros(ncand), np.zeros(ncand), False
            for r in range(nrec):
                wr = w[r]
                if wr == 0.0:
                    continue
                R = np.asarray(shift_R[r], np.float64)[g]
                b = np.asarray(shift_b[r], np.float64)[g]
                n = receiver_norm(R)
                if not n > 0.0:
                    continue
                _, xgx = cr.quad(nbr[g, r], x, K)
                minv, arg = np.zeros(ncand), np.full(ncand, -1)
                for q in range(len(R)):
                    xb = np.zeros(ncand)
                    for i in range(K):
                        xb = xb + x[i] * b[q, i]
                    val = (R[q] - 2.0 * xb) + xgx
                    val = np.where(val > 0.0, val, 0.0)
                    take = (arg < 0) | (val < minv)
                    minv = np.where(take, val, minv)
                    arg = np.where(take, q, arg)
                m = np.sqrt(minv)
                v = wr / n if anarchy else wr
                if outer_norm == "l1norm":
                    Ls = Ls + v * m
                    Ds = Ds + v * n
                else:
                    v2 = v * v
                    Ls = Ls + v2 * minv
                    Ds = Ds + v2 * (n * n)
                counted = True
                out["receiver_val"][g, :, r] = minv
                out["receiver_misfit"][g, :, r] = m.astype(np.float32)
                out["receiver_norm"][g, r] = np.float32(n)
                out["cand_shift"][g, :, r] = (fl_lo[r] + arg).astype(np.int16)
            mf = np.full(ncand, np.nan)
            if counted:
                mf = Ls / Ds if outer_norm == "l1norm" else np.sqrt(Ls / Ds)
            out["misfit"][g], out["status"][g] = mf, 0 if counted else 1
            bi, bv = cr.first_minimum(mf)
            out["best_index"][g], out["best_misfit"][g] = bi, bv
            if bi >= 0:
                out["best_shift"][g] = out["cand_shift"][g, bi]
    return out
