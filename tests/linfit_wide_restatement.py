"""numpy restatement of kiwi_hip_linear_fit_wide (kiwi_amd/csrc/kiwi_linfit_wide.hpp) on top of tests/linfit_restatement.py:
the per-receiver sums are `linfit_restatement.gram_by_receiver`'s for any K (every element keeps linfit_gram_kernel's order);
here the fold, the penalty, the Cholesky over a passive set and the non-negative active-set loop, every fp64 operation in the
documented order, so that the device can be asked for the same BITS.  Not a test module: tests/test_linfit_wide.py and
tests/test_linfit_wide_gpu.py use it."""
import numpy as np

from tests import linfit_restatement as lr

MAX_BASIS = 64
EPS = 2.0 ** -52


def fold(nbr, weights=None, anarchy=False):
    """[ngroup, NN]: receivers ascending, N = N + (w w) N_r with the skip rules of linfit_solve_kernel"""
    ng, nrec, NN = nbr.shape
    w = np.ones(nrec) if weights is None else np.asarray(weights, np.float64)
    N = np.zeros((ng, NN))
    with np.errstate(all="ignore"):
        for r in range(nrec):
            if w[r] == 0.0:
                continue
            wr = np.full(ng, w[r])
            if anarchy:
                Rr = nbr[:, r, NN - 1]
                wr = np.where(Rr > 0.0, wr / np.sqrt(np.where(Rr > 0.0, Rr, 1.0)), 0.0)
            w2 = wr * wr
            N = np.where((wr != 0.0)[:, None], N + w2[:, None] * nbr[:, r, :], N)
    return N


def cholesky_subset(A, c, idx, tol):
    """A_PP z = c_P over the indices `idx` (ascending) of the scaled matrix A (symmetric, unit diagonal) by the Cholesky of
    linfit_restatement.solve: (ok, z [len(idx)], smallest pivot up to and including the one that broke down)"""
    n = len(idx)
    Ap = A[np.ix_(idx, idx)]
    L = np.zeros((n, n))
    pmin = 1.0
    for j in range(n):
        v = Ap[j:, j].copy()                                  # (v[0] starts from the unit diagonal: d)
        for k in range(j):
            v = v - L[j:, k] * L[j, k]
        d = v[0]
        if d < pmin:
            pmin = d
        if not d > tol:
            return False, None, pmin
        ljj = np.sqrt(d)
        L[j, j] = ljj
        L[j + 1:, j] = v[1:] / ljj
    v = np.array(c[idx], np.float64)
    y = np.zeros(n)
    for j in range(n):
        y[j] = v[j] / L[j, j]
        v[j + 1:] = v[j + 1:] - L[j + 1:, j] * y[j]
    z = np.zeros(n)
    for i in range(n - 1, -1, -1):
        t = float(y[i])
        p = L[i + 1:, i] * z[i + 1:]
        for k in range(len(p)):
            t = t - float(p[k])
        z[i] = t / L[i, i]
    return True, z, pmin


def gradient(A, c, x, P, i):
    """w_i = c_i - sum_{j in P ascending} A_ij x_j of the scaled problem, each product and difference rounded on its own"""
    w = c[i]
    for j in P:
        w = w - A[i, j] * x[j]
    return w


def nonneg_threshold(c, K):
    """10 K 2^-52 max_i |c_i|: a gradient component not above it does not enter the passive set"""
    return (10.0 * K * EPS) * np.max(np.abs(c))


def solve_one(N, K, nonneg=False, penalty=None, penalty_relative=False):
    """one group's folded sums N [NN] -> dict(coef [K], misfit, status, pivot_min, npositive, nsolves; barred: the indices
    the active-set loop barred and passive: its final passive set, which the device does not report; scaled: (A, c, x) of
    the scaled problem, for `gradient`)"""
    NG = K * (K + 1) // 2
    nan = np.nan
    out = dict(coef=np.full(K, nan), misfit=nan, status=1, pivot_min=0.0, npositive=0, nsolves=0, barred=[], passive=[])
    R = N[NG + K]
    G = np.zeros((K, K))                                      # the PENALISED sums, symmetric
    for i in range(K):
        for j in range(i, K):
            G[i, j] = G[j, i] = N[lr.tri(K, i, j)]
    G0 = G.copy()
    with np.errstate(all="ignore"):
        if penalty is not None:
            lam = 1.0
            if penalty_relative:
                lam = 0.0
                for i in range(K):
                    lam = lam + G0[i, i]
                lam = lam / float(K)
            for i in range(K):
                for j in range(i, K):
                    G[i, j] = G[j, i] = G0[i, j] + lam * penalty[lr.tri(K, i, j)]
        D = np.diag(G).copy()
        if not np.all(D > 0.0):
            return out
        s = 1.0 / np.sqrt(D)
        A = np.ones((K, K))
        for i in range(K):
            for j in range(i):
                A[i, j] = A[j, i] = (G[j, i] * s[i]) * s[j]   # row i > column j, as scaled_cholesky forms it
        c = N[NG:NG + K] * s
        tol = K * EPS
        x = np.zeros(K)
        if nonneg and not (np.all(np.isfinite(c)) and np.all(np.isfinite(A))):
            return out                                        # (the lanes of the device loop would disagree on a NaN gradient)
        inP = np.zeros(K, bool)
        status, nsolves, pmin = 0, 0, 1.0
        barred = np.zeros(K, bool)
        if not nonneg:
            nsolves = 1
            ok, z, pmin = cholesky_subset(A, c, np.arange(K), tol)
            if not ok:
                out.update(pivot_min=pmin, nsolves=1)
                return out
            x = z
        else:
            thr = nonneg_threshold(c, K)
            while status == 0:
                # 1: the largest gradient component among the free indices, lowest index among equals
                best, bw = -1, 0.0
                P = np.flatnonzero(inP)
                for i in range(K):
                    if inP[i] or barred[i]:
                        continue
                    w = gradient(A, c, x, P, i)
                    if best < 0 or w > bw:
                        best, bw = i, w
                if best < 0 or not bw > thr:
                    break
                inP[best] = True
                while True:
                    # 2: solve over the passive set
                    if nsolves == 3 * K:
                        status = 4
                        break
                    nsolves += 1
                    P = np.flatnonzero(inP)
                    ok, z, pm = cholesky_subset(A, c, P, tol)
                    if not ok:
                        inP[best] = False
                        barred[best] = True
                        x[best] = 0.0
                        break
                    pmin = pm
                    neg = ~(z > 0.0)
                    if not neg.any():
                        x[P] = z
                        break
                    # 3: the longest feasible step towards z, lowest index among equals
                    alpha, im = np.inf, -1
                    for q in np.flatnonzero(neg):
                        den = x[P[q]] - z[q]
                        a = x[P[q]] / den if den > 0.0 else 0.0
                        if a < alpha:
                            alpha, im = a, P[q]
                    x[P] = x[P] + alpha * (z - x[P])
                    x[im] = 0.0
                    drop = P[~(x[P] > 0.0)]
                    x[drop] = 0.0
                    inP[drop] = False
        if not R > 0.0:
            out.update(pivot_min=pmin, nsolves=nsolves)
            return out
        coef = x * s
        b = N[NG:NG + K]
        xb = 0.0
        for i in range(K):
            xb = xb + coef[i] * b[i]
        xgx = 0.0
        for i in range(K):
            row = 0.0
            for j in range(K):
                row = row + G0[i, j] * coef[j]
            xgx = xgx + coef[i] * row
        val = (R - 2.0 * xb) + xgx
        val = val if val > 0.0 else 0.0
        return dict(coef=coef, misfit=np.sqrt(val / R), status=status, pivot_min=pmin, npositive=int(np.sum(x > 0.0)),
                    nsolves=nsolves, barred=[int(i) for i in np.flatnonzero(barred)],
                    passive=[int(i) for i in np.flatnonzero(inP)] if nonneg else list(range(K)), scaled=(A, c, x.copy()))


def solve(nbr, K, weights=None, anarchy=False, nonneg=False, penalty=None, penalty_relative=False):
    """fold and solve every group: dict(coef, misfit, status, pivot_min, npositive, nsolves, normal)"""
    N = fold(nbr, weights, anarchy)
    res = [solve_one(N[g], K, nonneg, penalty, penalty_relative) for g in range(len(N))]
    return dict(coef=np.stack([r["coef"] for r in res]), misfit=np.array([r["misfit"] for r in res]),
                status=np.array([r["status"] for r in res], np.int32), pivot_min=np.array([r["pivot_min"] for r in res], np.float64),
                npositive=np.array([r["npositive"] for r in res], np.int32), nsolves=np.array([r["nsolves"] for r in res], np.int32),
                normal=N)


def fit(syn, ref, receivers, dt, weights=None, anarchy=False, nonneg=False, penalty=None, penalty_relative=False, syn_factor=1.0):
    """the whole call, as linfit_restatement.fit"""
    K = syn[0].shape[1]
    nrec = len(receivers)
    w = np.ones(nrec) if weights is None else np.array(np.broadcast_to(np.asarray(weights, np.float64), (nrec,)))
    w = np.where([len(sl) > 0 for sl in receivers], w, 0.0)
    nbr = lr.gram_by_receiver(syn, ref, receivers, dt, syn_factor)
    out = solve(nbr, K, w, anarchy, nonneg, penalty, penalty_relative)
    out["by_receiver"] = nbr
    return out
