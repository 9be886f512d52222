"""numpy restatement of kiwi_hip_linear_fit_robust (kiwi_amd/csrc/kiwi_linfit_robust.hpp): the l2 start of
tests/linfit_restatement.py, then the reweighting passes of mode A (inner l1norm) or mode B (inner l2norm), every fp64
operation in the documented order, so that the device can be asked for the same BITS.  Traces and receivers in the layout
of tests/linfit_restatement.py.  Not a test module: tests/test_linfit_robust.py and tests/test_linfit_robust_gpu.py use it."""
import numpy as np

from tests import linfit_restatement as lr

THREADS = lr.THREADS


def na_of(K):
    return K * (K + 1) // 2 + K + 3


def huber(m, a):
    with np.errstate(all="ignore"):
        return np.where(m >= a, m - 0.5 * a, (m * m) / (2.0 * a))


def cholesky(S, K):
    """scaled_cholesky on sums [ng, >= NG + K] laid out as G upper triangle by rows, then b: (x [ng, K] with NaN where it
    failed, ok [ng]).  lr.solve with the sums as its one receiver of weight 1: 0 + 1 x S is S bit for bit."""
    NG = K * (K + 1) // 2
    one = np.concatenate([S[:, :NG + K], np.ones((len(S), 1))], 1)[:, None, :]
    out = lr.solve(one, K)
    return out["coef"], out["status"] == 0


def _weights(receivers, weights):
    nrec = len(receivers)
    w = np.ones(nrec) if weights is None else np.array(np.broadcast_to(np.asarray(weights, np.float64), (nrec,)))
    return np.where([len(sl) > 0 for sl in receivers], w, 0.0)


def pass_by_receiver(syn, ref, receivers, dt, x, nbr, w, eps, syn_factor=1.0):
    """robust_pass_kernel: [ngroup, nrec, NA] sums G, b, L, H, D of every receiver at the coefficients x [ngroup, K]; zeros
    for skipped receivers (w == 0 or not R_r > 0: per group)."""
    ngroup, K = syn[0].shape[0], syn[0].shape[1]
    NG, NN, NA = K * (K + 1) // 2, lr.nn_of(K), na_of(K)
    f = np.float32(syn_factor)
    dt64 = np.float64(np.float32(dt))
    out = np.zeros((ngroup, len(receivers), NA))
    with np.errstate(all="ignore"):
        for r, slots in enumerate(receivers):
            if not slots or w[r] == 0.0:
                continue
            Rr = nbr[:, r, NN - 1]
            T = sum(np.asarray(ref[m]).shape[0] for m in slots)
            ar = (np.float64(eps) * np.sqrt(Rr / (dt64 * np.float64(T))))[:, None]
            acc = np.zeros((ngroup, NA, THREADS))
            for m in slots:
                s32 = np.asarray(syn[m], np.float32)
                if f != np.float32(1.0):
                    s32 = f * s32
                wlen = s32.shape[2]
                nstep = (wlen + THREADS - 1) // THREADS
                s = np.zeros((ngroup, K, nstep * THREADS))       # (a sample past the window adds +0.0 to every sum)
                s[:, :, :wlen] = s32
                d = np.zeros(nstep * THREADS)
                d[:wlen] = np.asarray(ref[m], np.float32)
                for j in range(nstep):
                    sj = s[:, :, j * THREADS:(j + 1) * THREADS]
                    dj = d[j * THREADS:(j + 1) * THREADS][None, :]
                    pred = np.zeros((ngroup, THREADS))
                    for a in range(K):
                        pred = pred + x[:, a, None] * sj[:, a]
                    e = dj - pred
                    ae = np.abs(e)
                    om = 1.0 / np.where(ae > ar, ae, ar)
                    o = [om * sj[:, a] for a in range(K)]
                    p = 0
                    for a in range(K):
                        for b in range(a, K):
                            acc[:, p] = acc[:, p] + o[a] * sj[:, b]
                            p += 1
                    for a in range(K):
                        acc[:, NG + a] = acc[:, NG + a] + o[a] * dj
                    acc[:, NG + K] = acc[:, NG + K] + ae
                    acc[:, NG + K + 1] = acc[:, NG + K + 1] + huber(ae, ar)
                    acc[:, NG + K + 2] = acc[:, NG + K + 2] + np.abs(dj)
            v = acc.reshape(ngroup, NA, THREADS // 64, 64).copy()
            off = 32
            while off > 0:
                v[..., :off] = v[..., :off] + v[..., off:2 * off]
                off //= 2
            t = (v[:, :, 0, 0] + v[:, :, 1, 0]) + (v[:, :, 2, 0] + v[:, :, 3, 0])
            out[:, r] = np.where((Rr > 0.0)[:, None], dt64 * t, 0.0)
    return out


def fold_a(wbr, nbr, K, w, anarchy):
    """robust_step_kernel's fold: S [ng, NA]"""
    ng, nrec, NA = wbr.shape
    NN = lr.nn_of(K)
    S = np.zeros((ng, NA))
    with np.errstate(all="ignore"):
        for r in range(nrec):
            if w[r] == 0.0:
                continue
            take = nbr[:, r, NN - 1] > 0.0
            v = np.full(ng, w[r])
            if anarchy:
                Dr = wbr[:, r, NA - 1]
                v = np.where(Dr > 0.0, v / np.where(Dr > 0.0, Dr, 1.0), 0.0)
                take = take & (v != 0.0)
            S = np.where(take[:, None], S + v[:, None] * wbr[:, r, :], S)
    return S


def sums_b(nbr, K, x, w, anarchy, eps):
    """one iteration of robust_receiver_kernel before its solve: (S [ng, NG + K], L, H, D [ng])"""
    ng, nrec, NN = nbr.shape
    NG = K * (K + 1) // 2
    S = np.zeros((ng, NG + K))
    Ls, Hs, Ds = np.zeros(ng), np.zeros(ng), np.zeros(ng)
    with np.errstate(all="ignore"):
        for r in range(nrec):
            if w[r] == 0.0:
                continue
            q = nbr[:, r, :]
            Rr = q[:, NN - 1]
            take = Rr > 0.0
            xb = np.zeros(ng)
            for i in range(K):
                xb = xb + x[:, i] * q[:, NG + i]
            xgx = np.zeros(ng)
            for i in range(K):
                row = np.zeros(ng)
                for j in range(K):
                    row = row + q[:, lr.tri(K, min(i, j), max(i, j))] * x[:, j]
                xgx = xgx + x[:, i] * row
            val = (Rr - 2.0 * xb) + xgx
            val = np.where(val > 0.0, val, 0.0)
            m, n = np.sqrt(val), np.sqrt(np.where(take, Rr, 1.0))
            v = np.full(ng, w[r]) / n if anarchy else np.full(ng, w[r])
            a = np.float64(eps) * n
            u = v / np.where(m > a, m, a)
            S = np.where(take[:, None], S + u[:, None] * q[:, :NG + K], S)
            Ls = np.where(take, Ls + v * m, Ls)
            Hs = np.where(take, Hs + v * huber(m, a), Hs)
            Ds = np.where(take, Ds + v * n, Ds)
    return S, Ls, Hs, Ds


def fit(syn, ref, receivers, dt, mode, weights=None, anarchy=False, niter=8, eps=1e-3, syn_factor=1.0):
    """the whole call, mode "A" (inner l1norm, outer l1norm) or "B" (inner l2norm, outer l1norm): dict(coef [ng, K], misfit
    [ng], status [ng] int32, trace [ng, niter + 1, 2], start: the l2 fit of lr.fit; coef_at [ng, niter + 1, K], misfit_at,
    status_at [ng, niter + 1]: what a call with niter = n answers, for every n <= niter -- its trace is trace[:, :n + 1])"""
    K = syn[0].shape[1]
    ng = syn[0].shape[0]
    NG = K * (K + 1) // 2
    w = _weights(receivers, weights)
    start = lr.fit(syn, ref, receivers, dt, weights, anarchy, syn_factor)
    nbr = start["by_receiver"]
    x = start["coef"].copy()
    status = start["status"].copy()
    misfit = start["misfit"].copy()
    trace = np.full((ng, niter + 1, 2), np.nan)
    coef_at, misfit_at, status_at = np.zeros((ng, niter + 1, K)), np.zeros((ng, niter + 1)), np.zeros((ng, niter + 1), np.int32)
    with np.errstate(all="ignore"):
        for it in range(niter + 1):
            active = status == 0
            if mode == "A":
                S = fold_a(pass_by_receiver(syn, ref, receivers, dt, x, nbr, w, eps, syn_factor), nbr, K, w, anarchy)
                Ls, Hs, Ds = S[:, NG + K], S[:, NG + K + 1], S[:, NG + K + 2]
            else:
                S, Ls, Hs, Ds = sums_b(nbr, K, x, w, anarchy, eps)
            trace[:, it, 0] = np.where(active, Hs / Ds, np.nan)
            trace[:, it, 1] = np.where(active, Ls / Ds, np.nan)
            misfit = np.where(active, Ls / Ds, misfit)
            coef_at[:, it], misfit_at[:, it], status_at[:, it] = x, misfit, status
            if it == niter:
                break
            xn, ok = cholesky(S, K)
            status = np.where(active & ~ok, 3, status).astype(np.int32)
            x = np.where((active & ok)[:, None], xn, x)
    return dict(coef=x, misfit=misfit, status=status, trace=trace, start=start, coef_at=coef_at, misfit_at=misfit_at, status_at=status_at)


def forwarded(syn, ref, receivers, dt, weights=None, anarchy=False, niter=8, syn_factor=1.0):
    """l2norm inside and outside: lr.fit's answer, its misfit as the one trace row there is"""
    start = lr.fit(syn, ref, receivers, dt, weights, anarchy, syn_factor)
    trace = np.full((len(start["misfit"]), max(niter, 0) + 1, 2), np.nan)
    trace[:, 0, 0] = trace[:, 0, 1] = start["misfit"]
    return dict(coef=start["coef"], misfit=start["misfit"], status=start["status"], trace=trace, start=start)
