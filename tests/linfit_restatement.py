"""numpy restatement of kiwi_hip_linear_fit (kiwi_amd/csrc/kiwi_linfit.hpp): traces in, coef / misfit / status / pivot_min /
normal / normal_by_receiver out, every fp64 operation in the documented order, so that the device can be asked for the same
BITS.  Not a test module: tests/test_linfit.py and tests/test_linfit_gpu.py use it.

Traces: per misfit slot (enabled receivers, receiver-major, components in string order) `syn[slot]` float32
[ngroup, K, wlen] -- what the comparator holds of every basis source before the synthetics factor -- and `ref[slot]` float32
[wlen], the reference side of the same comparison.  `receivers`: for EVERY receiver the list of its slots ([] if disabled)."""
import numpy as np

THREADS = 256


def nn_of(K):
    return K * (K + 1) // 2 + K + 1


def tri(K, i, j):
    """index of G[i][j], i <= j, in the upper triangle stored by rows"""
    return i * K - i * (i - 1) // 2 + (j - i)


def gram_by_receiver(syn, ref, receivers, dt, syn_factor=1.0):
    """[ngroup, nrec, NN]: G_r (upper triangle by rows), b_r, R_r of every receiver; zeros for disabled ones.  Thread tid of
    256 takes samples tid, tid + 256, ... of the receiver's first slot, then of the next, into the same accumulators; tree:
    lanes of a wavefront v[l] + v[l + off], off = 32 ... 1; then (w0 + w1) + (w2 + w3); times dt."""
    ngroup, K = syn[0].shape[0], syn[0].shape[1]
    NG, NN = K * (K + 1) // 2, nn_of(K)
    f = np.float32(syn_factor)
    out = np.zeros((ngroup, len(receivers), NN))
    for r, slots in enumerate(receivers):
        if not slots:
            continue
        acc = np.zeros((ngroup, NN, THREADS))
        for m in slots:
            s32 = np.asarray(syn[m], np.float32)
            if f != np.float32(1.0):
                s32 = f * s32                                # fp32 product, as the comparator forms it
            wlen = s32.shape[2]
            nstep = (wlen + THREADS - 1) // THREADS
            s = np.zeros((ngroup, K, nstep * THREADS))       # (a sample past the window adds +0.0: leaves every sum as it is)
            s[:, :, :wlen] = s32
            d = np.zeros(nstep * THREADS)
            d[:wlen] = np.asarray(ref[m], np.float32)
            for j in range(nstep):
                sj = s[:, :, j * THREADS:(j + 1) * THREADS]
                dj = d[j * THREADS:(j + 1) * THREADS]
                p = 0
                for a in range(K):
                    for b in range(a, K):
                        acc[:, p] = acc[:, p] + sj[:, a] * sj[:, b]
                        p += 1
                for a in range(K):
                    acc[:, NG + a] = acc[:, NG + a] + sj[:, a] * dj
                acc[:, NN - 1] = acc[:, NN - 1] + dj * dj
        v = acc.reshape(ngroup, NN, THREADS // 64, 64).copy()
        off = 32
        while off > 0:
            v[..., :off] = v[..., :off] + v[..., off:2 * off]
            off //= 2
        t = (v[:, :, 0, 0] + v[:, :, 1, 0]) + (v[:, :, 2, 0] + v[:, :, 3, 0])
        out[:, r] = np.float64(np.float32(dt)) * t
    return out


def solve(nbr, K, weights=None, anarchy=False):
    """fold the receivers with their weights and solve; nbr [ngroup, nrec, NN] from gram_by_receiver, weights [nrec] with
    zeros for disabled receivers (None: ones)."""
    ng, nrec, NN = nbr.shape
    NG = K * (K + 1) // 2
    w = np.ones(nrec) if weights is None else np.asarray(weights, np.float64)
    with np.errstate(all="ignore"):
        N = np.zeros((ng, NN))
        for r in range(nrec):
            if w[r] == 0.0:
                continue
            wr = np.full(ng, w[r])
            if anarchy:
                Rr = nbr[:, r, NN - 1]
                wr = np.where(Rr > 0.0, wr / np.sqrt(np.where(Rr > 0.0, Rr, 1.0)), 0.0)
            w2 = wr * wr
            N = np.where((wr != 0.0)[:, None], N + w2[:, None] * nbr[:, r, :], N)
        R = N[:, NN - 1]
        D = [N[:, tri(K, i, i)] for i in range(K)]
        diag_ok = np.ones(ng, bool)
        for i in range(K):
            diag_ok &= D[i] > 0.0
        s = [1.0 / np.sqrt(D[i]) for i in range(K)]
        tol = K * 2.0 ** -52
        L = np.zeros((ng, K, K))
        ok = np.ones(ng, bool)
        pmin = np.ones(ng)
        for j in range(K):
            d = np.ones(ng)
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            pmin = np.where(ok & (d < pmin), d, pmin)
            ok = ok & (d > tol)
            ljj = np.sqrt(d)
            L[:, j, j] = ljj
            for i in range(j + 1, K):
                v = (N[:, tri(K, j, i)] * s[i]) * s[j]
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / ljj
        y = [None] * K
        for i in range(K):
            v = N[:, NG + i] * s[i]
            for k in range(i):
                v = v - L[:, i, k] * y[k]
            y[i] = v / L[:, i, i]
        for i in range(K - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, K):
                v = v - L[:, k, i] * y[k]
            y[i] = v / L[:, i, i]
        x = [y[i] * s[i] for i in range(K)]
        status = np.where(diag_ok & ok, 0, 1).astype(np.int32)
        pmin = np.where(diag_ok, pmin, 0.0)
        status = np.where(R > 0.0, status, 1).astype(np.int32)
        xb = np.zeros(ng)
        for i in range(K):
            xb = xb + x[i] * N[:, NG + i]
        xgx = np.zeros(ng)
        for i in range(K):
            row = np.zeros(ng)
            for j in range(K):
                row = row + N[:, tri(K, min(i, j), max(i, j))] * x[j]
            xgx = xgx + x[i] * row
        val = (R - 2.0 * xb) + xgx
        val = np.where(val > 0.0, val, 0.0)
        mis = np.sqrt(val / R)
        solved = status == 0
        coef = np.where(solved[:, None], np.stack(x, 1), np.nan)
        mis = np.where(solved, mis, np.nan)
    return dict(coef=coef, misfit=mis, status=status, pivot_min=pmin, normal=N)


def fit(syn, ref, receivers, dt, weights=None, anarchy=False, syn_factor=1.0):
    """the whole call: dict(coef, misfit, status, pivot_min, normal, by_receiver).  weights: [nrec] or None = ones; a
    disabled receiver (no slots) never counts."""
    K = syn[0].shape[1]
    nrec = len(receivers)
    w = np.ones(nrec) if weights is None else np.array(np.broadcast_to(np.asarray(weights, np.float64), (nrec,)))
    w = np.where([len(sl) > 0 for sl in receivers], w, 0.0)
    nbr = gram_by_receiver(syn, ref, receivers, dt, syn_factor)
    out = solve(nbr, K, w, anarchy)
    out["by_receiver"] = nbr
    return out


def predicted_slot_misfits(nbr_slots, coef):
    """per-slot l2norm misfit sqrt(R - 2 x.b + x.G.x) of the combination `coef` [K] from per-SLOT sums [nslot, NN] (a
    gram_by_receiver call with every slot as a receiver of its own), plain numpy: what an evaluation of the fitted source should give"""
    nslot, NN = nbr_slots.shape
    K = len(coef)
    NG = K * (K + 1) // 2
    out = np.zeros(nslot)
    for m in range(nslot):
        G = np.zeros((K, K))
        for i in range(K):
            for j in range(i, K):
                G[i, j] = G[j, i] = nbr_slots[m, tri(K, i, j)]
        b = nbr_slots[m, NG:NG + K]
        out[m] = np.sqrt(max(nbr_slots[m, NN - 1] - 2.0 * coef @ b + coef @ G @ coef, 0.0))
    return out


def full_matrix(normal, K):
    """(G [K, K] symmetric, b [K], R) of one row of `normal`"""
    G = np.zeros((K, K))
    for i in range(K):
        for j in range(i, K):
            G[i, j] = G[j, i] = normal[tri(K, i, j)]
    NG = K * (K + 1) // 2
    return G, np.array(normal[NG:NG + K]), float(normal[NG + K])
