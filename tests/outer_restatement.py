"""CPU restatement of the device's outer misfits and per-draw minima (kiwi_amd/csrc/kiwi_outer.hpp): numpy, fp64, in the
device's operation order, so that the GPU tests can ask for bit identity.  Sequential sums are loops (over a receiver's
slots k, over the receivers r), vectorised over sources and draws; every product, sum, quotient and root is one IEEE
operation in numpy as on the device (-ffp-contract=off there: no fused multiply-add).

What it restates, in the reference's terms (seismosizer.py:843-922, as kiwi_amd/engine.py make_global_misfits has it):
  prepare  per (source, receiver): l1norm M = sum_k m, N = sum_k n; l2norm M = sqrt(sum_k m m), N = sqrt(sum_k n n);
           receiver weight rw = w_r, with anarchy q = w_r / (N != 0 ? N : -1), rw = q if q > 0 or NaN else 0
           (numpy's maximum(q, 0)); a = M rw, b = N rw, both squared under l2norm;
  draws    ms = sum_r a c[d, r], ns = sum_r b c[d, r], r ascending, from zero; g = ms / ns where ns > 0 (its root under
           l2norm); excluded (NaN) where ns <= 0 or g < 0 or g is NaN.  The host multiplies rw by sqrt(c) BEFORE squaring;
           the device multiplies the square by c: a few ulp apart, deliberately;
  minima   per draw the lowest g and the LOWEST source index that has it (nanargmin); NaN, 0 when every source is excluded."""
import numpy as np


def prepare(misfit, norm, slot_receiver, nrec, outer_norm, receiver_weights=None, anarchy=False):
    """a, b [N_s, nrec] float64 from the per-slot float32 arrays [N_s, nmis]."""
    m = np.asarray(misfit, np.float32)
    n = np.asarray(norm, np.float32)
    sr = np.asarray(slot_receiver, np.int64)
    l2 = {"l1norm": False, "l2norm": True}[outer_norm]
    ns = m.shape[0]
    w = np.ones(nrec) if receiver_weights is None else np.broadcast_to(np.asarray(receiver_weights, np.float64), (nrec,))
    a = np.zeros((ns, nrec))
    b = np.zeros((ns, nrec))
    with np.errstate(all="ignore"):
        for r in range(nrec):
            M = np.zeros(ns)
            N = np.zeros(ns)
            for k in np.nonzero(sr == r)[0]:                      # slot order
                mv = m[:, k].astype(np.float64)
                nv = n[:, k].astype(np.float64)
                if l2:
                    M = M + mv * mv
                    N = N + nv * nv
                else:
                    M = M + mv
                    N = N + nv
            if l2:
                M = np.sqrt(M)
                N = np.sqrt(N)
            rw = np.full(ns, w[r])
            if anarchy:
                q = rw / np.where(N != 0.0, N, -1.0)
                rw = np.where((q > 0.0) | np.isnan(q), q, 0.0)
            av = M * rw
            bv = N * rw
            if l2:
                av = av * av
                bv = bv * bv
            a[:, r] = av
            b[:, r] = bv
    return a, b


def draw_misfits(a, b, draw_weights, outer_norm):
    """g [N_s, B]: the global misfit of every source under every draw, NaN where excluded."""
    l2 = {"l1norm": False, "l2norm": True}[outer_norm]
    c = np.asarray(draw_weights, np.float64)
    ns, nrec = a.shape
    ms = np.zeros((ns, len(c)))
    nn = np.zeros((ns, len(c)))
    with np.errstate(all="ignore"):
        for r in range(nrec):
            ms = ms + a[:, r, None] * c[None, :, r]
            nn = nn + b[:, r, None] * c[None, :, r]
        pos = nn > 0.0
        g = np.where(pos, ms / np.where(pos, nn, 1.0), np.nan)
        if l2:
            g = np.sqrt(g)
        g = np.where(g >= 0.0, g, np.nan)
    return g


def minima(g):
    """(best_value[B], best_index[B]) of g [N_s, B]: lowest value, then lowest source index; NaN, 0 without a candidate."""
    nd = g.shape[1]
    bv = np.full(nd, np.nan)
    bi = np.zeros(nd, np.int32)
    if g.shape[0] == 0:
        return bv, bi
    has = ~np.all(np.isnan(g), 0)
    if np.any(has):
        gh = g[:, has]
        with np.errstate(all="ignore"):
            vmin = np.nanmin(gh, 0)
        bi[has] = np.argmax(gh == vmin[None, :], 0)               # the first source that has the lowest value (a NaN never equals)
        bv[has] = vmin
    return bv, bi


def outer_misfits(misfit, norm, slot_receiver, nrec, outer_norm="l2norm", receiver_weights=None, anarchy=False,
                  draw_weights=None, which_draw=None, block=512):
    """What kiwi_hip_outer_misfits answers: (best_value[B], best_index[B], global_of_draw[N_s] or None).  Draws go in blocks
    (the [N_s, B] matrix of a large case need not exist at once); the arithmetic per element does not depend on it."""
    dw = np.ones((1, nrec)) if draw_weights is None else np.asarray(draw_weights, np.float64)
    a, b = prepare(misfit, norm, slot_receiver, nrec, outer_norm, receiver_weights, anarchy)
    bv = np.full(len(dw), np.nan)
    bi = np.zeros(len(dw), np.int32)
    gout = None
    for d0 in range(0, len(dw), block):
        g = draw_misfits(a, b, dw[d0:d0 + block], outer_norm)
        bv[d0:d0 + block], bi[d0:d0 + block] = minima(g)
        if which_draw is not None and d0 <= which_draw < d0 + block:
            gout = g[:, which_draw - d0].copy()
    return bv, bi, gout


def flatten(misfits_by_src, norms_by_src, ncomponents):
    """The per-slot float32 arrays [N_s, nmis] and slot_receiver[nmis] of [N_s, N_r, N_k] arrays whose receiver r has
    ncomponents[r] slots (Engine.outer_misfits does the same)."""
    m = np.asarray(misfits_by_src)
    n = np.asarray(norms_by_src)
    nrec = m.shape[1]
    cols = [(r, k) for r in range(nrec) for k in range(int(ncomponents[r]))]
    ri = np.array([r for r, _ in cols], np.int64)
    ki = np.array([k for _, k in cols], np.int64)
    return m[:, ri, ki].astype(np.float32), n[:, ri, ki].astype(np.float32), ri.astype(np.int32)
