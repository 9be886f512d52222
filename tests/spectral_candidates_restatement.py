"""The arithmetic of kiwi_hip_spectral_candidates' candidate kernels (kiwi_amd/csrc/kiwi_spectral_candidates.hpp) restated in
numpy, operation for operation and in the same order: the fp32 combination of the basis spectra, the amplitude with a correctly
rounded root, the fp64 sums over the kept bins (bins ascending), the slot misfits and the outer fold of kiwi_outer.hpp for one
draw of weights 1.  The GPU tests feed it with the device's own spectra and ask for the same bits.  Not a test module.

A group is described by per-slot rows: spectra[m] complex as float32 [nbins, K, 2] of the kept bins klo .. khi, refamp[m] and
filtw[m] float32 [nbins], ntrans[m], norm[m] float32 (the slot's norm factor), has_filter[m], slot_receiver[m] (ascending)."""
import numpy as np

F32 = np.float32
NAN = float("nan")


def amp_rn(x, y):
    """|x + i y| of float32 arrays: scaled by the power of two of the larger component, the squares and their sum rounded in
    fp32, a correctly rounded root (numpy's float32 sqrt), scaled back"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        m = np.fmax(np.abs(x), np.abs(y))
        special = ~(m > 0) | (m > F32(3.0e38))
        e = np.frexp(np.where(special, F32(1), m))[1].astype(np.int32)
        sx, sy = np.ldexp(x, -e).astype(F32), np.ldexp(y, -e).astype(F32)
        s = (sx * sx + sy * sy).astype(F32)
        out = np.ldexp(np.sqrt(s).astype(F32), e).astype(F32)
        plain = np.where(m != m, m, np.abs(x) + np.abs(y)).astype(F32)
    return np.where(special, plain, out).astype(F32)


def combine(spec, xf):
    """re, im [ncand, nbins] float32 of X = sum_a xf_a S_a: re = xf_0 S_0.re; re = re + xf_a S_a.re, a ascending"""
    spec, xf = np.asarray(spec, F32), np.asarray(xf, F32)
    re = (xf[:, None, 0] * spec[None, :, 0, 0]).astype(F32)
    im = (xf[:, None, 0] * spec[None, :, 0, 1]).astype(F32)
    for a in range(1, spec.shape[1]):
        re = (re + (xf[:, None, a] * spec[None, :, a, 0]).astype(F32)).astype(F32)
        im = (im + (xf[:, None, a] * spec[None, :, a, 1]).astype(F32)).astype(F32)
    return re, im


def _seq_sum(v):
    """fp64 sum over the bins (axis 1) in ascending order from zero"""
    if v.shape[1] == 0:
        return np.zeros(v.shape[0])
    return np.cumsum(v.astype(np.float64), axis=1)[:, -1]


def slot_sums(spec, refamp, filtw, has_filter, xf, method, syn_factor=1.0, free=False):
    """acc [ncand] of one slot (free: P, Q, A)"""
    sf = F32(syn_factor)
    unit = sf == F32(1)
    re, im = combine(spec, xf)
    b = amp_rn(re, im)
    if has_filter:
        b = (b * np.asarray(filtw, F32)[None, :]).astype(F32)
    a = np.broadcast_to(np.asarray(refamp, F32)[None, :], b.shape)
    if free:
        bs = (b if unit else (sf * b).astype(F32)).astype(np.float64)
        ad = a.astype(np.float64)
        return _seq_sum(ad * bs), _seq_sum(bs * bs), _seq_sum(ad * ad)
    d = (a - b).astype(F32) if unit else ((F32(1) * a).astype(F32) - (sf * b).astype(F32)).astype(F32)
    d = d.astype(np.float64)
    return _seq_sum(d * d) if method == 3 else _seq_sum(np.abs(d))


def df_of(ntrans, dt):
    return F32(1) / (F32(ntrans) * F32(dt))


def best_of(misfit):
    """(index, value) per group: NaN passed over, then the value, then the lowest index; (-1, NaN) if none"""
    bi, bv = np.full(len(misfit), -1, np.int32), np.full(len(misfit), NAN)
    for g, row in enumerate(misfit):
        if np.any(row == row):
            bi[g] = int(np.nanargmin(row))
            bv[g] = row[bi[g]]
    return bi, bv


def evaluate_group(slots, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor=1.0, free_scale=False, cache=None):
    """one group.  slots: list of dicts (spectra, refamp, filtw, ntrans, norm, has_filter) per slot; w [nrec] float64 (0 for a
    disabled receiver).  cache: a dict that keeps the sums over the bins of (slot, method, free_scale) between calls that differ in
    the fold only (same slots, x and syn_factor).  Returns (misfit [ncand], scale [ncand] or None, slot_misfit [ncand, nmis]
    float32, status)"""
    def sums(m, sl, free):
        key = (m, method, free)
        if cache is None or key not in cache:
            r = slot_sums(sl["spectra"], sl["refamp"], sl["filtw"], sl["has_filter"], xf, method, syn_factor, free)
            if cache is None:
                return r
            cache[key] = r
        return cache[key]

    xf = np.asarray(x, np.float64).astype(F32)
    nc, nmis = len(xf), len(slots)
    l2 = outer == "l2norm"
    w = np.asarray(w, np.float64)
    smis = np.zeros((nc, nmis), F32)
    ms, ns = np.zeros(nc), 0.0
    SP, SQ, SA = np.zeros(nc), np.zeros(nc), np.zeros(nc)
    Mr, Nr = np.zeros(nc), 0.0
    pr, qr, ar = np.zeros(nc), np.zeros(nc), np.zeros(nc)
    with np.errstate(all="ignore"):
        for m, sl in enumerate(slots):
            df = np.float64(df_of(sl["ntrans"], dt))
            nv = np.float64(F32(sl["norm"]))
            if free_scale:
                P, Q, A = sums(m, sl, True)
                pr, qr, ar = pr + df * P, qr + df * Q, ar + df * A
                Nr = Nr + nv * nv
            else:
                acc = sums(m, sl, False)
                mf = np.sqrt(df * acc).astype(F32) if method == 3 else (df * acc).astype(F32)
                smis[:, m] = mf
                mv = mf.astype(np.float64)
                if l2:
                    Mr, Nr = Mr + mv * mv, Nr + nv * nv
                else:
                    Mr, Nr = Mr + mv, Nr + nv
            if m + 1 < nmis and slot_receiver[m + 1] == slot_receiver[m]:
                continue
            if l2:
                Mr, Nr = np.sqrt(Mr), np.sqrt(Nr)
            rw = w[slot_receiver[m]]
            if anarchy:
                q = rw / (Nr if Nr != 0.0 else -1.0)
                rw = q if (q > 0.0 or q != q) else 0.0
            bv = Nr * rw
            if free_scale:
                W = rw * rw
                SP, SQ, SA = SP + W * pr, SQ + W * qr, SA + W * ar
                ns = ns + bv * bv
            else:
                av = Mr * rw
                if l2:
                    av, bv = av * av, bv * bv
                ms, ns = ms + av * 1.0, ns + bv * 1.0
            Mr, Nr = np.zeros(nc), 0.0
            pr, qr, ar = np.zeros(nc), np.zeros(nc), np.zeros(nc)
        misfit, scale = np.full(nc, NAN), None
        if free_scale:
            scale = np.where(SQ > 0.0, SP / np.where(SQ > 0.0, SQ, 1.0), NAN)
            if ns > 0.0:
                val = (SA - 2.0 * scale * SP) + (scale * scale) * SQ
                val = np.where(val > 0.0, val, np.where(val == val, 0.0, val))
                misfit = np.sqrt(val / ns)
        elif ns > 0.0:
            misfit = ms / ns
            if l2:
                misfit = np.sqrt(misfit)
            misfit = np.where(misfit >= 0.0, misfit, NAN)
    return misfit, scale, smis, (0 if ns > 0.0 else 1)


def evaluate(groups, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor=1.0, free_scale=False, cache=None):
    """groups: list of slot lists.  cache: a dict (see evaluate_group), one entry per group is made in it.  Returns a dict of
    arrays as the call returns them"""
    res = [evaluate_group(g, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor, free_scale,
                          None if cache is None else cache.setdefault(i, {})) for i, g in enumerate(groups)]
    misfit = np.array([r[0] for r in res])
    bi, bv = best_of(misfit)
    return dict(misfit=misfit, scale=np.array([r[1] for r in res]) if free_scale else None,
                slot_misfit=np.array([r[2] for r in res]), status=np.array([r[3] for r in res], np.int32), best_index=bi, best_misfit=bv)


def groups_from_scan(scan, has_filter):
    """the per-slot rows of every group from a `SpectralCandidateScan` with spectra and slot norms"""
    out = []
    for g in range(len(scan.spectra)):
        slots = []
        for m in range(scan.spectra.shape[1]):
            klo, khi, nt = (int(v) for v in scan.spectra_range[g, m])
            nb = max(khi - klo + 1, 0)
            slots.append(dict(spectra=scan.spectra[g, m, :nb], refamp=scan.spectra_ref[g, m, :nb, 0], filtw=scan.spectra_ref[g, m, :nb, 1],
                              ntrans=nt, norm=scan.slot_norm[g, m], has_filter=bool(has_filter[m]), klo=klo, khi=khi))
        out.append(slots)
    return out


# ---- what the host does around the kernels, for inputs that do not come from the device --------------------------------------
def filter_weights(fx, fy, nb, df):
    """plf_taper_array with cosine flanks on ones (kiwi_host.hpp): weight of bin j at abscissa j df, float32"""
    fx, fy, df = np.asarray(fx, F32), np.asarray(fy, F32), F32(df)
    a = np.ones(nb, F32)
    ibeg = int(np.floor(fx[0] / df))
    a[:max(min(ibeg, nb - 1) + 1, 0)] = 0
    atleast = 0
    for i in range(len(fx) - 1):
        ibeg = max(int(np.floor(fx[i] / df)) + 1, 0, atleast)
        iend = min(int(np.floor(fx[i + 1] / df)), nb - 1)
        for j in range(ibeg, iend + 1):
            xi = F32(j) * df
            if fy[i + 1] != fy[i]:
                f = fy[i] + (fy[i + 1] - fy[i]) * (F32(0.5) - F32(0.5) * F32(np.cos(F32((xi - fx[i]) / (fx[i + 1] - fx[i]) * F32(np.pi)))))
            else:
                f = fy[i]
            a[j] = a[j] * F32(f)
        atleast = iend + 1
    iend = int(np.floor(fx[-1] / df)) + 1
    if nb - 1 >= iend:
        a[max(iend, 0):] = 0
    return a


def kept_range(filtw, refamp, has_filter):
    """the smallest bin range that holds every non-zero filter weight; a skipped bin with a non-zero reference amplitude is an
    error (the call refuses it)"""
    nb = len(filtw)
    if not has_filter:
        return 0, nb - 1
    nz = np.nonzero(np.asarray(filtw) != 0)[0]
    klo, khi = (int(nz[0]), int(nz[-1])) if len(nz) else (0, -1)
    skipped = np.ones(nb, bool)
    skipped[klo:khi + 1] = False
    if np.any(np.asarray(refamp)[skipped] != 0):
        raise ValueError("a skipped bin has a reference amplitude that is not 0")
    return klo, khi


def spectra_of(traces, ntrans):
    """complex spectra of K real traces [K, wlen] zero-padded to ntrans, as float32 [ntrans / 2 + 1, K, 2] (numpy's fp64
    transform rounded once)"""
    z = np.fft.rfft(np.asarray(traces, np.float64), n=ntrans, axis=1)
    return np.stack([z.real.T, z.imag.T], axis=2).astype(F32)
