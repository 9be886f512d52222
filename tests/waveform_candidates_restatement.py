"""The arithmetic of kiwi_hip_waveform_candidates (kiwi_amd/csrc/kiwi_waveform_candidates.hpp) restated in numpy, operation for
operation and in the same order: the fp32 combination of the basis rows, the residual as misfit_kernel forms it, the fp64 sum
over the window samples (ascending), the slot misfits and the outer fold of kiwi_outer.hpp for one draw of weights 1.  The GPU
tests feed it with the device's own kept traces and ask for the same bits.  Not a test module.

Traces come in the layout of tests/linfit_cases.py: syn[m] float32 [ngroup, K, wlen_m] (the kept rows, WITHOUT the synthetics
factor), ref[m] float32 [wlen_m] (the reference side of the same comparison), norm float32 [ngroup, nmis] (the slot norm factors
of every group's first source), slot_receiver[m] (ascending), w [nrec] float64 (0 for a disabled receiver).  method 1 l2norm,
2 l1norm."""
import numpy as np

F32 = np.float32
NAN = float("nan")


def combine(rows, xf):
    """v [ncand, wlen] float32 of sum_a xf_a s_a: v = xf_0 s_0; v = v + xf_a s_a, a ascending, every product and sum rounded"""
    rows, xf = np.asarray(rows, F32), np.asarray(xf, F32)
    v = (xf[:, None, 0] * rows[None, 0, :]).astype(F32)
    for a in range(1, rows.shape[0]):
        v = (v + (xf[:, None, a] * rows[None, a, :]).astype(F32)).astype(F32)
    return v


def _seq_sum(v):
    """fp64 sum over the samples (axis 1) in ascending order from zero"""
    if v.shape[1] == 0:
        return np.zeros(v.shape[0])
    return np.cumsum(v.astype(np.float64), axis=1)[:, -1]


def slot_sums(rows, ref, xf, method, syn_factor=1.0):
    """acc [ncand] float64 of one slot"""
    sf = F32(syn_factor)
    with np.errstate(all="ignore"):
        v = combine(rows, xf)
        a = np.broadcast_to(np.asarray(ref, F32)[None, :], v.shape)
        d = (a - v).astype(F32) if sf == F32(1) else ((F32(1) * a).astype(F32) - (sf * v).astype(F32)).astype(F32)
        d = d.astype(np.float64)
        return _seq_sum(d * d) if method == 1 else _seq_sum(np.abs(d))     # (d d is exact in fp64: the fused multiply-add rounds once)


def slot_misfits(rows, ref, x, method, dt, syn_factor=1.0):
    """float32 [ncand] of one slot: (float) sqrt((double) dt acc) | (float) ((double) dt acc)"""
    xf = np.atleast_2d(np.asarray(x, np.float64)).astype(F32)
    acc = slot_sums(rows, ref, xf, method, syn_factor)
    d = np.float64(F32(dt))
    return np.sqrt(d * acc).astype(F32) if method == 1 else (d * acc).astype(F32)


def fold(smis, norm, slot_receiver, w, anarchy, outer):
    """(misfit [ncand] float64, status) of one group from its slot misfits smis [ncand, nmis] float32 and norm factors norm [nmis]:
    kiwi_hip_outer_misfits for one draw of weights 1, per slot"""
    smis, norm = np.asarray(smis, F32), np.asarray(norm, F32)
    nc, nmis = smis.shape
    l2 = {"l1norm": False, "l2norm": True}[outer]
    w = np.asarray(w, np.float64)
    ms, ns = np.zeros(nc), 0.0
    Mr, Nr = np.zeros(nc), 0.0
    with np.errstate(all="ignore"):
        for m in range(nmis):
            mv, nv = smis[:, m].astype(np.float64), np.float64(norm[m])
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
            av, bv = Mr * rw, Nr * rw
            if l2:
                av, bv = av * av, bv * bv
            ms, ns = ms + av * 1.0, ns + bv * 1.0
            Mr, Nr = np.zeros(nc), 0.0
        misfit = np.full(nc, NAN)
        if nmis > 0 and ns > 0.0:
            misfit = ms / ns
            if l2:
                misfit = np.sqrt(misfit)
            misfit = np.where(misfit >= 0.0, misfit, NAN)
    return misfit, (0 if nmis > 0 and ns > 0.0 else 1)


def best_of(misfit):
    """(index, value) per group: NaN passed over, then the value, then the lowest index; (-1, NaN) if none"""
    bi, bv = np.full(len(misfit), -1, np.int32), np.full(len(misfit), NAN)
    for g, row in enumerate(misfit):
        if np.any(row == row):
            bi[g] = int(np.nanargmin(row))
            bv[g] = row[bi[g]]
    return bi, bv


def slot_misfits_of(syn, ref, x, method, dt, syn_factor=1.0):
    """float32 [ngroup, ncand, nmis]: the slot misfits of every group (they do not depend on the fold)"""
    ngroup = syn[0].shape[0] if len(syn) else 0
    x = np.atleast_2d(np.asarray(x, np.float64))
    out = np.zeros((ngroup, len(x), len(syn)), F32)
    for m in range(len(syn)):
        for g in range(ngroup):
            out[g, :, m] = slot_misfits(syn[m][g], ref[m], x, method, dt, syn_factor)
    return out


def evaluate(syn, ref, norm, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor=1.0, smis=None):
    """a dict of arrays as the call returns them.  smis: `slot_misfits_of` of the same traces, candidates, method and factor, where
    several folds are made of them"""
    if smis is None:
        smis = slot_misfits_of(syn, ref, x, method, dt, syn_factor)
    norm = np.asarray(norm, F32).reshape(len(smis), -1)
    res = [fold(smis[g], norm[g], slot_receiver, w, anarchy, outer) for g in range(len(smis))]
    misfit = np.array([r[0] for r in res])
    bi, bv = best_of(misfit)
    return dict(misfit=misfit, slot_misfit=smis, slot_norm=norm, status=np.array([r[1] for r in res], np.int32), best_index=bi, best_misfit=bv)
