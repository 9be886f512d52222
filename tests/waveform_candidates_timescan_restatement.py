"""The arithmetic of kiwi_hip_waveform_candidates_time_scan (kiwi_amd/csrc/kiwi_waveform_candidates_timescan.hpp) restated in
numpy, operation for operation and in the same order: the fp32 combination of the UNTAPERED basis rows once per extended sample,
per offset the taper product, the residual as misfit_kernel forms it and the fp64 sum over the window samples (ascending), the
slot misfits, the fold of tests/waveform_candidates_restatement.py per (group, offset) and the first minimum over the offsets.  The
GPU tests feed it with the call's own rows and ask for the same bits.  Not a test module.

raw[m] float32 [ngroup, K, wlen_m + 2 S]: the folded, scaled, untapered rows over the window made S = max |k| samples wider on
either side; taper[m] float32 [wlen_m]; ref[m] float32 [wlen_m], the tapered reference; norm float32 [ngroup, nmis];
slot_receiver[m] (ascending); w [nrec] float64 (0 for a disabled receiver).  method 1 l2norm, 2 l1norm.  Offsets k0 + j kstep."""
import numpy as np

from tests import waveform_candidates_restatement as wr

F32 = np.float32
NAN = float("nan")


def offsets(k0, kstep, nk):
    return [k0 + j * kstep for j in range(nk)]


def raw_of(rows, row_offset, wlens, S):
    """the call's `rows` [ngroup, K, row_stride] cut into raw[m] [ngroup, K, wlen_m + 2 S]"""
    return [np.ascontiguousarray(rows[:, :, o:o + n + 2 * S]) for o, n in zip(row_offset, wlens)]


def slot_misfits(raw, taper, ref, xf, method, dt, S, ks, syn_factor=1.0):
    """float32 [nk, ncand] of one slot of one group: raw [K, wlen + 2 S]"""
    sf, d64 = F32(syn_factor), np.float64(F32(dt))
    taper, ref = np.asarray(taper, F32), np.asarray(ref, F32)
    n = len(taper)
    out = np.zeros((len(ks), len(xf)), F32)
    with np.errstate(all="ignore"):
        u = wr.combine(raw, xf)                                # [ncand, wlen + 2 S], once for every offset
        for j, k in enumerate(ks):
            vt = (u[:, S - k:S - k + n] * taper[None, :]).astype(F32)
            a = np.broadcast_to(ref[None, :], vt.shape)
            d = (a - vt).astype(F32) if sf == F32(1) else ((F32(1) * a).astype(F32) - (sf * vt).astype(F32)).astype(F32)
            d = d.astype(np.float64)
            acc = wr._seq_sum(d * d) if method == 1 else wr._seq_sum(np.abs(d))
            out[j] = np.sqrt(d64 * acc).astype(F32) if method == 1 else (d64 * acc).astype(F32)
    return out


def slot_misfits_of(raw, taper, ref, x, method, dt, S, ks, syn_factor=1.0):
    """float32 [ngroup, nk, ncand, nmis]"""
    xf = np.atleast_2d(np.asarray(x, np.float64)).astype(F32)
    ngroup = raw[0].shape[0] if len(raw) else 0
    out = np.zeros((ngroup, len(ks), len(xf), len(raw)), F32)
    for m in range(len(raw)):
        for g in range(ngroup):
            out[g, :, :, m] = slot_misfits(raw[m][g], taper[m], ref[m], xf, method, dt, S, ks, syn_factor)
    return out


def first_minimum(v):
    """per row of v [n, nk]: (index, value) of the first smallest value, NaN passed over; (-1, NaN) where every value is NaN"""
    v = np.asarray(v, np.float64)
    bi, bv = np.full(len(v), -1, np.int32), np.full(len(v), NAN)
    for g, row in enumerate(v):
        if np.any(row == row):
            bi[g] = int(np.nanargmin(row))                     # (numpy: the first of equal values)
            bv[g] = row[bi[g]]
    return bi, bv


def fold_offsets(smis, norm, slot_receiver, w, anarchy, outer):
    """a dict of arrays as the call returns them from smis [ngroup, nk, ncand, nmis] and norm [ngroup, nmis]"""
    ngroup, nk, nc, nmis = smis.shape
    norm = np.asarray(norm, F32).reshape(ngroup, -1)
    misfit = np.full((ngroup, nk, nc), NAN)
    status = np.zeros(ngroup, np.int32)
    for g in range(ngroup):
        for j in range(nk):
            misfit[g, j], st = wr.fold(smis[g, j], norm[g], slot_receiver, w, anarchy, outer)
            if j == 0:
                status[g] = st
    bi, bv = wr.best_of(misfit.reshape(ngroup * nk, nc))
    bi, bv = bi.reshape(ngroup, nk), bv.reshape(ngroup, nk)
    best_offset, _ = first_minimum(bv)
    co, cm = first_minimum(np.moveaxis(misfit, 1, 2).reshape(ngroup * nc, nk))
    return dict(misfit=misfit, slot_misfit=smis, slot_norm=norm, status=status, best_index=bi, best_misfit=bv, best_offset=best_offset,
                cand_misfit=cm.reshape(ngroup, nc), cand_offset=co.reshape(ngroup, nc))


def evaluate(raw, taper, ref, norm, slot_receiver, w, anarchy, x, method, outer, dt, S, k0, kstep, nk, syn_factor=1.0, smis=None):
    """smis: `slot_misfits_of` of the same rows, candidates, method, factor and offsets, where several folds are made of them"""
    if smis is None:
        smis = slot_misfits_of(raw, taper, ref, x, method, dt, S, offsets(k0, kstep, nk), syn_factor)
    return fold_offsets(smis, norm, slot_receiver, w, anarchy, outer)
