"""The arithmetic of kiwi_hip_waveform_candidates_floating (kiwi_amd/csrc/kiwi_waveform_candidates_floating.hpp) restated in numpy,
operation for operation and in the same order: the tapered, shifted references as floating_norm_kernel forms them, per shift the
slot misfits of tests/waveform_candidates_restatement.py (combination, residual, ascending fp64 sum), the fp32 sum over a
receiver's slots and its FIRST minimum as floating_select_kernel has them, and the per-slot outer fold.  The GPU tests feed it with
the device's own kept traces and ask for the same bits.  Not a test module.

Layout: syn[m] float32 [ngroup, K, wlen_m] (the kept rows, WITHOUT the synthetics factor); aq[m] float32 [ns_m, wlen_m], row q the
reference moved by lo + q and tapered (`shifted_references`; the slots of a receiver share ns); lo [nrec] the first shift of every
receiver's range; norm float32 [ngroup, nmis]; slot_receiver[m] (ascending); w [nrec] float64 (0 for a disabled receiver).  method 1
l2 inside (floating_l2norm), 2 l1 inside (floating_l1norm)."""
import numpy as np

from tests import waveform_candidates_restatement as wr

F32 = np.float32


def shifted_references(refx, tw, ns):
    """[ns, wlen] float32: a_q[i] = refx[i + (ns - 1 - q)] * tw[i], one fp32 product; refx is the un-tapered reference over
    [w0 - hi, w0 + wlen - 1 - lo], wlen + ns - 1 samples"""
    refx, tw = np.asarray(refx, F32), np.asarray(tw, F32)
    assert len(refx) == len(tw) + ns - 1
    return np.stack([(refx[ns - 1 - q:ns - 1 - q + len(tw)] * tw).astype(F32) for q in range(ns)])


def slot_misfits_per_shift(rows, aq, x, method, dt, syn_factor=1.0):
    """float32 [ncand, ns] of one slot: m_kq, one accumulator per shift"""
    return np.stack([wr.slot_misfits(rows, a, x, method, dt, syn_factor) for a in aq], 1)


def select(mkq, method):
    """q* [ncand] and m_{k, q*} [ncand, ncomp] of one receiver from mkq [ncomp][ncand, ns]: sum_q = 0.f; sum_q = sum_q + (m | m m),
    k ascending, fp32; the first minimum: q == 0 || sum_q < best"""
    with np.errstate(all="ignore"):
        total = np.zeros(mkq[0].shape, F32)
        for m in mkq:
            total = (total + (m if method == 2 else (m * m).astype(F32))).astype(F32)
        best, q = total[:, 0].copy(), np.zeros(len(total), np.int64)
        for j in range(1, total.shape[1]):
            take = total[:, j] < best
            best, q = np.where(take, total[:, j], best), np.where(take, j, q)
    return q, np.stack([m[np.arange(len(q)), q] for m in mkq], 1)


def receiver_minimum(mkq, method):
    """float64 [ncand]: min_q of sum_k m_kq (l1 inside) or of sqrt(sum_k m_kq^2) (l2 inside), in fp64 -- what the tests compare
    with another evaluation's, 1-Lipschitz in the per-shift values"""
    m = np.stack(mkq).astype(np.float64)
    return np.min(m.sum(0) if method == 2 else np.sqrt((m * m).sum(0)), axis=1)


def evaluate(syn, aq, lo, norm, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor=1.0, mkq=None):
    """a dict of arrays as the call returns them.  mkq: [ngroup][nmis] of `slot_misfits_per_shift` of the same traces, candidates,
    method and factor, where several folds are made of them"""
    ngroup, nmis, nrec = (syn[0].shape[0] if len(syn) else 0), len(syn), len(w)
    x = np.atleast_2d(np.asarray(x, np.float64))
    if mkq is None:
        mkq = [[slot_misfits_per_shift(syn[m][g], aq[m], x, method, dt, syn_factor) for m in range(nmis)] for g in range(ngroup)]
    smis = np.zeros((ngroup, len(x), nmis), F32)
    cshift = np.zeros((ngroup, len(x), nrec), np.int16)
    for g in range(ngroup):
        for r in sorted(set(slot_receiver)):
            slots = [m for m in range(nmis) if slot_receiver[m] == r]
            q, mk = select([mkq[g][m][:len(x)] for m in slots], method)
            smis[g][:, slots] = mk
            cshift[g, :, r] = lo[r] + q
    out = wr.evaluate(syn, None, norm, slot_receiver, w, anarchy, x, method, outer, dt, syn_factor, smis=smis)
    bi = out["best_index"]
    out["cand_shift"] = cshift
    out["best_shift"] = np.stack([cshift[g, bi[g]].astype(np.int32) if bi[g] >= 0 else np.zeros(nrec, np.int32) for g in range(ngroup)]) \
        if ngroup else np.zeros((0, nrec), np.int32)
    return out
