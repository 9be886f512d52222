"""Inputs shared by tests/test_outer_bootstrap.py and tests/test_outer_bootstrap_gpu.py: random [N_s, N_r, N_k] misfit
and norm arrays as make_misfits_for_sources returns them (float64 holding float32 values, unused component columns zero),
the option matrix of the outer misfit, and the bound between the device's arithmetic and the host path's."""
import itertools

import numpy as np

from kiwi_amd.engine import bootstrap_draw_weights

# |g_device - g_host| <= (N_r + 16) 2^-52 g_host.  The accounting: all summands are non-negative, so no operation loses more
# than its own rounding, relatively.  Per source and draw both paths form M rw c (two products each; the host takes sqrt(c)
# first and squares afterwards under l2norm -- the sqrt(c) reordering --, the device squares and multiplies by c), add N_r
# such terms (the device from zero, r ascending; numpy blockwise), divide and, under l2norm, take a root.  Charging one
# rounding (2^-53 per path, 2^-52 for the pair) to each of the N_r additions and to each of the up to 16 other operations
# of the chain (products of the prepare, the weight, its root and squares, the draw products, quotient, root) gives the
# constant.  Under l2norm the final root halves what the sums carried and the bound is strict; under l1norm the errors of
# numerator and denominator could in the worst case all point apart and reach (2 N_r + 5) 2^-52, which no rounding pattern
# met in practice comes near (3000 sources x 50 receivers over eight decades: 5.6 2^-52 at worst).  The bound is kept as
# stated, not widened.
def ulp_bound(nrec):
    return (nrec + 16) * 2.0 ** -52


def make_case(ns, ncomponents, seed, failing=(), decades=8.0):
    """misfits_by_src, norms_by_src [ns, N_r, max N_k]: magnitudes spread over `decades` decades per receiver, misfits
    around 0.1 .. 2 norms; the sources listed in `failing` keep zero misfits AND zero norms (gridsearch.py compute)."""
    rng = np.random.default_rng(seed)
    nrec = len(ncomponents)
    kmax = max(list(ncomponents) + [1])
    scale = 10.0 ** rng.uniform(-decades / 2, decades / 2, (1, nrec, 1))
    nor = (scale * rng.uniform(0.5, 1.5, (1, nrec, kmax))).astype(np.float32).astype(np.float64)
    nor = np.repeat(nor, ns, 0)
    mis = (nor * rng.uniform(0.1, 2.0, (ns, nrec, kmax))).astype(np.float32).astype(np.float64)
    for r, k in enumerate(ncomponents):
        mis[:, r, k:] = 0.0
        nor[:, r, k:] = 0.0
    for s in failing:
        mis[s] = 0.0
        nor[s] = 0.0
    return mis, nor


def weights_with_a_zero(nrec, seed):
    w = np.random.default_rng(seed).uniform(0.25, 4.0, nrec)
    w[nrec // 2] = 0.0
    return w


def mask_with_gaps(nrec):
    m = np.ones(nrec, bool)
    m[::7] = False
    if not m.any():
        m[0] = True
    return m


# outer norm x anarchy x receiver weights (None, or one of them zero) x receiver mask (None, or some receivers off)
OPTIONS = list(itertools.product(("l1norm", "l2norm"), (False, True), (False, True), (False, True)))


def option_id(o):
    return "%s-%s-%s-%s" % (o[0], "anarchy" if o[1] else "plain", "weights" if o[2] else "ones", "mask" if o[3] else "all")


def draws_for(nrec, ndraw, seed, weighted, masked):
    """(receiver_weights or None, receiver_mask or None, draw_weights[ndraw, nrec]) of one option."""
    w = weights_with_a_zero(nrec, seed + 1) if weighted and nrec > 1 else None
    mask = mask_with_gaps(nrec) if masked and nrec > 1 else None
    return w, mask, bootstrap_draw_weights(nrec, ndraw, np.random.default_rng(seed), mask, w)
