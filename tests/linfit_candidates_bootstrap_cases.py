"""Shared pieces of the GPU tests of kiwi_hip_linear_fit_candidates_bootstrap: the host route that DEFINES the call
(`linear_fit_candidates_time_scan(..., receiver_misfit=True)`, then `Engine.outer_misfits` on nk x ncand "sources" of one slot per
receiver, once for all groups and once per group), the comparison, the draw rows, and -- run as a script -- the packing case in a
process of its own (KIWI_HIP_CHUNK_MB is read when a context is made).  Not a test module."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("best_value", "best_group", "best_offset", "best_cand", "status", "group_value", "group_offset", "group_cand")
PACK_NCAND, PACK_NDRAW = 300, 40
PASS_GROUPS, PASS_SCAN, PASS_NDRAW = 2, (-2, 2, 3), 10000     # 3 offsets x 3 tiles x 10000 draws x 12 bytes: a slab above 1 MiB


def draw_rows(nrec, ndraw, counted, skipped, seed=0):
    """[ndraw, nrec]: row 0 all ones, row 1 all zeros, row 2 non-zero only on the `skipped` receivers, then resampling counts of
    the `counted` receivers from `bootstrap_draw_weights`"""
    from kiwi_amd.engine import bootstrap_draw_weights
    mask = np.zeros(nrec, bool)
    mask[list(counted)] = True
    dw = np.zeros((max(ndraw, 3), nrec))
    dw[0] = 1.0
    dw[2, list(skipped)] = 3.0
    dw[3:] = bootstrap_draw_weights(nrec, len(dw) - 3, np.random.default_rng(seed), receiver_mask=mask)
    return dw[:ndraw]


def host_route(p, isrc0, ngroup, K, cand, dw, k0, kstep, nk, outer_norm, receiver_weights, anarchy, scan=None):
    """what the library offered before: the candidate scan's float arrays downloaded, then kiwi_hip_outer_misfits on them, for all
    groups at once and per group (tests/linfit_candidates_bootstrap_restatement.py from_scan's dict)"""
    from tests import linfit_candidates_bootstrap_restatement as br
    if scan is None:
        scan = p.linear_fit_candidates_time_scan(isrc0, ngroup, K, cand, k0, kstep, nk, outer_norm=outer_norm, receiver_weights=receiver_weights,
                                                 anarchy=anarchy, marginal=False, receiver_misfit=True)
    nrec = scan.receiver_norm.shape[1]

    def outer(mis, nor, slots, nrec_, norm, w, an, draws):
        return p.outer_misfits(mis[:, :, None], nor[:, :, None], outer_norm=norm, receiver_weights=w, anarchy=an, draw_weights=draws,
                               ncomponents=[1] * nrec)
    return br.from_scan(scan.receiver_misfit, scan.receiver_norm, scan.status, dw, outer_norm, receiver_weights, anarchy, outer=outer)


def assert_boot(got, want, what, ndraw=None, slack=None, same_batch=False):
    """a CandidateBootstrap against the dict of the host route or of the restatement, the first `ndraw` draws of it (a draw does
    not depend on the others).  exact contract: the same bits in every array the call made.  fused: the two sides' synthetics may
    come from different instantiations of the accumulate kernel (tests/common.py same_bits); the statuses agree, and where `slack`
    is given (tests/linfit_candidates_timescan_cases.py slack_of's largest figure) the values within it.  same_batch: both sides
    come from the same evaluation of the same uploaded batch on one context -- the same synthetics, hence the same bits under
    either contract"""
    from tests import common
    assert np.array_equal(got.status, want["status"]), (what, "status", got.status, want["status"])
    nd = len(got.best_value) if ndraw is None else ndraw
    if common.arith() != "exact" and not same_batch:
        if slack is not None:
            with np.errstate(invalid="ignore"):
                a, b = got.best_value, want["best_value"][:nd]
                assert np.all((np.abs(a - b) <= slack) | ((a != a) & (b != b))), (what, "best_value")
        return
    for name in FIELDS:
        a, b = getattr(got, name), want[name]
        if a is None:
            continue
        if name != "status":
            b = b[..., :nd]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        same = np.array_equal(a, b, equal_nan=a.dtype != np.int32)
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
        assert same, (what, name)


def pack_candidates():
    return np.random.default_rng(10).uniform(-2.0, 2.0, (PACK_NCAND, 6))


def pack_draws(nrec):
    return draw_rows(nrec, PACK_NDRAW, range(5), [5], seed=3)


def pass_candidates(C):
    return np.random.default_rng(12).uniform(-2.0, 2.0, (2 * C + 3, 6))


def pass_rows():
    from tests.test_linfit_gpu import colocated_groups
    return colocated_groups(np.random.default_rng(13), PASS_GROUPS, 6)


def main(out):
    """the bootstrap of linfit_timescan_cases.chunk_rows() as this process's environment cuts it into chunks, and a case whose
    slab of ONE group exceeds the bound, so that the draws go in passes"""
    from tests import linfit_timescan_cases as lc
    sc, p = lc.standard()
    try:
        z = {}
        C = p.linear_fit_candidates_bootstrap_shape(6)[0]
        for norm in ("l1norm", "l2norm"):
            p.set_source_params("moment_tensor", lc.chunk_rows())
            p.kernel_ms()
            boot = p.linear_fit_candidates_bootstrap(0, lc.CHUNK_GROUPS, lc.CHUNK_K, pack_candidates(), pack_draws(sc.nrec), *lc.CHUNK_SCAN,
                                                     outer_norm=norm, anarchy=True, per_group=True)
            z.update({norm + "_" + name: getattr(boot, name) for name in boot._fields})
            z[norm + "_launches"] = np.array(p.kernel_ms()[1])
            p.set_source_params("moment_tensor", pass_rows())
            boot = p.linear_fit_candidates_bootstrap(0, PASS_GROUPS, 6, pass_candidates(C), draw_rows(sc.nrec, PASS_NDRAW, range(5), [5], seed=4),
                                                     *PASS_SCAN, outer_norm=norm, anarchy=True, per_group=True)
            z.update({norm + "_pass_" + name: getattr(boot, name) for name in boot._fields})
        np.savez(out, **z)
    finally:
        p.close()


if __name__ == "__main__":
    main(sys.argv[1])
