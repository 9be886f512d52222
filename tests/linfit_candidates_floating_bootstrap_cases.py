"""Shared pieces of the GPU tests of kiwi_hip_linear_fit_candidates_floating_bootstrap: the host route that DEFINES the call
(`linear_fit_candidates_floating(..., cand_shift=True, receiver_misfit=True)`, then `Engine.outer_misfits` on ngroup x ncand
"sources" of one slot per receiver, once for all groups and once per group; the winner's row of cand_shift), the comparison, and
the six-receiver set-up with its shift ranges.  Not a test module."""
import numpy as np

from tests import linfit_candidates_floating_bootstrap_restatement as fbr
from tests.linfit_candidates_bootstrap_cases import draw_rows  # noqa: F401  (the draw rows are the sibling's)
from tests.linfit_candidates_floating_cases import RANGES_A, RANGES_B, set_ranges  # noqa: F401

FIELDS = ("best_value", "best_group", "best_cand", "best_shift", "status", "group_value", "group_cand", "group_shift")
DRAW_AXIS = dict(best_value=0, best_group=0, best_cand=0, best_shift=0, group_value=1, group_cand=1, group_shift=1)
WEIGHTS = np.array([1.0, 0.0, 2.5, 0.7, 1.3, 4.0])           # a zero weight; the weight of the disabled receiver never counts
COUNTED, SKIPPED = [0, 2, 4], [3, 5]                          # with WEIGHTS receiver 2 (index 1) is skipped too


def standard_with_skipped_receivers():
    """tests/test_linfit_candidates_floating_gpu.py's six receivers of 1 to 5 components: receiver 6 disabled, receiver 4 with
    references of zeros; WEIGHTS gives receiver 2 the weight 0.  (scenario, engine), the method still l2norm"""
    from tests.test_linfit_candidates_gpu import zero_reference
    from tests.test_linfit_gpu import COMPS, build
    sc, p = build(COMPS)
    p.switch_receiver(6, False)
    zero_reference(p, sc, 4)
    return sc, p


def floating(p, sc, ranges):
    p.set_misfit_method("floating_l2norm")
    set_ranges(p, sc.gf["dt"], ranges)


def host_route(p, isrc0, ngroup, K, cand, dw, outer_norm, receiver_weights, anarchy):
    """what the library offered before: the parent call's float arrays and shifts downloaded, then kiwi_hip_outer_misfits on them,
    for all groups at once and per group (tests/linfit_candidates_floating_bootstrap_restatement.py from_scan's dict)"""
    scan = p.linear_fit_candidates_floating(isrc0, ngroup, K, cand, outer_norm=outer_norm, receiver_weights=receiver_weights, anarchy=anarchy,
                                            misfit=True, cand_shift=True, receiver_misfit=True)
    nrec = scan.receiver_norm.shape[1]

    def outer(mis, nor, slots, nrec_, norm, w, an, draws):
        return p.outer_misfits(mis[:, :, None], nor[:, :, None], outer_norm=norm, receiver_weights=w, anarchy=an, draw_weights=draws,
                               ncomponents=[1] * nrec)
    return fbr.from_scan(scan.receiver_misfit, scan.receiver_norm, scan.cand_shift, scan.status, dw, outer_norm, receiver_weights, anarchy,
                         outer=outer)


def assert_boot(got, want, what, ndraw=None, slack=None, same_batch=False):
    """a CandidateFloatingBootstrap against the dict of the host route or of the restatement, the first `ndraw` draws of it (a draw
    does not depend on the others).  exact contract: the same bits in every array the call made.  fused: the two sides' synthetics
    may come from different instantiations of the accumulate kernel; the statuses agree, and where `slack` is given the values
    within it.  same_batch: both sides come from the same evaluation of the same uploaded batch on one context -- the same
    synthetics, hence the same bits under either contract"""
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
            b = np.take(b, np.arange(nd), axis=DRAW_AXIS[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        same = np.array_equal(a, b, equal_nan=a.dtype != np.int32)
        if not same:
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            print(what, name, "differs at", bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
        assert same, (what, name)
