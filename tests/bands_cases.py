"""Shared pieces of the misfit-band tests: the bands, the separate evaluations a band call is held against, the comparison
under the two arithmetic contracts, and -- run as a script -- one band call in a process of its own (for settings the library
reads from the environment when a context is made)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILTER = ([0.01, 0.03, 0.25, 0.4], [0., 1., 1., 0.])
TIME_DOMAIN = ["l2norm", "l1norm", "scalar_product", "peak"]
# every kind of band: four time-domain norms plain and filtered, two spectral norms plain and filtered
ALL_BANDS = ([(m, None, None) for m in TIME_DOMAIN] + [(m, FILTER[0], FILTER[1]) for m in TIME_DOMAIN] +
             [("ampspec_l2norm", None, None), ("ampspec_l1norm", None, None),
              ("ampspec_l2norm", FILTER[0], FILTER[1]), ("ampspec_l1norm", FILTER[0], FILTER[1])])
COMPS = ["d", "ne", "ned", "ned", "ne", "d"]


def separate(p, bands, isrc0=0, nsrc=None, ntrans=None):
    """what the parent commit offers: per band install its filter and method, evaluate, read the misfits.  Returns
    (misfit[n, nband, nmis], norm[...], global[n, nband]); leaves the context without filter under l2norm.  ntrans: a set that
    collects the transform lengths of receiver 1's first component seen on the way (get_amp_spectrum's n)."""
    ms, ns, gs = [], [], []
    for name, fx, fy in bands:
        p.set_misfit_filter(0, [] if fx is None else fx, [] if fx is None else fy)
        p.set_misfit_method(name)
        p.eval(isrc0, nsrc)
        m, n, g = p.get_misfits(isrc0, nsrc)
        if ntrans is not None and name.startswith("ampspec"):
            for s in range(isrc0, isrc0 + len(m)):
                ntrans.add(2 * (len(p.get_amp_spectrum(1, 1, isrc=s)[1]) - 1))
        ms.append(m); ns.append(n); gs.append(g)
    p.set_misfit_filter(0, [], [])
    p.set_misfit_method("l2norm")
    return np.stack(ms, 1), np.stack(ns, 1), np.stack(gs, 1)


def assert_bands_equal(got, want, what=""):
    """band call against separate evaluations (or another route of the band call).  exact contract: the same bits.  fused: the
    two calls evaluate batches of different shape (the band call keeps the synthetics), a different instantiation of the
    accumulate kernel may have made them, and then the tolerance include/kiwi_hip.h states for KIWI_ARITH_FUSED holds: 1e-6 of
    max(misfit, norm factor); for the global misfit g = |m| / |n| that is 1e-6 sqrt(g^2 + 1) (tests/common.py misfit_close).
    The norm factors come from the references alone: the same bits under both."""
    from tests import common
    (m, n, g), (m0, n0, g0) = got, want
    assert m.shape == m0.shape and g.shape == g0.shape, what
    assert np.array_equal(n, n0), (what, "norm factors")
    if common.arith() == "exact":
        for name, a, b in (("misfit", m, m0), ("global", g, g0)):
            if not np.array_equal(a, b):
                bad = np.argwhere(a != b)
                print(what, name, "differs at", bad[:6], a[tuple(bad[0])], b[tuple(bad[0])])
            assert np.array_equal(a, b), (what, name)
        return
    if np.array_equal(m, m0) and np.array_equal(g, g0):
        return
    print("%s: fused contract, the two calls' synthetics differ in bits: tolerance 1e-6 of max(misfit, norm factor) applied" % what)
    m64, n64, g64 = m0.astype(np.float64), n0.astype(np.float64), g0.astype(np.float64)
    assert np.all(np.abs(m - m64) <= 1e-6 * np.maximum(np.abs(m64), np.abs(n64))), (what, "misfit")
    assert np.all(np.abs(g - g64) <= 1e-6 * np.sqrt(g64 * g64 + 1.0)), (what, "global")


def trial_list(n=8):
    """`bilateral` sources with a rise time of 2 s: a fold of five taps at the database's 0.5 s"""
    from kiwi_amd import synthetic
    return synthetic.bilat_strike_sweep(n, step=1.5)


def no_rise_list(n=8):
    """`moment_tensor` sources WITHOUT a rise time, every one its own time, place and tensor: a plain evaluation of such a batch
    under an unfiltered time-domain method compares inside the accumulate kernel"""
    rng = np.random.default_rng(77)
    rows = np.zeros((n, 11), np.float32)
    rows[:, 0] = rng.uniform(-5., 5., n)
    rows[:, 1:3] = rng.uniform(-3000., 3000., (n, 2))
    rows[:, 3] = rng.uniform(8000., 12000., n)
    rows[:, 4:10] = rng.standard_normal((n, 6)) * 1e18
    return rows


TD_BANDS = ALL_BANDS[:4]


def main(out, nsrc, which="all", sources="bilateral", with_separate=False):
    """one band call of the standard scenario in this process -> npz (or the refusal's message); with_separate: the separate
    evaluations of the same context beside it"""
    from kiwi_amd.lib import KiwiHipError
    from tests.test_linfit_gpu import build
    sc, p = build(COMPS, planted=False)
    try:
        p.switch_receiver(6, False)
        bands = TD_BANDS if which == "td" else ALL_BANDS
        if sources == "norise":
            p.set_source_params("moment_tensor", no_rise_list(nsrc))
        else:
            p.set_source_params("bilateral", trial_list(nsrc))
        p.set_misfit_bands(bands)
        try:
            m, n, g = p.band_misfits()
            extra = {}
            launches = np.array(p.kernel_ms()[1])
            if with_separate:
                sm, sn, sg = separate(p, bands)
                extra = dict(sep_misfit=sm, sep_norm=sn, sep_glob=sg)
            np.savez(out, misfit=m, norm=n, glob=g, launches=launches, error="", **extra)
        except KiwiHipError as e:
            np.savez(out, error=str(e))
    finally:
        p.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), *(sys.argv[3:5]), with_separate=len(sys.argv) > 5 and sys.argv[5] == "1")
