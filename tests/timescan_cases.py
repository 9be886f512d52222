"""Shared pieces of the time-scan tests: the sources, the separate evaluations a scan is held against (the source moved, or the
references and tapers moved the other way), the comparison under the two arithmetic contracts, and -- run as a script -- named
cases in a process of its own (for settings the library reads from the environment when a context is made).  Not a test module."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COMPS = ["d", "ne", "ned", "ned", "ne", "d"]
FILTER = ([0.01, 0.03, 0.25, 0.4], [0., 1., 1., 0.])
TIME_DOMAIN = ["l2norm", "l1norm", "scalar_product", "peak"]
METHODS = ["l2norm", "l1norm", "ampspec_l2norm", "ampspec_l1norm", "scalar_product", "peak"]
FILTERS = ["none", "all", "receiver2"]
OFFSETS = (-7, 3, 6)                                      # k0, kstep, nk: -7, -4, -1, 2, 5, 8
WINDOW = 150
PER_PASS = 4                                              # offsets per pass of time_scan_kernel (kiwi_timescan.hpp kPerPass)


def offsets(k0, kstep, nk):
    return [k0 + j * kstep for j in range(nk)]


def exact_mt_rows(n=8):
    """`moment_tensor` sources without a rise-time fold whose times are multiples of 0.25 s.  (A `moment_tensor` row's own
    rise-time parameter is discretised into centroids, never folded; 0.5 s gives two centroids at time -+ 0.125 s, and 0 would
    be a source without moment.)  Every centroid's time / dt is exact in fp32 at the scenario's dt = 0.5 s, and so is every
    time + k dt"""
    rng = np.random.default_rng(41)
    rows = np.zeros((n, 11), np.float32)
    rows[:, 0] = rng.integers(-12, 13, n) * 0.25
    rows[0, 0] = 1.25
    rows[:, 1:3] = rng.uniform(-3000., 3000., (n, 2))
    rows[:, 3] = rng.uniform(8000., 12000., n)
    rows[:, 4:10] = rng.standard_normal((n, 6)) * 1e18
    rows[:, 10] = 0.5
    return rows


def dyadic_tables(n=6, ncent=4, seed=43):
    """explicit centroid tables (north, east, depth, time, six tensor components) with dyadic times"""
    rng = np.random.default_rng(seed)
    tabs = []
    for _ in range(n):
        t = np.zeros((ncent, 10), np.float32)
        t[:, 0:2] = rng.uniform(-3000., 3000., (ncent, 2))
        t[:, 2] = rng.uniform(8000., 12000., ncent)
        t[:, 3] = rng.integers(-16, 17, ncent) * 0.125 + rng.integers(-4, 5) * 0.5
        t[:, 4:10] = rng.standard_normal((ncent, 6)) * 1e18 / ncent
        tabs.append(t)
    return tabs


def moved(tables, seconds):
    out = []
    for t in tables:
        t = t.copy()
        t[:, 3] += np.float32(seconds)
        out.append(t)
    return out


def set_filters(p, which):
    p.set_misfit_filter(0, [], [])
    if which == "all":
        p.set_misfit_filter(0, *FILTER)
    elif which == "receiver2":
        p.set_misfit_filter(2, *FILTER)


def separate_params(p, sourcetype, rows, ks, dt):
    """what the parent commit offers: per offset the sources with their times moved by k dt, evaluated and read.  Returns
    (misfit[n, nk, nmis], norm[n, nmis], global[n, nk])"""
    ms, gs, n0 = [], [], None
    for k in ks:
        r = np.array(rows, np.float32, copy=True)
        r[:, 0] += np.float32(k * dt)
        p.set_source_params(sourcetype, r)
        p.eval()
        m, n, g = p.get_misfits()
        assert n0 is None or np.array_equal(n, n0), "the norm factors do not depend on the source"
        n0 = n
        ms.append(m); gs.append(g)
    return np.stack(ms, 1), n0, np.stack(gs, 1)


def separate_tables(p, tables, moments, rises, ks, dt):
    ms, gs, n0 = [], [], None
    for k in ks:
        p.set_sources(moved(tables, k * dt), moments, rises)
        p.eval()
        m, n, g = p.get_misfits()
        n0 = n
        ms.append(m); gs.append(g)
    return np.stack(ms, 1), n0, np.stack(gs, 1)


def assert_scan_equal(got, want, what=""):
    """scan against separate evaluations (or another route of the scan): (misfit[n, nk, nmis], norm[n, nmis], global[n, nk]).
    exact contract: the same bits.  fused: the two calls evaluate batches of different shape and row length, a different
    instantiation of the accumulate kernel may have made them, and then the tolerance include/kiwi_hip.h states for
    KIWI_ARITH_FUSED holds: 1e-6 of max(misfit, norm factor); for the global misfit 1e-6 sqrt(g^2 + 1) (tests/common.py
    misfit_close).  The norm factors come from the references alone: the same bits under both."""
    from tests import common
    (m, n, g), (m0, n0, g0) = got[:3], want[:3]
    assert m.shape == m0.shape and g.shape == g0.shape and n.shape == n0.shape, (what, m.shape, m0.shape)
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
    assert_scan_close(got, want, what)


def assert_scan_close(got, want, what=""):
    """the header's bound for an unfiltered time-domain method compared inside the accumulate kernel by the plain evaluation"""
    (m, n, g), (m0, n0, g0) = got[:3], want[:3]
    assert np.array_equal(n, n0), (what, "norm factors")
    m64, n64, g64 = m0.astype(np.float64), n0.astype(np.float64)[:, None, :], g0.astype(np.float64)
    assert np.all(np.abs(m - m64) <= 1e-6 * np.maximum(np.abs(m64), np.abs(n64))), (what, "misfit")
    assert np.all(np.abs(g - g64) <= 1e-6 * np.sqrt(g64 * g64 + 1.0)), (what, "global")


def first_argmin(g):
    return np.array([int(np.argmin(row)) for row in g], np.int32)


def standard(window=WINDOW):
    from tests.test_linfit_gpu import build
    sc, p = build(COMPS, planted=False, window=window)
    p.switch_receiver(6, False)
    return sc, p


def grid(sc):
    from kiwi_amd import gridsearch
    from tests.linfit_cases import PLANTED, mt_row
    base = mt_row(PLANTED, risetime=0.5)                      # two centroids at -+ 0.125 s: exact, see exact_mt_rows
    return gridsearch.MisfitGrid("moment_tensor", base, param_values=[("depth", [9000., 10000., 11000.]),
                                                                      ("time", [-1.0, -0.5, 0.0, 0.5, 1.0])])


# ---------------------------------------------------------------------------------------------- cases of the child process
def case_methods(z):
    """every method, with and without filter, exact sources: scan and separate evaluations on the same context"""
    sc, p = standard()
    try:
        dt = sc.gf["dt"]
        rows = exact_mt_rows(8)
        ks = offsets(*OFFSETS)
        for method in METHODS:
            for filt in FILTERS:
                set_filters(p, filt)
                p.set_misfit_method(method)
                p.set_source_params("moment_tensor", rows)
                m, n, g, b = p.time_scan(0, None, *OFFSETS)
                sm, sn, sg = separate_params(p, "moment_tensor", rows, ks, dt)
                key = "methods_%s_%s_" % (method, filt)
                z.update({key + "m": m, key + "n": n, key + "g": g, key + "b": b, key + "sm": sm, key + "sn": sn, key + "sg": sg})
    finally:
        p.close()


def fold_batch():
    tabs = dyadic_tables(6)
    moments = np.array([1.0, 0.5, 2.0, 1.0, 1.5, 0.25], np.float32)
    rises = np.array([0.0, 1.0, 2.0, 0.0, 2.0, 1.0], np.float32)
    return tabs, moments, rises


def case_fold(z):
    """rise times 0, 1 and 2 s mixed in one batch of explicit centroid tables"""
    sc, p = standard()
    try:
        dt = sc.gf["dt"]
        tabs, moments, rises = fold_batch()
        ks = offsets(*OFFSETS)
        for method in ("l2norm", "ampspec_l1norm"):
            p.set_misfit_method(method)
            p.set_sources(tabs, moments, rises)
            m, n, g, b = p.time_scan(0, None, *OFFSETS)
            sm, sn, sg = separate_tables(p, tabs, moments, rises, ks, dt)
            key = "fold_%s_" % method
            z.update({key + "m": m, key + "n": n, key + "g": g, key + "b": b, key + "sm": sm, key + "sn": sn, key + "sg": sg})
    finally:
        p.close()


def case_grid(z):
    sc, p = standard()
    try:
        a, b = grid(sc), grid(sc)
        a.compute(p)
        b.compute(p, time_scan=True)
        z.update(grid_m=a.misfits_by_src, grid_n=a.norms_by_src, grid_sm=b.misfits_by_src, grid_sn=b.norms_by_src)
    finally:
        p.close()


def routing_sources():
    from tests.bands_cases import trial_list
    tr = trial_list(16)
    dup = np.tile(tr[:1], (8, 1))
    dup[:, 4] *= np.linspace(0.5, 2.0, 8).astype(np.float32)          # one centroid table, eight moments
    return tr, dup


def case_routing(z):
    """the scan of two batches as this process's environment routes it (chunks, shared synthetics)"""
    sc, p = standard()
    try:
        tr, dup = routing_sources()
        for name, rows in (("list", tr), ("dup", dup)):
            p.set_source_params("bilateral", rows)
            m, n, g, b = p.time_scan(0, None, *OFFSETS)
            z.update({"routing_%s_m" % name: m, "routing_%s_n" % name: n, "routing_%s_g" % name: g, "routing_%s_b" % name: b,
                      "routing_%s_launches" % name: np.array(p.kernel_ms()[1])})
    finally:
        p.close()


def case_nofused(z):
    """KIWI_HIP_FUSED_FFT=0: a filtered slot is refused, an unfiltered time-domain method is served"""
    from kiwi_amd.lib import KiwiHipError
    sc, p = standard()
    try:
        dt = sc.gf["dt"]
        tabs, moments, rises = fold_batch()
        p.set_sources(tabs, moments, rises)
        p.set_misfit_filter(2, *FILTER)
        try:
            p.time_scan(0, None, *OFFSETS)
            z["nofused_error"] = np.array("")
        except KiwiHipError as e:
            z["nofused_error"] = np.array(str(e))
        p.set_misfit_filter(0, [], [])
        p.set_sources(tabs, moments, rises)
        m, n, g, b = p.time_scan(0, None, *OFFSETS)
        sm, sn, sg = separate_tables(p, tabs, moments, rises, offsets(*OFFSETS), dt)
        z.update(nofused_m=m, nofused_n=n, nofused_g=g, nofused_sm=sm, nofused_sn=sn, nofused_sg=sg)
    finally:
        p.close()


def main(out, cases):
    z = {}
    for name in cases:
        globals()["case_" + name](z)
    np.savez(out, **z)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
