"""Shared pieces of the tests of kiwi_hip_linear_fit_time_scan: basis sources as explicit centroid tables with fractional times
and rise times, route B (the parent's kiwi_hip_linear_fit with references and tapers moved by -k samples), the flattening of a
scan into the shape tests/test_linfit_gpu.py assert_same_fit takes, and -- run as a script -- a case in a process of its own
(KIWI_HIP_CHUNK_MB is read when a context is made).  Not a test module."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOW = 150
CHUNK_GROUPS, CHUNK_K, CHUNK_SCAN = 40, 6, (-7, 3, 6)


def scattered_tables(rng, ngroup, K):
    """tests/test_linfit_gpu.py scattered_groups as explicit centroid tables of two centroids each (fractional times, a sixth of a
    second apart), so that a rise time can be FOLDED on the device: (tables, moments, rise times 0, 1, 2 s in turn)"""
    from tests.test_linfit_gpu import scattered_groups
    rows = scattered_groups(rng, ngroup, K)
    tabs = []
    for r in rows:
        t = np.zeros((2, 10), np.float32)
        t[:, 0:3] = r[1:4]
        t[:, 3] = r[0] + np.array([-0.083, 0.083], np.float32)
        t[:, 4:10] = r[4:10] / 2
        tabs.append(t)
    n = len(rows)
    return tabs, np.linspace(0.5, 1.5, n).astype(np.float32), np.array([0.0, 1.0, 2.0] * n, np.float32)[:n]


def flat(fit):
    """a ScanFit [ngroup, nk, ...] as a LinearFit over ngroup x nk groups"""
    from kiwi_amd.engine import LinearFit
    n = fit.status.size
    return LinearFit(fit.coef.reshape(n, -1), fit.misfit.reshape(n), fit.status.reshape(n), fit.pivot_min.reshape(n),
                     None if fit.normal is None else fit.normal.reshape(n, -1), None)


def stacked(fits):
    """LinearFits [ngroup, ...] of nk separate calls as one LinearFit over ngroup x nk groups, offset running fastest"""
    from kiwi_amd.engine import LinearFit
    st = lambda name: np.stack([getattr(f, name) for f in fits], 1)          # noqa: E731
    n = fits[0].status.size * len(fits)
    return LinearFit(st("coef").reshape(n, -1), st("misfit").reshape(n), st("status").reshape(n), st("pivot_min").reshape(n),
                     st("normal").reshape(n, -1), None)


def route_b(p, sc, ks, call):
    """per offset k the references and the tapers moved by -k samples, then `call()` (the parent's linear_fit); everything is
    put back afterwards.  Returns the list of what the calls gave."""
    dt = sc.gf["dt"]
    out = []
    for k in ks:
        for ir in range(1, sc.nrec + 1):
            p.shift_ref_seismogram(ir, -k * dt)
            x, y = sc.tapers[ir]
            p.set_misfit_taper(ir, np.asarray(x, np.float32) - np.float32(k * dt), y)
        out.append(call())
        for ir in range(1, sc.nrec + 1):
            p.shift_ref_seismogram(ir, k * dt)
    for ir in range(1, sc.nrec + 1):
        p.set_misfit_taper(ir, *sc.tapers[ir])
    return out


def first_best(fit):
    """the first smallest misfit among the offsets with status 0 per group, -1 where there is none"""
    out = np.full(len(fit.status), -1, np.int32)
    for g in range(len(fit.status)):
        ok = np.nonzero(fit.status[g] == 0)[0]
        if len(ok):
            out[g] = ok[int(np.argmin(fit.misfit[g][ok]))]
    return out


def standard(window=WINDOW, planted=True, engine=None):
    from tests.test_linfit_gpu import COMPS, build
    sc, p = build(COMPS, planted=planted, window=window, engine=engine)
    p.switch_receiver(6, False)
    return sc, p


def chunk_rows():
    from tests.test_linfit_gpu import colocated_groups
    return colocated_groups(np.random.default_rng(8), CHUNK_GROUPS, CHUNK_K)


def main(out):
    """the scan of chunk_rows() as this process's environment cuts it into chunks"""
    sc, p = standard()
    try:
        p.set_source_params("moment_tensor", chunk_rows())
        p.kernel_ms()
        fit = p.linear_fit_time_scan(0, CHUNK_GROUPS, CHUNK_K, *CHUNK_SCAN, normal=True)
        np.savez(out, coef=fit.coef, misfit=fit.misfit, status=fit.status, pivot_min=fit.pivot_min, best=fit.best, normal=fit.normal,
                 launches=np.array(p.kernel_ms()[1]))
    finally:
        p.close()


if __name__ == "__main__":
    main(sys.argv[1])
