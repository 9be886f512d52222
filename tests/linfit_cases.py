"""Shared inputs of tests/test_linfit.py (CPU, oracle traces) and tests/test_linfit_gpu.py (device traces): the traces of
groups of basis sources per misfit slot, in the layout tests/linfit_restatement.py takes.  Not a test module."""
import numpy as np

from kiwi_amd import mtfit, synthetic

UNIT = 1e18
LOCATION = [0., 0., 0., 10000.]
# a full tensor (not a double couple, not trace-free) with every component of the same order, so that a relative bound per
# component means something for each of them; N m
PLANTED = np.array([4.1e18, -2.3e18, 7.7e18, 3.5e18, -2.9e18, 5.2e18], np.float32)


def mt_row(tensor, location=LOCATION, risetime=1.0):
    return np.array(list(location) + list(tensor) + [risetime], np.float32)


def receivers_of(comps, enabled=None):
    """slot lists per receiver (enabled receivers, receiver-major), [] for disabled ones"""
    out, m = [], 0
    for ir, c in enumerate(comps):
        if (enabled is not None and not enabled[ir]) or len(c) == 0:
            out.append([])
            continue
        out.append(list(range(m, m + len(c))))
        m += len(c)
    return out


def oracle_traces(e, comps, sourcetype, rows, K):
    """tapered synthetics (ko.Engine.synthetic(..., 2)) of the sources `rows` [ngroup * K, nparams] and tapered references
    of an oracle engine whose every receiver is enabled: (syn[slot] [ngroup, K, wlen], ref[slot] [wlen], receivers)"""
    rows = np.atleast_2d(rows)
    ngroup = len(rows) // K
    syn, ref = None, []
    for ir, c in enumerate(comps):
        for k in range(len(c)):
            ref.append(e.reference(ir + 1, k + 1, 2)[1])
    for i, p in enumerate(rows):
        e.set_source_params(sourcetype, p)
        e.get_misfits()
        m = 0
        if syn is None:
            syn = [np.zeros((ngroup, K, len(r)), np.float32) for r in ref]
        for ir, c in enumerate(comps):
            for k in range(len(c)):
                lo, d = e.synthetic(ir + 1, k + 1, 2)
                assert len(d) == len(ref[m]), "a tapered synthetic spans the taper, like the tapered reference"
                syn[m][i // K, i % K] = d
                m += 1
    return syn, ref, receivers_of(comps)


def device_traces(p, comps, enabled, isrc0, ngroup, K, which=2):
    """the same from the product engine's own kept traces (get_synthetics(which), get_reference(which)) of the uploaded
    sources [isrc0, isrc0 + ngroup K)"""
    syn, ref = [], []
    for ir, c in enumerate(comps):
        if not enabled[ir]:
            continue
        for k in range(len(c)):
            r = p.get_reference(ir + 1, k + 1, which, maxn=1 << 14)[1]
            ref.append(r)
            a = np.zeros((ngroup, K, len(r)), np.float32)
            for i in range(ngroup * K):
                a[i // K, i % K] = p.get_synthetics(isrc0 + i, ir + 1, k + 1, which, maxn=1 << 14)[1]
            syn.append(a)
    return syn, ref, receivers_of(comps, enabled)


def slots_as_receivers(receivers):
    """every slot a receiver of its own: per-slot sums from gram_by_receiver"""
    return [[m] for sl in receivers for m in sl]


def basis_rows(sourcetype, row):
    return mtfit.elementary_params(sourcetype, np.atleast_2d(row), UNIT)
