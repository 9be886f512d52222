"""Shared inputs of tests/test_linfit.py (CPU, oracle traces) and tests/test_linfit_gpu.py (device traces): the traces of
groups of basis sources per misfit slot, in the layout tests/linfit_restatement.py takes.  Not a test module."""
import os

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


def _is_empty(lo, d):
    """what ko.Engine.synthetic / reference hand out for a probe that holds nothing: one zero sample"""
    return len(d) == 0 or (len(d) == 1 and d[0] == 0.0)


class _Window:
    """A receiver's taper on the oracle's side: its samples [a, b] (discrete_plf_span) and the oracle's own tapering routine.
    ko.Engine.synthetic(..., 2) hands out the part of a tapered probe that has DATA; what a comparison sums is the probe over the
    whole taper -- zeros in front of the data, the LAST value held behind them (a static displacement stays: comparator.f90
    probe_set_array), times the taper.  The plain probes (which = 1) are extended that way here."""

    def __init__(self, x, y, dt):
        import ctypes as C
        from oracle import ko
        self.C, self.ko, self.dt = C, ko, dt
        self.plf = ko.make_plf(np.asarray(x, np.float32), np.asarray(y, np.float32))
        w = (C.c_int * 2)()
        ko.lib().ko_discrete_plf_span(C.byref(self.plf), dt, w)
        self.a, self.b = w[0], w[1]

    def taper(self, arr, lo, hi):
        """the oracle's routine on samples lo .. hi held in arr, in place (make_array_tapered)"""
        self.ko.lib().ko_plf_taper_array_r(self.C.byref(self.plf), arr.ctypes.data_as(self.ko.c_float_p), lo, hi, self.dt, 0)

    def weights(self):
        w = np.ones(self.b - self.a + 1, np.float32)
        self.taper(w, self.a, self.b)
        return w

    def extended(self, lo, d, S=0):
        """the plain probe (lo, d) over [a - S, b + S]: zeros in front of its data, its last value behind them"""
        a, b = self.a - S, self.b + S
        out = np.zeros(b - a + 1, np.float32)
        if not _is_empty(lo, d):
            i0, i1 = max(a, lo), min(b, lo + len(d) - 1)
            if i0 <= i1:
                out[i0 - a:i1 - a + 1] = d[i0 - lo:i1 - lo + 1]
            if lo + len(d) - 1 < b:
                out[max(lo + len(d) - a, 0):] = d[-1]
        return out

    def tapered(self, lo, d, check=None):
        """the tapered probe over [a, b] as the oracle's make_array_tapered makes it (from the first sample with data on);
        check: the oracle's own tapered samples (which = 2), which must be the same bits where it has them"""
        out = np.zeros(self.b - self.a + 1, np.float32)
        if _is_empty(lo, d):
            return out
        hi = max(self.b, lo + len(d) - 1)
        arr = np.full(hi - lo + 1, d[-1], np.float32)
        arr[:len(d)] = d
        self.taper(arr, lo, hi)
        i0, i1 = max(self.a, lo), min(self.b, hi)
        if i0 <= i1:
            out[i0 - self.a:i1 - self.a + 1] = arr[i0 - lo:i1 - lo + 1]
        if check is not None and not _is_empty(*check):
            clo, cd = check
            j0, j1 = max(self.a, clo), min(self.b, clo + len(cd) - 1)
            assert j0 > j1 or np.array_equal(out[j0 - self.a:j1 - self.a + 1], cd[j0 - clo:j1 - clo + 1]), (lo, len(d), self.a, self.b)
        return out


def _enabled_slots(comps, enabled):
    return [(ir, k) for ir, c in enumerate(comps) if enabled[ir] for k in range(len(c))]


def oracle_traces_padded(e, comps, enabled, tapers, dt, set_source, rows, K):
    """`oracle_traces` for set-ups in which a tapered trace need not span the taper: a slot that traces missing from the
    database left empty (one zero sample), windows that reach past the data, static end values (_Window).  tapers: {receiver
    (1-based): (x, y)}; `set_source(e, row)` makes `row` the oracle's source, whose synthetics factor is 1; `enabled`: per
    receiver, disabled ones get no slots (the layout of device_traces).  Returns (syn, ref, receivers, empty [nslot, ngroup, K]
    bool: the synthetics that were empty)."""
    t = oracle_rows_padded(e, comps, enabled, tapers, dt, set_source, rows, K, 0)
    return t["syn"], t["ref"], t["receivers"], t["empty"]


def oracle_rows_padded(e, comps, enabled, tapers, dt, set_source, rows, K, S):
    """oracle_traces_padded and, for the restatements that move a trace under the fixed taper (tests/linfit_timescan_restatement.py,
    the floating ones), the untapered rows: dict(syn, ref, receivers, empty as there; raw[slot] [ngroup, K, wlen + 2 S], the plain
    extended probes over the window made S samples wider on either side; rawref[slot] [wlen + 2 S], the references likewise;
    taper[slot] [wlen], the routine's weights)"""
    rows = np.atleast_2d(rows)
    ngroup = len(rows) // K
    slots = _enabled_slots(comps, enabled)
    win = {ir: _Window(*tapers[ir + 1], dt) for ir in {ir for ir, _ in slots}}
    ref = [win[ir].tapered(*e.reference(ir + 1, k + 1, 1), check=e.reference(ir + 1, k + 1, 2)) for ir, k in slots]
    rawref = [win[ir].extended(*e.reference(ir + 1, k + 1, 1), S=S) for ir, k in slots]
    taper = [win[ir].weights() for ir, k in slots]
    syn = [np.zeros((ngroup, K, len(r)), np.float32) for r in ref]
    raw = [np.zeros((ngroup, K, len(r) + 2 * S), np.float32) for r in ref]
    empty = np.zeros((len(slots), ngroup, K), bool)
    for i, p in enumerate(rows):
        set_source(e, p)
        e.get_misfits()
        for m, (ir, k) in enumerate(slots):
            plain = e.synthetic(ir + 1, k + 1, 1)
            empty[m, i // K, i % K] = _is_empty(*plain)
            syn[m][i // K, i % K] = win[ir].tapered(*plain, check=e.synthetic(ir + 1, k + 1, 2))
            raw[m][i // K, i % K] = win[ir].extended(*plain, S=S)
    for m in range(len(slots)):                                 # (unmoved, the rows times the weights are the tapered traces)
        n = len(taper[m])
        assert np.array_equal((raw[m][:, :, S:S + n] * taper[m]).astype(np.float32), syn[m]), m
        assert np.array_equal((rawref[m][S:S + n] * taper[m]).astype(np.float32), ref[m]), m
    return dict(syn=syn, ref=ref, receivers=receivers_of(comps, enabled), empty=empty, raw=raw, rawref=rawref, taper=taper)


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


def eikonal_list_with_a_failed_piece(p, unit=2):
    """For engine p: three groups of `unit` `mt_eikonal` sources, every source of the middle group failing to discretise ("Empty
    rupture area": above the constraining planes).  In pieces of `unit` sources nothing is uploaded for the middle piece.
    Returns (the list, the list without the middle group)."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eikonal_vectors.npz"))
    p.set_source_crust(G["rupture_profile"], G["origin_profile"])
    p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
    eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (3 * unit, 1))
    eik[:, 13:19] = np.random.default_rng(6).standard_normal((3 * unit, 6)) * 1e18
    eik[unit:2 * unit, 3] = 500.0
    return eik, np.concatenate([eik[:unit], eik[2 * unit:]])


def assert_beside_a_failed_piece(got, alone, arith, what=""):
    """the arrays of `got` -- three groups (or sources), the middle one failed -- at groups 0 and 2 against `alone`, the same call on
    the list without the middle group, cut into the same pieces: the plain call's values on the same sources, bit for bit under the
    exact contract and rtol = 1e-3 under fused"""
    for i, (a, b) in enumerate(zip(got, alone)):
        if not isinstance(a, np.ndarray) or a.ndim == 0 or len(a) != 3:
            continue
        a = a[[0, 2]]
        assert a.shape == b.shape, (what, i)
        if arith == "exact" or a.dtype.kind in "iu":
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, i)
        else:
            np.testing.assert_allclose(a, b, rtol=1e-3, equal_nan=True, err_msg="%s %d" % (what, i))
