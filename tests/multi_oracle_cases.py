"""Fixtures of the oracle parity of accumulate_multi_kernel (tests/test_multi_oracle_cases.py checks them on the CPU,
tests/test_gpu_multi_oracle.py runs them on the device).

Everything sits on the database of tests/test_gpu_multi_plan.py -- 16 x 5 nodes 4000 m x 2000 m apart, 1100 samples of 0.5 s, the
`probe` variant: two 512-sample tiles of a pair, five 256-sample tiles of a group of four, the last one partial -- with three
receivers `ned`, `ard`, `swu` (the multi kernel takes receivers with horizontal and vertical components only; together the three
use every rotation and both signs of out4).

A trial source is a centroid table cut from the discretised bilateral source synthetic.TRUE_BILAT: its first three points (three
depths) with two time steps each and rise time 0, so that the comparison runs inside the kernel's epilogue (can_fuse) and the host
does not pick the cell kernels (half a point per centroid).  Source i of a list is the base source with its strike turned by
0.1 (i + 1) degrees, 100 (i mod 4) m deeper and delayed by DELAYS[i mod 4] seconds -- 1.25 s is two and a half samples --, so the
members of an aligned group of four or two are neighbours (a quarter of the node spacing: 1000 m, 500 m) with different blend
weights, rotations and shifts.  `origin` sets north and east of every centroid to 0: the back azimuth of the centroid then is the
origin's, lambda == 0 in the geometry and the apply takes its `plain` routines; the three points keep their depths, so the groups stay.

The references are NOT the full source (a 6-centroid cut is a few per cent of it, and a misfit of 0.95 norm factors says nothing
about the synthetic): they are the oracle's synthetics of a cut of the same kind -- base source, strike + 0.25 degrees, 150 m
deeper, 1.5 s later.  The misfits of the trial sources then are a few per cent to a third of their norm factors under l2norm and
l1norm, about one under scalar_product and about 1.4 under peak (test_multi_oracle_cases.py bounds them: 0.01 ... 2).

What a case reaches is in its name: ns4 / ns2 / mixed (sources per workgroup), ng10 / ng8, bil / near, rot / plain, then what
differs from the defaults (plans, l2norm, synthetics factor 1, windows of 1100 samples):
  core   ns x ng x interpolation x branch: every apply routine apply_group_asm_{10,8}_k{5,9}_{rot,plain} and both row-load forms
  noplan / rows   KIWI_HIP_MULTI_PLAN=0 (loop top from the head records), KIWI_HIP_COMPACT=0 (128-int descriptor rows)
  l1norm ... peak, f07   the general path of fused_acc4 and, for peak, the maximum of misfit_finish_kernel over a cleared buffer
  w130-256-600 / w257-512-513   windows of different lengths in one launch: tiles beyond a receiver's window, every tile boundary
  w130-200-256   max_wlen == 256: no pairs; of six sources four make a group, two go to the grouped kernel
  span16 / span17   first shifts of a group of four exactly 16 samples apart (kiwi_quad_shift_span): one group; 17: two pairs
  us21   spatial under-sampling (2, 1): members 500 m apart in north, neighbours only under the doubled limit; doubled row stride
  mixed  ten sources: two groups of four and a pair, both launches in one evaluation
"""
import collections
import functools

import numpy as np

from kiwi_amd import synthetic
from oracle import ko
from tests.common import Scenario

DT = 0.5                                  # sample interval of the database and effective dt of the sources
STEPS = 5                                 # time steps per point of the discretised base source
POINTS = ((0, 1), (1, 2), (2, 3))         # time steps kept of the first three points
DELAYS = (0.0, 0.5, 1.25, 2.0)            # origin delay of member i mod 4, seconds
COMPS = ["ned", "ard", "swu"]
METHODS = {"l2norm": 1, "l1norm": 2, "scalar_product": 5, "peak": 6}
QUAD_SPAN = 16                            # kiwi_quad_shift_span(): first shifts of a group of four, samples
NX, NZ, L = 16, 5, 1100
WINDOW_OFFSET = 480                       # windows shorter than the traces begin this many samples behind the reference's first

Case = collections.namedtuple("Case", "name ng bilinear origin nsrc duo env method factor windows delays us north quads pairs span")


def _case(name, ns=4, nsrc=None, quads=None, pairs=None, **kw):
    nsrc = (8 if ns == 4 else 6) if nsrc is None else nsrc
    if quads is None:
        quads = [tuple(range(a, a + 4)) for a in range(0, nsrc - 3, 4)] if ns == 4 else []
    if pairs is None:
        pairs = [] if ns == 4 else [(a, a + 1) for a in range(0, nsrc - 1, 2)]
    d = dict(ng=10, bilinear=True, origin=False, env=(), method="l2norm", factor=1.0, windows=(L, L, L), delays=DELAYS, us=(1, 1),
             north=0.0, span=4)
    d.update(kw)
    return Case(name=name, nsrc=nsrc, duo=ns, quads=tuple(quads), pairs=tuple(pairs), **d)


def _all_cases():
    out = []
    for ns in (4, 2):
        t = "ns%d-" % ns
        for ng in (10, 8):
            for bil in (True, False):
                for origin in (False, True):
                    out.append(_case(t + "ng%d-%s-%s" % (ng, "bil" if bil else "near", "plain" if origin else "rot"), ns, ng=ng,
                                     bilinear=bil, origin=origin))
        out.append(_case(t + "ng10-bil-rot-noplan", ns, env=(("KIWI_HIP_MULTI_PLAN", "0"),)))
        out.append(_case(t + "ng10-bil-rot-rows", ns, env=(("KIWI_HIP_COMPACT", "0"),)))
        for method in METHODS:
            for f in (1.0, 0.7):
                if method == "l2norm" and f == 1.0:
                    continue                                   # (the core case)
                out.append(_case(t + "ng10-bil-rot-%s%s" % (method, "-f07" if f != 1.0 else ""), ns, method=method, factor=f))
        out.append(_case(t + "ng10-bil-plain-peak", ns, origin=True, method="peak"))
        out.append(_case(t + "ng10-bil-plain-l1norm-f07", ns, origin=True, method="l1norm", factor=0.7))
        out.append(_case(t + "ng10-bil-rot-w130-256-600", ns, windows=(130, 256, 600)))
        out.append(_case(t + "ng10-bil-rot-w257-512-513", ns, windows=(257, 512, 513)))
    out.append(_case("ns4-ng10-bil-rot-w130-200-256", 4, nsrc=6, windows=(130, 200, 256), quads=[(0, 1, 2, 3)], pairs=[]))
    out.append(_case("ns4-ng10-bil-rot-span16", 4, nsrc=4, delays=(0.0, 0.5, 1.25, 8.0), span=16))
    out.append(_case("ns4-ng10-bil-rot-span17", 4, nsrc=4, delays=(0.0, 0.5, 1.25, 8.5), span=17, quads=[], pairs=[(0, 1), (2, 3)]))
    out.append(_case("ns4-ng10-bil-rot-us21", 4, us=(2, 1), north=500.0))
    out.append(_case("mixed-ng10-bil-rot", 4, nsrc=10, pairs=[(8, 9)]))
    return out


CASES = collections.OrderedDict((c.name, c) for c in _all_cases())


# ---------------------------------------------------------------- centroid tables
def cut_table(params, origin, t_add=0.0):
    """(centroid table, moment) of bilateral `params` cut to POINTS, delayed by t_add seconds; `origin`: north = east = 0"""
    cent, mo, _, _ = ko.discretize(1, np.asarray(params, np.float32), DT)
    assert len(cent) % STEPS == 0 and len(cent) // STEPS >= len(POINTS)
    rows = []
    for j, ks in enumerate(POINTS):
        for k in ks:
            row = cent[STEPS * j + k].copy()
            assert np.array_equal(row[:3], cent[STEPS * j][:3])                  # the same point: one centroid group
            row[3] += np.float32(t_add)
            rows.append(row)
    t = np.array(rows, np.float32)
    if origin:
        t[:, 0:2] = 0.0
    return t, mo


def source_params(case, i):
    p = np.array(synthetic.TRUE_BILAT, np.float32)
    p[1] += np.float32(case.north * (i % 4))
    p[3] += np.float32(100.0 * (i % 4))
    p[5] += np.float32(0.1 * (i + 1))
    return p


def trial_tables(case):
    """(tables, moments) of the case's trial sources: what goes to oracle.set_centroids and to Engine.set_sources"""
    tm = [cut_table(source_params(case, i), case.origin, case.delays[i % 4]) for i in range(case.nsrc)]
    return [t for t, _ in tm], [m for _, m in tm]


def reference_table(case):
    p = np.array(synthetic.TRUE_BILAT, np.float32)
    p[3] += np.float32(150.0)
    p[5] += np.float32(0.25)
    return cut_table(p, case.origin, 1.5)


def group_lengths(table):
    """lengths of the runs of consecutive centroids at the same point (the centroid groups: the time steps kept here are a sample
    apart, far inside the halo that would cut a run)"""
    out, k = [], 0
    while k < len(table):
        n = 1
        while k + n < len(table) and np.array_equal(table[k + n][:3], table[k][:3]):
            n += 1
        out.append(n)
        k += n
    return tuple(out)


def first_shift(table):
    """integer shift of a table's first centroid, as the host computes it (fp32 quotient, floor)"""
    return int(np.floor(np.float32(table[0][3]) / np.float32(DT)))


def neighbour_limits(case):
    return 0.25 * 4000.0 * case.us[0], 0.25 * 2000.0 * case.us[1]


# ---------------------------------------------------------------- scenario, references, windows
@functools.lru_cache(maxsize=None)
def _setup(ng, bilinear, us, origin, windows):
    """Scenario of these settings with the references (oracle synthetics of the reference table) and one taper per receiver that
    makes its window exactly windows[ir] samples long"""
    case = _case("setup", ng=ng, bilinear=bilinear, us=us, origin=origin, windows=windows)
    sc = Scenario(nx=NX, nz=NZ, ng=ng, L=L, nrec=3, comps_list=COMPS, variant="probe", bilinear=bilinear, effective_dt=DT)
    e = sc.oracle()
    e.set_interpolation(bilinear, us[0], us[1])
    t, mo = reference_table(case)
    e.set_centroids(t, mo, 0.0)
    e.calculate_seismograms()
    e.scale_seismograms()
    for ir in range(sc.nrec):
        for k in range(len(COMPS[ir])):
            sc.refs[(ir + 1, k + 1)] = e.synthetic(ir + 1, k + 1, 1)
        lo, d = sc.refs[(ir + 1, 1)]
        w = windows[ir]
        first = lo + (WINDOW_OFFSET if w < len(d) - WINDOW_OFFSET else 0)
        sc.tapers[ir + 1] = synthetic.full_taper(first, w, DT, sc.taper_ramp)
    e.close()
    sc.odb.close()
    sc.window_first = {ir: int(round(sc.tapers[ir][0][0] / DT)) for ir in sc.tapers}
    return sc


def setup(case):
    return _setup(case.ng, case.bilinear, case.us, case.origin, case.windows)


def oracle_engine(case):
    """a fresh oracle engine with the case's references, tapers, norm and factor (close it, and its .db, after use)"""
    sc = setup(case)
    e = sc.oracle()
    e.set_interpolation(case.bilinear, case.us[0], case.us[1])
    sc.apply_setup(e, True)
    e.set_misfit_method(METHODS[case.method])
    e.set_synthetics_factor(case.factor)
    return e


def product_engine(case):
    """a fresh device engine with the same setup (the environment is the caller's business)"""
    sc = setup(case)
    e = sc.oracle()                                   # (packs the database the product is handed)
    e.close()
    p = sc.product()
    sc.odb.close()
    p.set_spacial_undersampling(case.us[0], case.us[1])
    sc.apply_setup(p, False)
    p.set_misfit_method(case.method)
    p.set_synthetics_factor(case.factor)
    return p


OracleResults = collections.namedtuple("OracleResults", "misfits norms globals syn tapered ref geometry")


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_results(name):
    """The oracle's answers of a case, computed once and shared (read-only): misfits and norm factors [source, slot], global misfits
    [source], plain synthetics and tapered synthetics {(source, receiver, component): (first, data)} (1-based receiver and
    component), tapered references {(receiver, component): (first, data)}, geometry records {(source, receiver): GeoRec array}"""
    from kiwi_amd.engine import GEOREC
    case = CASES[name]
    tables, moments = trial_tables(case)
    e = oracle_engine(case)
    ms, ns, gs, syn, tap, geo, ref = [], [], [], {}, {}, {}, {}
    for s, (t, mo) in enumerate(zip(tables, moments)):
        e.set_centroids(t, mo, 0.0)
        m, n, g = e.get_misfits()
        ms.append(m.copy()); ns.append(n.copy()); gs.append(g)
        for ir in range(1, 4):
            geo[(s, ir)] = _frozen(e.centroid_geometry(ir, len(t), GEOREC))
            for k in range(1, len(COMPS[ir - 1]) + 1):
                lo, d = e.synthetic(ir, k, 1)
                syn[(s, ir, k)] = (lo, _frozen(d))
                lo, d = e.synthetic(ir, k, 2)
                tap[(s, ir, k)] = (lo, _frozen(d))
                if s == 0:
                    lo, d = e.reference(ir, k, 2)
                    ref[(ir, k)] = (lo, _frozen(d))
    e.close()
    e.db.close()
    return OracleResults(_frozen(np.array(ms)), _frozen(np.array(ns)), _frozen(np.array(gs, np.float32)), syn, tap, ref, geo)
