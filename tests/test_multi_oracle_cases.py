"""The fixtures of tests/multi_oracle_cases.py are what they claim to be -- on the CPU oracle alone, no device library.

These are conditions on the fixtures, not measurements of the product: a case whose misfits were tiny or of the size of their norm
factors would make the 1e-6 of the device comparison (tests/test_gpu_multi_oracle.py) say little about the synthetics; a case whose
tables were no neighbours, differed in structure or lay further apart in time than it says would not reach the kernel or the branch
it is named after."""
import numpy as np
import pytest

from tests import multi_oracle_cases as mc


@pytest.mark.parametrize("name", list(mc.CASES))
def test_fixture_is_what_it_claims(name):
    case = mc.CASES[name]
    tables, moments = mc.trial_tables(case)
    o = mc.oracle_results(name)
    nmis = sum(len(c) for c in mc.COMPS)
    assert o.misfits.shape == o.norms.shape == (case.nsrc, nmis) and len(tables) == case.nsrc

    # the misfits say something about the synthetics: between 0.01 and 2 norm factors in every slot
    assert np.all(o.norms > 0)
    ratio = o.misfits / o.norms
    assert np.all(ratio >= 0.01) and np.all(ratio <= 2.0), (ratio.min(), ratio.max())

    # every synthetic and every reference has non-zero samples inside its window, and the windows have the lengths of the case
    for ir in range(1, 4):
        for k in range(1, len(mc.COMPS[ir - 1]) + 1):
            lo, d = o.ref[(ir, k)]
            assert len(d) == case.windows[ir - 1] and np.count_nonzero(d) > len(d) // 2, (ir, k)
            for s in range(case.nsrc):
                lo, d = o.tapered[(s, ir, k)]
                assert np.count_nonzero(d) > case.windows[ir - 1] // 2, (s, ir, k)

    # groups of four and pairs: the same group lengths, end points within the neighbour limits
    lens = [mc.group_lengths(t) for t in tables]
    assert all(x == (2, 2, 2) for x in lens)
    near_h, near_z = mc.neighbour_limits(case)
    for grp in case.quads + case.pairs:
        a = tables[grp[0]]
        for i in grp[1:]:
            b = tables[i]
            assert lens[i] == lens[grp[0]] and len(a) == len(b)
            for row in (0, -1):
                assert abs(a[row][0] - b[row][0]) <= near_h and abs(a[row][1] - b[row][1]) <= near_h and abs(a[row][2] - b[row][2]) <= near_z
            assert not np.array_equal(a[:, :4], b[:, :4])              # (no two members share their geometry)
    if case.north:
        # under-sampled: neighbours only under the widened limit
        assert abs(tables[0][0][0] - tables[3][0][0]) > 0.25 * 4000.0

    # the first shifts of every complete aligned four are as far apart as the case says, and a group of four needs them within 16
    shifts = [mc.first_shift(t) for t in tables]
    for a in range(0, case.nsrc - 3, 4):
        assert max(abs(shifts[a + i] - shifts[a]) for i in range(1, 4)) == case.span, shifts
    assert case.span <= mc.QUAD_SPAN or not case.quads
    assert any(d / mc.DT != np.floor(d / mc.DT) for d in case.delays)         # a delay that is no whole number of samples

    # `plain` and `rot`: bit 1 of the oracle's geometry flags (lambda != 0) at every centroid and receiver
    for (s, ir), g in o.geometry.items():
        assert np.all(g["row"] >= 0), (s, ir)                              # every centroid finds its traces
        if case.origin:
            assert not np.any(g["flags"] & 2), (s, ir)
        else:
            assert np.all(g["flags"] & 2), (s, ir)


def test_axes_are_covered():
    """every value of every axis with four and with two sources per workgroup, and the named combinations"""
    cs = list(mc.CASES.values())
    assert 45 <= len(cs) <= 55 and len({c.name for c in cs}) == len(cs)
    for ns in (4, 2):
        mine = [c for c in cs if c.duo == ns and (c.quads if ns == 4 else c.pairs)]
        assert {(c.ng, c.bilinear, c.origin) for c in mine} == {(g, b, o) for g in (10, 8) for b in (True, False) for o in (True, False)}
        assert {c.env for c in mine} == {(), (("KIWI_HIP_MULTI_PLAN", "0"),), (("KIWI_HIP_COMPACT", "0"),)}
        assert {(c.method, c.factor) for c in mine if not c.origin} >= {(m, f) for m in mc.METHODS for f in (1.0, 0.7)}
        assert {c.method for c in mine if c.origin} >= {"peak", "l1norm", "l2norm"}
        assert {c.windows for c in mine} >= {(1100, 1100, 1100), (130, 256, 600), (257, 512, 513)}
    assert any(c.windows == (130, 200, 256) and c.nsrc == 6 and len(c.quads) == 1 and not c.pairs for c in cs)
    assert any(c.span == 16 and len(c.quads) == 1 for c in cs) and any(c.span == 17 and not c.quads and len(c.pairs) == 2 for c in cs)
    assert any(c.us == (2, 1) and c.quads for c in cs)
    assert any(len(c.quads) == 2 and len(c.pairs) == 1 and c.nsrc == 10 for c in cs)
