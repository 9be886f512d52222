"""accumulate_multi_kernel against the CPU oracle: the cases of tests/multi_oracle_cases.py (what each one reaches is said there),
under KIWI_HIP_POISON=1 and KIWI_HIP_DEBUG=1.

The device-versus-device comparisons of tests/test_gpu_multi_plan.py and tests/test_gpu_parity.py share geometry_kernel, the
coefficient lines, the apply routines, fused_acc4 and misfit_finish_kernel between the two sides; a mistake in any of those passes
them.  Here the other side is the oracle, per case:

  1. the kernel ran: the numbers of groups of four and of pairs the library reports for the chunk are the case's -- a case that
     falls back to the grouped kernel fails (the fixtures have every trace and rows that end in zero: tests/test_multi_oracle_cases.py,
     so the device refuses no (group, receiver) of those the host has flagged);
  2. synthetics (the kernel without its comparator): every source, receiver and component within SYN_RTOL of the oracle's trace
     maximum over the WHOLE window: windows shorter than the traces lie inside the oracle's data span altogether; a window as long
     as the traces reaches beyond it by the source's delay at most, and there the oracle's trace is zero and so must the device's be;
  3. bit identity under `exact` wherever the device's geometry records are the oracle's byte for byte (at least half of the
     (source, receiver) pairs of every case);
  4. misfits, norm factors and global misfits through the kernel's own comparator (no synthetics kept), with the tolerances of
     tests/common.py under both arithmetic contracts; `peak` under `fused` is one sample of the difference trace, no sum averages
     its round-off: 2e-6, as tests/fuzz_gpu_parity.py states it.

Instantiations of accumulate_multi_kernel<NG, FUSE, NS, COMPACT, PLAN> x apply routine and a case that reaches each (every case
runs FUSE = true in its first evaluation and FUSE = false in the one that keeps the synthetics):
  <10, *, 4, 1, 1> rot ns4-ng10-bil-rot         plain ns4-ng10-bil-plain      <8, *, 4, 1, 1> rot ns4-ng8-bil-rot    plain ns4-ng8-bil-plain
  <10, *, 2, 1, 1> rot ns2-ng10-bil-rot         plain ns2-ng10-bil-plain      <8, *, 2, 1, 1> rot ns2-ng8-bil-rot    plain ns2-ng8-bil-plain
  <10, *, 4, 1, 0> rot ns4-ng10-bil-rot-noplan  <10, *, 4, 0, 0> rot ns4-ng10-bil-rot-rows
  <10, *, 2, 1, 0> rot ns2-ng10-bil-rot-noplan  <10, *, 2, 0, 0> rot ns2-ng10-bil-rot-rows
(The table rests on reading can_fuse() and kiwi_hip_init, not on an assertion: the library's debug line reports the grouping only.
The fixtures have rise time 0, a taper at every receiver and a time-domain norm, which is what can_fuse() asks for, and the switches
are read when the context is made.  A change that made can_fuse() false for these fixtures, or ignored KIWI_HIP_MULTI_PLAN or
KIWI_HIP_COMPACT, would still pass here.)
Still open (they do not reach this kernel's comparator by design): databases with static end values or gaps (no compact
descriptors, the tail rule), missing traces (those pairs go to the grouped kernel) and sources with a rise time (can_fuse is false)."""
import numpy as np
import pytest

from tests import multi_oracle_cases as mc
from tests.common import SYN_RTOL, arith, misfit_close, multi_groups

pytestmark = pytest.mark.gpu

_SWITCHES = ("KIWI_HIP_ACCUM", "KIWI_HIP_FUSE", "KIWI_HIP_MULTI_PLAN", "KIWI_HIP_COMPACT", "KIWI_HIP_CELL", "KIWI_HIP_RUNS", "KIWI_HIP_DEDUPE",
             "KIWI_HIP_GROUP_THREADS", "KIWI_HIP_QUAD_SPAN")


def _engine(case, monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KIWI_HIP_DUO", str(case.duo))
    monkeypatch.setenv("KIWI_HIP_POISON", "1")             # a plan, descriptor or coefficient line read but not written shows
    monkeypatch.setenv("KIWI_HIP_DEBUG", "1")
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    p = mc.product_engine(case)
    tables, moments = mc.trial_tables(case)
    p.set_sources(tables, moments=moments)
    return p


def _on_window(lo_p, n, lo_o, so):
    """the oracle's trace (first sample lo_o) on the device's window lo_p .. lo_p + n - 1, zero outside its data span; and the overlap"""
    a, b = max(lo_o, lo_p), min(lo_o + len(so), lo_p + n)
    want = np.zeros(n, np.float32)
    if b > a:
        want[a - lo_p:b - lo_p] = so[a - lo_o:b - lo_o]
    return want, a, b


def _slots(case):
    return [(s, ir, k) for s in range(case.nsrc) for ir in range(1, 4) for k in range(1, len(mc.COMPS[ir - 1]) + 1)]


@pytest.mark.parametrize("name", list(mc.CASES))
def test_multi_kernel_against_oracle(monkeypatch, capfd, name, _arith):
    assert arith() == _arith                               # (the contract the instance is named after is the one in force)
    case = mc.CASES[name]
    o = mc.oracle_results(name)
    sc = mc.setup(case)
    capfd.readouterr()
    p = _engine(case, monkeypatch)
    p.eval()                                               # 4: compared in the kernel's epilogue, nothing kept
    pm, pn, pg = [x.copy() for x in p.get_misfits()]
    p.set_keep_synthetics(1)
    p.eval()                                               # 2: the synthetics themselves
    syn = {q: p.get_synthetics(*q, 1) for q in _slots(case)}
    p.close()
    taken = multi_groups(capfd.readouterr().err)

    # 1. the kernel under test ran, in both evaluations
    assert len(taken) == 2 and all(t == (case.nsrc, len(case.quads), len(case.pairs)) for t in taken), taken

    # 2. synthetics on the whole window
    worst = 0.0
    for q in _slots(case):
        s, ir, k = q
        lo_p, sp = syn[q]
        lo_o, so = o.syn[q]
        assert len(sp) == case.windows[ir - 1] and lo_p == sc.window_first[ir], q
        want, a, b = _on_window(lo_p, len(sp), lo_o, so)
        if len(sp) < mc.L:
            assert (a, b) == (lo_p, lo_p + len(sp)), q                  # the window lies inside the data span
        # a window as long as the traces begins at the reference's first sample (1.5 s = 3 samples late): a source delayed by d
        # samples begins at most d - 3 samples inside it, and its data span (1100 samples and the spread of its shifts) ends behind it
        late = int(np.ceil(case.delays[s % 4] / mc.DT)) - 3
        assert b - a >= len(sp) - max(late, 0) and np.any(want != 0), q
        err = float(np.max(np.abs(sp.astype(np.float64) - want))) / float(np.max(np.abs(so)))
        worst = max(worst, err)
        assert err <= SYN_RTOL, (q, err)

    # 4. misfits through the in-kernel comparator
    scale = np.maximum(np.abs(o.misfits), o.norms if arith() == "fused" else 0.0)
    mworst = float(np.max(np.abs(pm.astype(np.float64) - o.misfits) / scale))
    print("FIGURES %s %s: synthetics %.3g of the trace maximum, misfits %.3g of their scale, global %.3g" % (
        name, arith(), worst, mworst, float(np.max(np.abs(pg.astype(np.float64) - o.globals) / np.abs(o.globals)))))
    rtol = 2e-6 if (case.method == "peak" and arith() == "fused") else None
    assert pm.shape == o.misfits.shape and np.all(np.isfinite(pm))
    assert np.array_equal(pn, o.norms)
    assert misfit_close(pm, o.misfits, pn, rtol=rtol), mworst
    assert misfit_close(pg, o.globals, glob=True, rtol=rtol)


@pytest.mark.exact_only
@pytest.mark.parametrize("name", list(mc.CASES))
def test_multi_kernel_bitexact_given_geometry(monkeypatch, name, _arith):
    """The form of test_accumulate_bitexact_given_geometry: where the device's geometry records are the oracle's, so are the
    synthetics, bit for bit.  A (source, receiver) pair is left out only for differing records (device libm against glibc in the last
    place of an fp32 weight); at least half of a case's pairs are compared."""
    assert arith() == _arith == "exact"
    case = mc.CASES[name]
    o = mc.oracle_results(name)
    p = _engine(case, monkeypatch)
    p.set_keep_synthetics(1)
    p.eval()
    compared = 0
    for s in range(case.nsrc):
        for ir in range(1, 4):
            g = p.get_geometry(s, ir)
            g["flags"] &= 3                                 # bit 2 (same point as the predecessor) and the group hint are device-only
            g["pad"] = 0
            if g.tobytes() != o.geometry[(s, ir)].tobytes():
                continue
            compared += 1
            for k in range(1, len(mc.COMPS[ir - 1]) + 1):
                lo_p, sp = p.get_synthetics(s, ir, k, 1)
                lo_o, so = o.syn[(s, ir, k)]
                want, a, b = _on_window(lo_p, len(sp), lo_o, so)
                assert np.array_equal(sp[a - lo_p:b - lo_p].view(np.uint32), want[a - lo_p:b - lo_p].view(np.uint32)), (s, ir, k)
                assert np.array_equal(sp, want), (s, ir, k)             # (and zero outside the oracle's data span)
    p.close()
    print("FIGURES %s: %d of %d (source, receiver) pairs compared bit for bit" % (name, compared, 3 * case.nsrc))
    assert 2 * compared >= 3 * case.nsrc, compared
