"""kiwi_hip_band_misfits on the device: every band of one call is bit for bit what the separate evaluation with that band's
filter and method returns (the parent commit's path: set_misfit_filter + set_misfit_method + eval + get_misfits), whatever its
neighbour bands, the window and transform length, the rise-time fold, the synthetics factor, the first source, the pieces, the
chunking and the kind of context; failings; what the call leaves alone; the refusals; the example.  Under the `fused`
arithmetic contract the two calls may be served by different instantiations of the accumulate kernel: where their synthetics
differ, tests/bands_cases.py assert_bands_equal applies the tolerance of include/kiwi_hip.h and says so."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kiwi_amd.lib import KiwiHipError
from tests import common
from tests.bands_cases import ALL_BANDS, COMPS, FILTER, TD_BANDS, assert_bands_equal, no_rise_list, separate, trial_list
from tests.linfit_cases import eikonal_list_with_a_failed_piece
from tests.test_linfit_gpu import build, multi_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_shared = {}


def standard(arith):
    """band call and separate evaluations of the standard case, computed once per arithmetic contract and shared"""
    if arith not in _shared:
        sc, p = build(COMPS, planted=False)
        try:
            p.switch_receiver(6, False)
            tr = trial_list(8)
            p.set_source_params("bilateral", tr)
            want = separate(p, ALL_BANDS)
            p.set_misfit_bands(ALL_BANDS)
            got = p.band_misfits()
            _shared[arith] = (tr, want, got)
        finally:
            p.close()
    return _shared[arith]


def test_every_kind_of_band_equals_the_separate_evaluation(_arith):
    tr, want, got = standard(_arith)
    assert got[0].shape == (8, 12, 11) and got[2].shape == (8, 12)               # slots of d, ne, ned, ned, ne; the sixth receiver is off
    assert np.all(np.isfinite(got[0])) and np.all(got[0] != 0) and np.all(got[1] > 0) and np.all(got[2] > 0)
    assert_bands_equal(got, want, "12 bands")
    # a band's answer does not depend on its neighbours: two subsets (one filtered time-domain band only; a mix in another order)
    sc, p = build(COMPS, planted=False)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("bilateral", tr)
        for idx in ([5], [10, 7, 0, 9, 4, 3]):
            p.set_misfit_bands([ALL_BANDS[i] for i in idx])
            assert p.misfit_bands() == len(idx)
            assert_bands_equal(p.band_misfits(), tuple(x[:, idx] for x in want), "subset %s" % idx)
    finally:
        p.close()


@pytest.mark.parametrize("window", [100, 600, 1000, None, 4096])
def test_window_lengths_and_transform_edges(window):
    """windows of 100, 600, 1000 samples, the whole trace and 4096 samples: transform lengths of 1024 and 4096 (a pair's length
    is at least twice its reference's); with four filtered bands the spectrum is kept in an LDS copy (the length at which it
    does not fit: test_longest_transform_and_lengths_beyond_it)"""
    bands = [ALL_BANDS[i] for i in (0, 4, 5, 6, 7, 8, 10, 11)]
    sc, p = build(COMPS, window=window)
    try:
        rows = np.tile(sc.true_params, (6, 1))
        rows[:, 0] = np.linspace(-4.0, 4.0, 6)                # origin times: the strips move against the window
        rows[:, 4:10] *= np.linspace(0.5, 1.5, 6)[:, None].astype(np.float32)
        rows[:, 10] = 1.7                                     # rise time: three taps
        p.set_source_params("moment_tensor", rows)
        ntrans = set()
        want = separate(p, bands, ntrans=ntrans)
        p.set_misfit_bands(bands)
        assert_bands_equal(p.band_misfits(), want, "window %s" % window)
        print("window %s: transform lengths %s" % (window, sorted(ntrans)))
        _shared.setdefault("ntrans", set()).update(ntrans)
        assert min(ntrans) >= (window or 1) and all(n & (n - 1) == 0 for n in ntrans)
        # two distinct transform lengths over the cases: the references' length sets 1024 for the windows inside them, the long window its own
        assert (max(ntrans) >= 4096) == (window == 4096)
    finally:
        p.close()


def _child(args, env_extra):
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_bands_child_%d.npz" % os.getpid())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bands_cases.py"), out] + [str(a) for a in args], capture_output=True, text=True,
                       env=dict(os.environ, **env_extra), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = dict(np.load(out))
    os.remove(out)
    return z


def test_longest_transform_and_lengths_beyond_it():
    """A reference of 10000 samples makes its slot's transform 32768 samples long, the longest the in-LDS transforms take and
    the one length at which the copy of the spectrum does not fit (2 x 128 KiB): the row is transformed again per filtered band,
    beside slots of 1024 samples that keep the copy.  A reference of 20000 samples asks for 65536 and is refused with the length
    in the message; so is a window that does not fit the row."""
    bands = [ALL_BANDS[i] for i in (0, 4, 5, 6, 8, 10, 11)]
    sc, p = build(COMPS, planted=False)
    try:
        lo, d = sc.refs[(1, 1)]
        p.set_ref_seismogram(1, 1, lo, np.concatenate([d, np.zeros(10000 - len(d), np.float32)]))
        p.set_source_params("bilateral", trial_list(5))
        ntrans = set()
        want = separate(p, bands, ntrans=ntrans)
        assert ntrans == {32768}, ntrans                      # (receiver 1's only slot)
        p.set_misfit_bands(bands)
        assert_bands_equal(p.band_misfits(), want, "32768 samples")
        p.set_ref_seismogram(1, 1, lo, np.concatenate([d, np.zeros(20000 - len(d), np.float32)]))
        with pytest.raises(KiwiHipError, match="needs a transform of 65536 samples"):
            p.band_misfits()
        p.set_misfit_bands(TD_BANDS)                          # no spectrum needed: no transform length to refuse
        assert_bands_equal(p.band_misfits(), separate(p, TD_BANDS), "time-domain bands beside a long reference")
    finally:
        p.close()
    sc, q = build(COMPS, planted=False, window=40000)
    try:
        q.set_source_params("bilateral", trial_list(5))
        q.set_misfit_bands(TD_BANDS)
        with pytest.raises(KiwiHipError, match="a misfit window of 40000 samples does not fit"):
            q.band_misfits()
    finally:
        q.close()


def test_sources_without_rise_time_and_the_comparator_inside_the_accumulate_kernel(_arith):
    """The one documented exception to `bit for bit` (include/kiwi_hip.h): no source of the batch has a rise time, so the plain
    evaluation of an unfiltered time-domain method compares inside the accumulate kernel, whose fp64 partial sums run per tile
    and wave; the bands sum in misfit_kernel's order.  Both orders add the same fp32-exact terms in fp64 (relative difference of
    the sums ~1e-15), so the fp32 results agree within the bound the header states and the existing suite holds the two
    comparators to (tests/test_gpu_parity.py): 1e-6 of max(misfit, norm factor).  With KIWI_HIP_FUSE=0, in a process of its
    own, the plain evaluation uses misfit_kernel and the bits are equal."""
    rows = no_rise_list(8)
    sc, p = build(COMPS, planted=False)
    try:
        p.switch_receiver(6, False)
        p.set_source_params("moment_tensor", rows)
        sm, sn, sg = separate(p, TD_BANDS)
        p.set_misfit_bands(TD_BANDS)
        m, n, g = p.band_misfits()
        print("no rise time, default setting: misfits equal in bits: %s, largest |difference| / max(misfit, norm) %.3g" % (
            np.array_equal(m, sm), np.max(np.abs(m.astype(np.float64) - sm) / np.maximum(np.abs(sm), sn))))
        assert np.array_equal(n, sn)
        assert np.all(np.abs(m.astype(np.float64) - sm) <= 1e-6 * np.maximum(np.abs(sm.astype(np.float64)), sn))
        assert np.all(np.abs(g.astype(np.float64) - sg) <= 1e-6 * np.sqrt(sg.astype(np.float64) ** 2 + 1.0))
        if common.arith() == "exact":
            assert np.array_equal(m[:, 3], sm[:, 3])          # peak: a maximum has no order
    finally:
        p.close()
    z = _child([8, "td", "norise", 1], dict(KIWI_HIP_FUSE="0"))
    assert str(z["error"]) == ""
    assert_bands_equal((z["misfit"], z["norm"], z["glob"]), (z["sep_misfit"], z["sep_norm"], z["sep_glob"]), "no rise time, KIWI_HIP_FUSE=0")
    assert np.array_equal(z["norm"], n)


def test_rise_time_fold_and_synthetics_factor():
    sc, p = build(COMPS, planted=False)
    try:
        tr = trial_list(5)
        tr[:, 13] = [0.0, 1.2, 3.4, 6.1, 2.0]                 # no fold, 3, 7 and 13 taps
        p.set_synthetics_factor(0.7)
        p.set_source_params("bilateral", tr)
        want = separate(p, ALL_BANDS)
        p.set_misfit_bands(ALL_BANDS)
        assert_bands_equal(p.band_misfits(), want, "fold, factor 0.7")
    finally:
        p.close()


def test_first_source_pieces_chunks_and_contexts(_arith, monkeypatch):
    tr, want, got = standard(_arith)
    n = len(tr)
    sc, p = build(COMPS, planted=False)
    try:
        p.switch_receiver(6, False)
        p.set_misfit_bands(ALL_BANDS)
        p.set_source_params("bilateral", tr)
        assert_bands_equal(p.band_misfits(0, n), got, "band_misfits(0, n)")
        assert_bands_equal(p.band_misfits(3, n - 3), tuple(x[3:] for x in got), "isrc0 = 3")
        for piece in (2, n):
            m, nn, g, failings = p.band_misfits_for_params("bilateral", tr, piece=piece)
            assert failings == [] and p.nsrc == piece
            assert_bands_equal((m, nn, g), got, "piece %d" % piece)
    finally:
        p.close()
    # several chunks: KIWI_HIP_CHUNK_MB is read when a context is made -- a process of its own
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_bands_chunks_%d.npz" % os.getpid())
    env = dict(os.environ, KIWI_HIP_CHUNK_MB="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bands_cases.py"), out, str(n)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    os.remove(out)
    assert str(z["error"]) == "" and z["launches"][1] >= 2, (str(z["error"]), z["launches"])
    assert_bands_equal((z["misfit"], z["norm"], z["glob"]), got, "%d chunks" % z["launches"][1])
    # two contexts stacked on one device where there is no second one
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("KIWI_HIP_MULTI_OVERSUBSCRIBE", "1")
    sc, m2 = build(COMPS, planted=False, engine=multi_engine(2))
    try:
        assert m2.ndevices() == 2
        m2.switch_receiver(6, False)
        m2.set_misfit_bands(ALL_BANDS)
        m, nn, g, failings = m2.band_misfits_for_params("bilateral", tr, piece=3)
        assert failings == []
        assert_bands_equal((m, nn, g), got, "two devices")
    finally:
        m2.close()


def test_failings_read_as_zeros():
    bands = [ALL_BANDS[i] for i in (0, 5, 8, 11)]
    sc, p = build(None, planted=False)
    try:
        G = np.load(os.path.join(ROOT, "tests", "golden", "eikonal_vectors.npz"))
        p.set_source_crust(G["rupture_profile"], G["origin_profile"])
        p.set_source_constraints(np.array([[0, 0, 6500.0], [0, 0, 15500.0]], np.float32), np.array([[0, 0, -1.0], [0, 0, 1.0]], np.float32))
        eik = np.tile(np.array([0., 0., 0., 10500., 1.0, 80., 70., 100., -50., 2500., 500., 200., 0.8] + [0.] * 6 + [1.5], np.float32), (5, 1))
        eik[:, 13:19] = np.random.default_rng(6).standard_normal((5, 6)) * 1e18
        eik[2, 3] = 500.0                                     # "Empty rupture area": above the constraining planes
        p.set_misfit_bands(bands)
        m, n, g, failings = p.band_misfits_for_params("mt_eikonal", eik)
        assert failings == [2]
        assert np.all(m[2] == 0) and np.all(n[2] == 0) and np.all(g[2] == 0)
        good = [0, 1, 3, 4]
        p.set_source_params("mt_eikonal", eik[good])
        assert_bands_equal((m[good], n[good], g[good]), separate(p, bands), "sources beside a failing")
        # the failing inside an uploaded batch
        try:
            p.set_source_params("mt_eikonal", eik)
        except KiwiHipError:
            pass
        assert list(np.nonzero(p.get_source_status())[0]) == [2]
        assert_bands_equal(p.band_misfits(), (m, n, g), "uploaded batch with a failing")
    finally:
        p.close()


def test_nothing_else_changes():
    sc, p = build(COMPS, planted=False)
    try:
        tr = trial_list(6)
        p.set_misfit_filter(0, *FILTER)
        p.set_misfit_method("l1norm")
        p.set_source_params("bilateral", tr)
        p.eval()
        before = p.get_misfits()
        p.set_misfit_bands(ALL_BANDS[:3])
        p.eval()
        for a, b in zip(p.get_misfits(), before):
            assert np.array_equal(a, b)                       # bands set: eval as before
        p.band_misfits()
        # after a band call get_misfits returns what a plain evaluation leaves (the context's own method and filter) -- never band values
        for a, b in zip(p.get_misfits(), before):
            assert common.same_bits(a, b) if common.arith() == "exact" else common.misfit_close(a, b, norm=before[1] if a.ndim == 2 else None, glob=a.ndim == 1)
        p.eval()
        for a, b in zip(p.get_misfits(), before):
            assert np.array_equal(a, b)                       # method and filter are what they were
        p.set_misfit_bands([])
        assert p.misfit_bands() == 0
        p.eval()
        for a, b in zip(p.get_misfits(), before):
            assert np.array_equal(a, b)
        with pytest.raises(KiwiHipError, match="no misfit bands set"):
            p.band_misfits()
    finally:
        p.close()


def test_refusals_name_the_reason():
    sc, p = build(COMPS, planted=False)
    try:
        tr = trial_list(5)
        p.set_source_params("bilateral", tr)
        with pytest.raises(KiwiHipError, match="no misfit bands set"):
            p.band_misfits()
        with pytest.raises(KiwiHipError, match="floating norm"):
            p.set_misfit_bands([("l2norm", None, None), ("floating_l2norm", None, None)])
        assert p.misfit_bands_max() == 16
        with pytest.raises(KiwiHipError, match="17 bands; at most 16"):
            p.set_misfit_bands([("l2norm", None, None)] * 17)
        assert p.misfit_bands() == 0
        p.set_misfit_bands(ALL_BANDS[:2])
        with pytest.raises(KiwiHipError, match="not inside the uploaded batch"):
            p.band_misfits(2, 4)
        p.set_misfit_method("floating_l1norm")
        with pytest.raises(KiwiHipError, match="floating norm"):
            p.band_misfits()
        p.set_misfit_method("l2norm")
        p.set_misfit_taper(2, [], [])
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.band_misfits()
        with pytest.raises(KiwiHipError, match="no misfit taper"):
            p.band_misfits_for_params("bilateral", tr)
        # the context is usable afterwards
        p.set_misfit_taper(2, *sc.tapers[2])
        p.set_source_params("bilateral", tr)
        m, n, g = p.band_misfits()
        assert_bands_equal((m, n, g), separate(p, ALL_BANDS[:2]), "after the refusals")
    finally:
        p.close()


def test_library_transforms_only_is_refused_in_a_process_of_its_own(_arith):
    """KIWI_HIP_FUSED_FFT=0: bands that need a spectrum are refused with the documented message (Limits)"""
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "kiwi_bands_nofused_%d.npz" % os.getpid())
    env = dict(os.environ, KIWI_HIP_FUSED_FFT="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bands_cases.py"), out, "5"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    os.remove(out)
    assert "KIWI_HIP_FUSED_FFT=0 switches off" in str(z["error"]) and "misfit" not in z.files
    # bands of unfiltered time-domain methods alone need no transform: served, and equal to the separate evaluations
    z = _child([5, "td", "bilateral", 1], dict(KIWI_HIP_FUSED_FFT="0"))
    assert str(z["error"]) == ""
    assert_bands_equal((z["misfit"], z["norm"], z["glob"]), (z["sep_misfit"], z["sep_norm"], z["sep_glob"]), "time-domain bands, KIWI_HIP_FUSED_FFT=0")


def test_band_misfits_ms():
    sc, p = build(COMPS, planted=False)
    try:
        p.set_source_params("bilateral", trial_list(5))
        p.set_misfit_bands(ALL_BANDS)
        p.band_misfits()
        ms = p.band_misfits_ms()
        print("band call: evaluation %.3f ms, band kernels %.3f ms, downloads %.3f ms" % ms)
        assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0 and ms[2] >= 0
    finally:
        p.close()


def test_example_script_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "invert_multiband.py")], capture_output=True, text=True,
                         env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "planted source recovered" in out.stdout, out.stdout
    if common.arith() == "exact":                             # (fused: the two routes' batches differ in shape, see the module's docstring)
        assert "equal the separate evaluations bit for bit: True" in out.stdout, out.stdout


# ------------------------------------------------------------------------------------------------ a piece of which nothing is uploaded
def test_a_piece_in_which_every_source_fails_to_discretise():
    """three `mt_eikonal` sources in pieces of one, the middle one failing to discretise: nothing is uploaded for that piece.  It reads
    as zeros, its neighbours as the call without it gives them"""
    bands = [ALL_BANDS[i] for i in (0, 5, 8, 11)]
    sc, p = build(None, planted=False)
    try:
        eik, good = eikonal_list_with_a_failed_piece(p, 1)
        p.set_misfit_bands(bands)
        m, n, g, failings = p.band_misfits_for_params("mt_eikonal", eik, piece=1)
        assert failings == [1]
        assert not np.any(m[1]) and not np.any(n[1]) and not np.any(g[1])
        m2, n2, g2, none = p.band_misfits_for_params("mt_eikonal", good, piece=1)
        assert none == []
        assert_bands_equal((m[[0, 2]], n[[0, 2]], g[[0, 2]]), (m2, n2, g2), "sources beside a piece of which nothing is uploaded")
    finally:
        p.close()
