"""Batched fast-marching solves and the staged eikonal discretiser, the parts that need no GPU.

kiwi_hip_fast_marching_batch(where = 0) is the packed interface over the host's routine: a mixed batch -- the three field kinds
and the shapes of tests/test_fast_marching.py, 1 x 1, 1 x n and n x 1 grids, start points outside of the grid, a cfg4-sized grid
with `discard` -- gives, solve by solve, the bits of kiwi_hip_fast_marching(plain = 1).  The discretiser in three stages
(prepare, one batch of solves, finish; KIWI_HIP_EIK_STAGED=1 makes kiwi_hip_discretize_eikonal take that route with the host's
solver) gives the tables and error texts of the un-split one.  The size guard is tested through its predicate."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kiwi_amd import engine as ke
from kiwi_amd import lib as klib
from kiwi_amd.lib import KiwiHipError
from tests.test_fast_marching import fields, product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "eikonal_vectors.npz"))
N = int(G["n"])


def cfg4_field():
    """The field of test_cfg4_sized_grid_against_the_plain_routine: (speed, origin, delta, discard)."""
    nx, ny = 1200, 360
    yy, xx = np.mgrid[0:ny, 0:nx]
    depth = 6500.0 + (yy + 0.5) * 25.0
    speed = np.where(depth <= 12000.0, 3500.0, 3700.0).astype(np.float32) * np.float32(0.9)
    out = ((xx + 0.5 - nx / 2) * 25.0) ** 2 + (depth - 11000.0) ** 2 > 15000.0 ** 2
    dis = np.float32(speed.min() * np.float32(0.5))
    speed[out] = dis
    return speed, np.array([-15000., -4500.], np.float32), np.array([25., 25.], np.float32), float(dis)


def cfg4_starts(n, seed=5):
    """n start points spread over the rupture of cfg4_field (inside its bounding circle)."""
    rng = np.random.default_rng(seed)
    r = 13000.0 * np.sqrt(rng.uniform(0, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    x = np.clip(r * np.cos(phi), -14000, 14000)
    y = np.clip(r * np.sin(phi), -4000, 4000)
    return np.stack([x, y], 1).astype(np.float32)


def mixed_batch(with_cfg4=True):
    """(speeds, origins, deltas, starts, discards): the cases of test_both_marches_give_the_oracles_times (three kinds x 14
    seeds, among them 1 x n, n x 1 and 1 x 1 grids, start points outside of the grid), the early-termination cases, and one
    cfg4-sized grid with `discard`."""
    sp, og, dl, st, di = [], [], [], [], []
    for kind in ("layered", "uniform", "blocks"):
        for seed in range(14):
            rng = np.random.default_rng(1000 * len(kind) + seed)
            nx = 1 if seed == 0 else int(rng.integers(2, 90))
            ny = 1 if seed == 1 else int(rng.integers(2, 70))
            if seed == 2:
                nx, ny = 1, 1
            speed = fields(rng, kind, nx, ny)
            origin = rng.uniform(-5000, 0, 2).astype(np.float32)
            d = np.float32(rng.uniform(100, 900))
            delta = np.array([d, d], np.float32) if kind == "uniform" else rng.uniform(100, 900, 2).astype(np.float32)
            if kind == "uniform":
                start = (origin + (np.array([rng.integers(0, nx), rng.integers(0, ny)]) + 0.5) * delta).astype(np.float32)
            else:
                start = (origin + rng.uniform(-0.2, 1.2, 2) * delta * [nx, ny]).astype(np.float32)
            sp.append(speed); og.append(origin); dl.append(delta); st.append(start); di.append(np.nan)
    for seed in range(6):
        rng = np.random.default_rng(500 + seed)
        nx, ny = int(rng.integers(20, 120)), int(rng.integers(20, 80))
        speed = fields(rng, "layered", nx, ny)
        origin = np.array([-1000., -700.], np.float32)
        delta = rng.uniform(20, 60, 2).astype(np.float32)
        start = (origin + rng.uniform(0.3, 0.7, 2) * delta * [nx, ny]).astype(np.float32)
        sp.append(speed); og.append(origin); dl.append(delta); st.append(start); di.append(float(speed.min()))
    if with_cfg4:
        speed, origin, delta, dis = cfg4_field()
        sp.append(speed); og.append(origin); dl.append(delta); st.append(np.array([2300., -1000.], np.float32)); di.append(dis)
    return sp, og, dl, st, di


def plain_times(sp, og, dl, st, di):
    return [product(s, o, d, a, discard=float(q), plain=1)[0] for s, o, d, a, q in zip(sp, og, dl, st, di)]


def assert_same_bits(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "solve %d of shape %s differs" % (k, b.shape)


def test_host_batch_gives_the_plain_routines_bits_solve_by_solve():
    sp, og, dl, st, di = mixed_batch()
    shapes = {s.shape for s in sp}
    assert (1, 1) in shapes and any(s[0] == 1 and s[1] > 1 for s in shapes) and any(s[1] == 1 and s[0] > 1 for s in shapes)
    got, fb = ke.fast_marching_batch(sp, og, dl, st, di)
    assert fb == 0
    assert_same_bits(got, plain_times(sp, og, dl, st, di))
    # discards=None: every node solved
    got, fb = ke.fast_marching_batch(sp[:20], og[:20], dl[:20], st[:20])
    assert_same_bits(got, plain_times(sp[:20], og[:20], dl[:20], st[:20], [np.nan] * 20))


def test_host_batch_counts_the_solves_its_march_hands_to_the_plain_routine():
    speed = np.full((6, 9), 2000.0, np.float32)
    speed[2, 3] = 0.0
    speed[4, 6] = -1500.0
    ok = np.full((6, 9), 2000.0, np.float32)
    origin, delta, start = np.zeros(2, np.float32), np.array([100., 120.], np.float32), np.array([450., 350.], np.float32)
    got, fb = ke.fast_marching_batch([ok, speed, ok], [origin] * 3, [delta] * 3, [start] * 3)
    assert fb == 1
    assert_same_bits(got, plain_times([ok, speed, ok], [origin] * 3, [delta] * 3, [start] * 3, [np.nan] * 3))


def _raw_batch(ctx, where, nsolve, nx, ny, null=None):
    L = klib.load()
    n = max(nsolve, 1)
    nxa, nya = np.array(nx, np.int32), np.array(ny, np.int32)
    ofs = np.zeros(n, np.int64)
    speed = np.full(64, 1000.0, np.float32)
    two = np.ones((n, 2), np.float32)
    dis = np.full(n, np.nan, np.float32)
    times = np.zeros(64, np.float32)
    fp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    args = dict(nx=ip(nxa), ny=ip(nya), ofs=ofs.ctypes.data_as(C.POINTER(C.c_longlong)), speed=fp(speed), origin=fp(two), delta=fp(two),
                start=fp(two), discard=fp(dis), times=fp(times))
    if null:
        args[null] = None
    rc = L.kiwi_hip_fast_marching_batch(ctx, where, nsolve, args["nx"], args["ny"], args["ofs"], args["speed"], args["origin"], args["delta"],
                                        args["start"], args["discard"], args["times"], None)
    buf = C.create_string_buffer(512)
    L.kiwi_hip_last_error(ctx, buf, 512)
    return rc, buf.value.decode()


def test_argument_errors_answer_non_zero_with_a_message():
    rc, msg = _raw_batch(None, 0, 1, [4], [4])
    assert rc == 0
    for kw, word in ((dict(where=1), "context"), (dict(where=2), "where"), (dict(where=-1), "where"), (dict(nsolve=0), "at least one"),
                     (dict(nx=[0]), "grid side"), (dict(ny=[-3]), "grid side")):
        a = dict(where=0, nsolve=1, nx=[4], ny=[4])
        a.update(kw)
        rc, msg = _raw_batch(None, a["where"], a["nsolve"], a["nx"], a["ny"])
        assert rc != 0 and word in msg, (kw, rc, msg)
    for name in ("nx", "ny", "ofs", "speed", "origin", "delta", "start", "discard", "times"):
        rc, msg = _raw_batch(None, 0, 1, [4], [4], null=name)
        assert rc != 0 and "null" in msg, (name, rc, msg)
    with pytest.raises(ValueError):
        ke.fast_marching_batch([np.ones(5, np.float32)], [[0, 0]], [[1, 1]], [[0, 0]])
    with pytest.raises(ValueError):
        ke.fast_marching_batch([np.ones((2, 2), np.float32)], [[0, 0]], [[1, 1]], [[0, 0], [1, 1]])


def test_grids_whose_padded_size_exceeds_an_int_are_not_marched_on_the_int_layout():
    """The optimised host march and the device march index the padded grid (nx + 2) x (ny + 2) with int: the predicate both
    use, at the boundary.  (A thin grid passes the older nx * ny <= 2^30 test and still overflows: 2^30 x 1 pads to 3 * 2^30.)"""
    ok = ke.fast_marching_grid_ok
    assert ok(1, 1) and ok(1200, 360)
    assert ok(46338, 46338) and not ok(46339, 46339)                 # 46340^2 = 2147395600 <= INT_MAX < 46341^2
    assert not ok(2 ** 30, 1)                                        # (2^30 + 2) * 3 > INT_MAX although nx * ny = 2^30
    assert not ok(1, 2 ** 30)
    assert ok(715827880, 1) and not ok(715827881, 1)                 # (nx + 2) * 3 <= 2147483647  <=>  nx <= 715827880
    assert not ok(0, 5) and not ok(5, -1) and not ok(2 ** 40, 2 ** 40)
    for nx, ny in ((3, 7), (65535, 32765), (65536, 32768), (2 ** 31 - 3, 1), (10 ** 9, 2)):
        assert ok(nx, ny) == ((nx + 2) * (ny + 2) <= 2 ** 31 - 1), (nx, ny)


def _discretise(st, p, edt, prof, cp, cn):
    try:
        a, mo, ri = ke.discretize_eikonal(st, p, edt, prof, cp, cn)
        return ("ok", a, mo, ri)
    except KiwiHipError as e:
        return ("error", str(e))


def _staged(monkeypatch, on):
    if on:
        monkeypatch.setenv("KIWI_HIP_EIK_STAGED", "1")
    else:
        monkeypatch.delenv("KIWI_HIP_EIK_STAGED", raising=False)


def test_three_stage_discretiser_equals_the_unsplit_one(monkeypatch):
    """The parameter sets of tests/test_eikonal_golden.py (the golden cases, the two rejections, random ruptures) through the
    staged route -- prepare, a where = 0 batch of solves behind the solve cache, finish -- and through discretize_eikonal:
    same tables bit for bit (and the reference's, for the golden cases), same error texts."""
    cases = []
    for k in range(N):
        cp, cn = G["e%d_con" % k]
        cases.append((int(G["e%d_type" % k]), G["e%d_params" % k], float(G["e%d_edt" % k]), cp, cn, G["e%d_cent" % k]))
    cp, cn = G["e0_con"]
    cases.append((5, G["fail_empty_params"], 1.0, cp, cn, "Empty rupture area"))
    q = G["e%d_params" % (N - 1)].copy()
    q[10] = 3 * q[9]
    cases.append((5, q, 1.0, cp, cn, "nucleation point is outside"))
    from tests.test_eikonal_golden import _random_ruptures
    for row in _random_ruptures(40, 424242):
        st = int(row[0])
        cases.append((st, row[2:2 + (20 if st == 5 else 15)].astype(np.float32), float(row[1]), cp, cn, None))
    nok = nerr = 0
    for st, p, edt, cp, cn, want in cases:
        _staged(monkeypatch, False)
        a = _discretise(st, p, edt, G["rupture_profile"], cp, cn)
        _staged(monkeypatch, True)
        b = _discretise(st, p, edt, G["rupture_profile"], cp, cn)
        assert a[0] == b[0]
        if a[0] == "error":
            assert a[1] == b[1]
            if isinstance(want, str):
                assert want in b[1]
            nerr += 1
            continue
        assert not isinstance(want, str)
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2:] == b[2:]
        if want is not None:
            assert np.array_equal(b[1].view(np.uint32), want.view(np.uint32))
        nok += 1
    assert nok >= N + 10 and nerr >= 2


def test_staged_route_uses_the_solve_cache_like_the_unsplit_one(monkeypatch):
    """A shifted rupture takes the stored arrival times on either route: same hit and miss counts for the same list."""
    from tests.test_eikonal_golden import _cache_stats
    prof = G["rupture_profile"]
    cp, cn = G["e0_con"]
    base = np.array(G["e%d_params" % (N - 1)], np.float32)
    edt = float(G["e%d_edt" % (N - 1)])
    trials = []
    for dn in (0.0, 400.0, -800.0):
        for de in (0.0, 250.0):
            p = base.copy()
            p[1] += dn; p[2] += de
            trials.append(p)
    deeper = base.copy()
    deeper[3] += 2500.0
    trials.append(deeper)
    counts, tables = {}, {}
    for on in (False, True):
        _staged(monkeypatch, on)
        _cache_stats(reset=True)
        klib.load().kiwi_hip_eikonal_cache_stats(None, None, 3)          # (drop the stored solves too)
        tables[on] = [ke.discretize_eikonal(5, p, edt, prof, cp, cn)[0] for p in trials]
        counts[on] = _cache_stats()
    assert counts[True] == counts[False] and counts[True][0] >= len(trials) - 3
    for a, b in zip(tables[False], tables[True]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_packing_and_staged_discretiser_under_asan_and_ubsan(tmp_path):
    """The new host code -- the cache's two halves around a solve, the staged discretiser with its solves done between the
    stages -- under AddressSanitizer + UBSan on the CPU build (tests/host_sanitizers/asan_staged.cpp; g++, the product's plain
    C++ headers only)."""
    from tests.test_host_sanitizers import build_and_run
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = build_and_run(tmp_path, "asan_staged", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                      env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "asan staged run: 0 bad" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]


def test_header_loader_and_fortran_binding_cover_the_new_entries():
    names = {"kiwi_hip_fast_marching_batch", "kiwi_hip_set_eikonal_solver", "kiwi_hip_get_eikonal_solver", "kiwi_hip_get_eikonal_solver_ms",
             "kiwi_hip_get_eikonal_solver_stats", "kiwi_hip_fast_marching_grid_ok"}
    assert names <= set(klib.declared_symbols())
    L = klib.load()
    f90 = open(os.path.join(ROOT, "kiwi_amd", "fortran", "kiwi_hip_binding.f90")).read()
    for n in names:
        assert getattr(L, n).argtypes is not None
        assert "name='%s'" % n in f90
