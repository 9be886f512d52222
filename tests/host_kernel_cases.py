"""Case files for tests/host_kernels/linfit_path_host.cpp -- the kernels of `Engine.linear_fit`'s path run on the host from their
own source text under AddressSanitizer + UBSan -- and the build of that program.  Not a test module: tests/test_host_kernels.py
uses it.  A case file holds what the library is given through its setters (database, receivers, references, tapers, the
sources' parameters or centroid tables, weights, K) and the oracle's plain synthetic strips, which stand in for what the
accumulate kernel leaves behind; nothing of it is committed, the tests write it into their tmp_path."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_kernels")
INC = os.path.join(ROOT, "kiwi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = {"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
_TYPES = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.uint8): 3}
_DTYPES = {v: k for k, v in _TYPES.items()}
NO_RUNTIME = ("FATAL: ThreadSanitizer", "ReserveShadowMemoryRange failed", "Shadow memory range interleaves", "unexpected memory mapping")


def write_arrays(path, arrays):
    with open(path, "wb") as f:
        f.write(b"KHK1" + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            assert a.dtype in _TYPES and len(name) < 24, (name, a.dtype)
            f.write(name.encode().ljust(24, b"\0") + struct.pack("<IQ", _TYPES[a.dtype], a.size) + a.tobytes())


def read_arrays(path):
    out = {}
    with open(path, "rb") as f:
        assert f.read(4) == b"KHK1"
        for _ in range(struct.unpack("<I", f.read(4))[0]):
            name = f.read(24).rstrip(b"\0").decode()
            t, n = struct.unpack("<IQ", f.read(12))
            dt = _DTYPES[t]
            out[name] = np.frombuffer(f.read(n * dt.itemsize), dt).copy()
    return out


def build(where, sanitize=True):
    """the program, built the way tests/test_host_sanitizers.py builds its own: the path of the executable, or a skip where this
    machine has no compiler or no sanitizer runtime.  sanitize=False: a plain -O0 build (seconds), for a comparison of results"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = os.path.join(str(where), "linfit_path_host")
    cmd = [cxx, "-O1" if sanitize else "-O0", "-g", "-std=c++17", "-fno-fast-math", "-ffp-contract=off", "-fno-omit-frame-pointer", "-pthread", "-I", SRC, "-I", INC] + \
        (SANITIZE if sanitize else []) + ["-o", exe, os.path.join(SRC, "linfit_path_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and ("cannot find -l" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this compiler has no AddressSanitizer runtime")
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, case_path, out_path, short=None):
    """the program on one case file: the CompletedProcess; a sanitizer runtime that cannot start here is a skip, not a finding"""
    cmd = [exe, str(case_path), str(out_path)] + (["--short", short] if short else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **ENV))
    if r.returncode != 0 and any(m in r.stderr for m in NO_RUNTIME):
        pytest.skip("the sanitizer runtime does not start here: " + r.stderr.strip().splitlines()[0][:120])
    return r


def is_clean(r):
    return r.returncode == 0 and "linfit path host run: clean" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr and "AUDIT" not in r.stderr


def oracle_strips(e, comps, enabled, set_source, rows):
    """the oracle's plain displacement strips (before moment, rise-time fold and taper: what the accumulate kernel makes) of every
    (source, slot of an enabled receiver): (first [n], offsets [n + 1], data)"""
    first, ofs, data = [], [0], []
    for row in np.atleast_2d(rows):
        set_source(e, row)
        e.calculate_seismograms()
        for ir, c in enumerate(comps):
            if not enabled[ir]:
                continue
            for k in range(len(c)):
                lo, d = e.displacement(ir + 1, k + 1)
                first.append(lo)
                data.append(np.asarray(d, np.float32))
                ofs.append(ofs[-1] + len(d))
    return np.array(first, np.int32), np.array(ofs, np.int32), (np.concatenate(data) if data else np.zeros(0)).astype(np.float32)


def case_arrays(sc, e, rows, K, set_source, sourcetype="moment_tensor", tables=None, enabled=None, weights=None, anarchy=False, factor=1.0,
                undersampling=(1, 1), expect_window=None):
    """the arrays of one case.  sc: the Scenario (its references and tapers set); e: an oracle engine of that scenario with every
    receiver enabled, from which the strips are taken; rows: the sources' parameter rows; tables: for the types the program does
    not discretise itself, (cent [n, 10], cent_ofs [nsrc + 1], moment [nsrc], risetime [nsrc])"""
    nrec = sc.nrec
    enabled = [True] * nrec if enabled is None else list(enabled)
    first, nsamp, data = sc.odb.dense_tables()
    g = sc.gf
    comps = np.zeros((nrec, 8), np.uint8)
    for ir, c in enumerate(sc.comps):
        comps[ir, :len(c)] = np.frombuffer(c.encode(), np.uint8)
    ref_first, ref_ofs, ref_data, tofs, tx, ty = [], [0], [], [0], [], []
    for ir, c in enumerate(sc.comps):
        for k in range(len(c)):
            lo, d = sc.refs[(ir + 1, k + 1)]
            ref_first.append(lo)
            ref_data.append(np.asarray(d, np.float32))
            ref_ofs.append(ref_ofs[-1] + len(d))
        x, y = sc.tapers.get(ir + 1, ([], []))
        tx += list(x)
        ty += list(y)
        tofs.append(len(tx))
    sf, so, sd = oracle_strips(e, sc.comps, enabled, set_source, rows)
    a = dict(gf_dims=np.array(list(data.shape[:3]) + [data.shape[3]], np.int32),
             gf_meta=np.array([g["dt"], g["dx"], g["dz"], g["firstx"], g["firstz"]], np.float32),
             gf_data=data.astype(np.float32), gf_first=first.astype(np.int32), gf_nsamp=nsamp.astype(np.int32),
             interp=np.array([int(sc.bilinear), undersampling[0], undersampling[1]], np.int32), origin=np.array([40.0, 30.0], np.float32),
             rec_lat=np.asarray(sc.lat, np.float64), rec_lon=np.asarray(sc.lon, np.float64), rec_depth=np.asarray(sc.depth, np.float32),
             rec_comps=comps, rec_enabled=np.array([int(v) for v in enabled], np.int32),
             ref_first=np.array(ref_first, np.int32), ref_ofs=np.array(ref_ofs, np.int32), ref_data=np.concatenate(ref_data).astype(np.float32),
             taper_ofs=np.array(tofs, np.int32), taper_x=np.array(tx, np.float32), taper_y=np.array(ty, np.float32),
             fit=np.array([K, int(anarchy)], np.int32), syn_factor=np.array([factor], np.float32),
             strip_first=sf, strip_ofs=so, strip_data=sd)
    if weights is not None:
        a["weights"] = np.asarray(weights, np.float64)
    if sourcetype == "moment_tensor":
        a.update(sourcetype=np.array([6], np.int32), params=np.ascontiguousarray(rows, np.float32), effective_dt=np.array([sc.effective_dt], np.float32))
    else:
        cent, cent_ofs, moment, risetime = tables
        a.update(sourcetype=np.array([5], np.int32), cent=np.ascontiguousarray(cent, np.float32), cent_ofs=np.asarray(cent_ofs, np.int32),
                 moment=np.asarray(moment, np.float32), risetime=np.asarray(risetime, np.float32))
    if expect_window is not None:
        a["expect_window"] = np.array(expect_window, np.int32)
    return a


def traces_of(res, nsrc, K):
    """the program's kept tapered traces and tapered references in the layout tests/linfit_restatement.py takes:
    (syn[slot] [ngroup, K, wlen], ref[slot] [wlen])"""
    syn, ref, a, b = [], [], 0, 0
    for wl in res["slot_wlen"]:
        syn.append(res["proc"][a:a + nsrc * wl].reshape(nsrc // K, K, wl))
        ref.append(res["reft"][b:b + wl])
        a += nsrc * wl
        b += wl
    return syn, ref
