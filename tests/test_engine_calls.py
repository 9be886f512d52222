"""What kiwi_amd/engine.py hands to the library for the 15 group families, without a device and without the library: the real
`Engine` methods run against a recording stand-in, and every call they make -- the function, every argument, which output array sits
in which place --, what they return, what they refuse and what they leave in `nsrc` is compared with tests/golden/engine_calls.json.
The fixture was recorded with this module's `record()` from the engine.py and lib.py BEFORE the group methods were folded onto
shared helpers (`python tests/test_engine_calls.py FILE` writes one), so the test passes against that tree and this one alike: the
binding moved nothing.  The last test pins the `argtypes` the loader derives to the lists that were typed out there."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from kiwi_amd import engine as ke  # noqa: E402
from kiwi_amd import lib as klib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_calls.json")
MAX_BASIS, WIDE_MAX_BASIS = 8, 64             # linfit::kMaxBasis, linfit::kWideMaxBasis (kiwi_amd/csrc/kiwi_linfit.hpp)
NPARAMS = {6: 11}                             # moment_tensor (kiwi_hip_source_nparams)
LAST_ERROR = "the stand-in refuses"
ISRC0, NGROUP, NCAND, NDRAW, PIECE, BINS, HELD, NSRC = 3, 2, 5, 4, 7, 6, 4, 9
SCAN = dict(k0=-2, kstep=3, nk=4)
COMPONENTS, ENABLED = ["ned", "d", "ne"], [True, False, True]      # nrec = 3, nmis = 5

# family -> (K, does it take candidates / draw_weights / the offsets / outer_norm / free_scale, its optional outputs, its further
# arguments with every output on, the same with every output off)
FAMILIES = {
    "linear_fit": (3, "", ["normal", "by_receiver"], {}, {}),
    "linear_fit_time_scan": (3, "s", ["normal"], {}, {}),
    "linear_fit_robust": (3, "n", [], dict(niter=5, eps=0.25), {}),
    "linear_fit_wide": (10, "", ["normal", "by_receiver"], dict(nonneg=True, penalty="matrix", penalty_relative=True),
                        dict(nonneg=2, penalty="triangle")),
    "linear_fit_candidates": (3, "cnf", ["misfit", "receiver_misfit"], {}, {}),
    "linear_fit_candidates_time_scan": (3, "csnf", ["marginal", "misfit", "receiver_misfit"], {}, {}),
    "linear_fit_candidates_bootstrap": (3, "cdsn", ["per_group"], {}, {}),
    "linear_fit_candidates_floating": (3, "cnf", ["misfit", "cand_shift", "receiver_misfit"], {}, {}),
    "linear_fit_candidates_floating_bootstrap": (3, "cdn", ["per_group"], {}, {}),
    "spectral_candidates": (3, "cnf", ["misfit", "slot_misfit", "spectra"], dict(spectra_bins=BINS), {}),
    "spectral_candidates_bootstrap": (3, "cdn", ["per_group"], {}, {}),
    "waveform_candidates": (3, "cn", ["misfit", "slot_misfit"], {}, {}),
    "waveform_candidates_floating": (3, "cn", ["misfit", "cand_shift", "slot_misfit"], {}, {}),
    "waveform_candidates_time_scan": (3, "csn", ["cand_misfit", "cand_offset", "misfit", "slot_misfit", "rows"], {}, {}),
    "waveform_candidates_bootstrap": (3, "cdsn", ["per_group"], {}, {}),
}


def _hash(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:8]


def _describe(v):
    """a returned value as JSON: arrays as [dtype, shape, hash], tuples field by field"""
    if isinstance(v, np.ndarray):
        return [str(v.dtype), list(v.shape), _hash(v)]
    if isinstance(v, tuple):
        return {f: _describe(x) for f, x in zip(v._fields, v)} if hasattr(v, "_fields") else [_describe(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


class StandIn:
    """The library as engine.py sees it.  It answers what the Python layer asks before it calls (parameter counts, basis limits,
    source statuses, the shape calls, the error text) and records every other call; an array it is handed that holds nothing but
    zeros is an output and is filled with -1, 0, 1, ... (the inputs of the cases have no zero row)."""

    def __init__(self, handle):
        self.h, self.calls, self.rc, self.shape_rc, self.held = handle, [], 0, 0, HELD

    def __getattr__(self, name):
        if not name.startswith("kiwi_hip_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        arrays = [a._arr for a in args if isinstance(a, C._Pointer)]
        if name == "kiwi_hip_source_nparams":
            return NPARAMS.get(args[0], -1)
        if name == "kiwi_hip_linear_fit_max_basis":
            return MAX_BASIS
        if name == "kiwi_hip_linear_fit_wide_max_basis":
            return WIDE_MAX_BASIS
        if name == "kiwi_hip_get_source_status":
            return 0 if args[1] + args[2] <= self.held else 1
        if name == "kiwi_hip_last_error":
            args[1].value = LAST_ERROR.encode()
            return 0
        if name.endswith("_shape"):
            for j, a in enumerate(arrays):
                a[...] = 11 + j
            return self.shape_rc
        if name == "kiwi_hip_waveform_candidates_time_scan_rows":
            arrays[0][...], arrays[1][...], arrays[2][...] = 2, 17, 3 * np.arange(len(arrays[2])) + 1
            return self.shape_rc
        rec = []
        for a in args:
            if a is self.h:
                rec.append("h")
            elif isinstance(a, C._Pointer):
                rec.append((type(a).__name__, a._arr.ctypes.data, [str(a._arr.dtype), list(a._arr.shape), _hash(a._arr)]))
            else:
                assert a is None or type(a) in (int, float), (name, a)
                rec.append(a)
        self.calls.append([name] + rec)
        for a in arrays:
            if not a.any():
                a.reshape(-1)[:] = np.arange(a.size) - 1
        return self.rc

    def resolved(self, result):
        """the calls with every pointer named: `out.<field>` where it points at a field of the returned tuple, else the array"""
        named = zip(result._fields, result) if hasattr(result, "_fields") else ()
        fields = {x.ctypes.data: "out." + f for f, x in named if isinstance(x, np.ndarray)}
        return [[a if not isinstance(a, tuple) else [a[0], fields[a[1]]] if a[1] in fields else [a[0]] + a[2] for a in call]
                for call in self.calls]


def _engine():
    e = ke.Engine.__new__(ke.Engine)
    e.h = C.c_void_p(0x5EED)
    e.L = StandIn(e.h)
    e.nsrc, e.components, e.enabled, e.misfit_method = NSRC, list(COMPONENTS), list(ENABLED), "l2norm"
    return e


def _run(method, *args, rc=0, shape_rc=0, **kw):
    """one case: a fresh engine, one method call, its record"""
    e = _engine()
    e.L.rc, e.L.shape_rc = rc, shape_rc
    out = {}
    try:
        result = getattr(e, method)(*args, **kw)
        out["result"] = _describe(result)
    except Exception as err:      # noqa: BLE001  (whatever it raises is part of the record)
        result = None
        out["error"] = [type(err).__name__, str(err)]
    out["calls"], out["nsrc"] = e.L.resolved(result), e.nsrc
    e.h = None
    return out


def _params(rows, ncol=11):
    return (np.arange(rows * ncol, dtype=np.float32) + 1).reshape(rows, ncol)


def _arguments(family, on, **change):
    """the keyword arguments of a family's two calls after (isrc0, ngroup, K) / (sourcetype, params, K)"""
    K, has, flags, extra_on, extra_off = FAMILIES[family]
    kw = {f: on for f in flags}
    kw.update(extra_on if on else extra_off)
    if kw.get("penalty") == "matrix":
        kw["penalty"] = np.add.outer(np.arange(K), np.arange(K)) + 1.0
    elif kw.get("penalty") == "triangle":
        kw["penalty"] = np.arange(K * (K + 1) // 2) + 1.0
    if "c" in has:      # float64 [ncand, K] as it is taken, float32 rows that are converted
        kw["candidates"] = 0.5 * (np.arange(NCAND * K) + 1).reshape(NCAND, K) if on else [list(r) for r in _params(NCAND, K)]
    if "d" in has:
        kw["draw_weights"] = (np.arange(NDRAW * 3) + 1.0).reshape(NDRAW, 3)
    if "s" in has:
        kw.update(SCAN)
    if "n" in has and on:
        kw["outer_norm"] = "l2norm"
    if "f" in has:
        kw["free_scale"] = on
    kw["anarchy"] = on
    kw["receiver_weights"] = [1.0, 0.5, 2.0] if on else None
    kw.update(change)
    return K, kw


def record():
    """every case of the fixture from the kiwi_amd on the path: {case: record}"""
    out = {}
    for family, (K, has, flags, _, _) in FAMILIES.items():
        kmax = WIDE_MAX_BASIS if family == "linear_fit_wide" else MAX_BASIS

        def both(case, on=False, K=K, rows=None, ncol=11, **change):
            """the uploaded call and the list call with the same further arguments"""
            k, kw = _arguments(family, on, **change)
            rc = {key: kw.pop(key) for key in ("rc", "shape_rc") if key in kw}
            if rows is None:
                out["%s/%s" % (family, case)] = _run(family, ISRC0, NGROUP, K, **kw, **rc)
            nrow = NGROUP * (K or 3) if rows is None else rows
            out["%s_params/%s" % (family, case)] = _run(family + "_params", "moment_tensor", _params(nrow, ncol), K, piece=PIECE, **kw, **rc)

        both("on", True)
        both("off")
        both("scalar weight", receiver_weights=0.25)
        both("the library fails", rc=1)
        both("K = 0", K=0)
        both("K = max + 1", K=kmax + 1)
        both("ragged list", rows=NGROUP * K + 1)
        both("empty list", rows=0)
        both("wrong parameter count", rows=NGROUP * K, ncol=10)
        if "n" in has:
            both("unknown outer_norm", outer_norm="l3norm")
        if "c" in has:
            both("candidates of the wrong width", candidates=np.ones((NCAND, K + 1)))
        if "d" in has:
            both("draw_weights of the wrong width", draw_weights=np.ones((NDRAW, 4)))
            both("draw_weights of the wrong rank", draw_weights=np.ones(3))
        if family == "linear_fit_wide":
            asym = np.add.outer(np.arange(K), 2.0 * np.arange(K))
            both("penalty not symmetric", penalty=asym)
            both("penalty of the wrong shape", penalty=np.ones(K))
        if family == "spectral_candidates":
            both("spectra sized by the engine", True, spectra_bins=None)
        if family == "waveform_candidates_time_scan":
            both("the rows call fails", True, shape_rc=1)
        out[family + "_ms"] = _run(family + "_ms")
        out[family + "_ms/the library fails"] = _run(family + "_ms", rc=1)
        if hasattr(ke.Engine, family + "_shape"):
            out[family + "_shape"] = _run(family + "_shape", K)
            out[family + "_shape/refused"] = _run(family + "_shape", kmax + 1, shape_rc=1)
    out["spectral_candidates_shape/no context"] = _run("spectral_candidates_shape", 3, context=False)
    out["waveform_candidates_time_scan_rows"] = _run("waveform_candidates_time_scan_rows", **SCAN)
    for name in ("outer_ms", "band_misfits_ms", "time_scan_ms", "linear_fit_max_basis", "linear_fit_wide_max_basis"):
        out[name] = _run(name)
    return out


def argtypes(L):
    """the argument types of the three entry points of every family, as names"""
    names = [fmt % f for f in FAMILIES for fmt in ("kiwi_hip_%s", "kiwi_hip_%s_params", "kiwi_hip_get_%s_ms")]
    return {n: [t.__name__ for t in getattr(L, n).argtypes] for n in names}


def _dump(cases, types):
    """compact JSON, one case per line"""
    line = lambda d: ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in d.items())      # noqa: E731
    return '{"cases":{\n%s\n},"argtypes":{\n%s\n}}\n' % (line(cases), line(types))


def _family(case):
    """the family whose test compares a case; None: the test of the others"""
    head = case.split("/")[0]
    return next((f for f in FAMILIES if head in (f, f + "_params", f + "_ms", f + "_shape")), None)


def _first_difference(got, want, where=""):
    if type(got) is not type(want):
        return "%s: %r, recorded %r" % (where, got, want)
    if isinstance(got, dict):
        for k in list(want) + [k for k in got if k not in want]:
            if k not in got or k not in want:
                return "%s: %s only %s" % (where, k, "recorded" if k in want else "here")
            d = _first_difference(got[k], want[k], "%s %s" % (where, k))
            if d:
                return d
    elif isinstance(got, list) and where.endswith(" calls"):
        if [c[0] for c in got] != [c[0] for c in want]:
            return "%s: %r, recorded %r" % (where, [c[0] for c in got], [c[0] for c in want])
        for i, (g, w) in enumerate(zip(got, want)):
            if len(g) != len(w):
                return "%s: call %d %s: %d arguments, recorded %d" % (where, i, g[0], len(g) - 1, len(w) - 1)
            for j in range(1, len(g)):
                if g[j] != w[j]:
                    return "%s: call %d %s: argument %d: %r, recorded %r" % (where, i, g[0], j - 1, g[j], w[j])
    elif got != want:
        return "%s: %r, recorded %r" % (where, got, want)
    return None


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def here():
    return json.loads(json.dumps(record()))


def test_the_fixture_has_exactly_the_recorders_cases(recorded, here):
    assert sorted(recorded["cases"]) == sorted(here)


@pytest.mark.parametrize("family", list(FAMILIES) + ["others"])
def test_every_call_result_refusal_and_nsrc_is_the_recorded_one(recorded, here, family):
    mine = [c for c in here if _family(c) == (None if family == "others" else family)]
    assert mine
    diffs = [d for d in (_first_difference(here[c], recorded["cases"][c], "case '%s'" % c) for c in mine) if d]
    assert not diffs, "\n".join(diffs)


def test_a_failed_list_call_leaves_no_batch_and_a_failed_uploaded_call_leaves_it(here):
    for family in FAMILIES:
        up, lst = here["%s/the library fails" % family], here["%s_params/the library fails" % family]
        for r in (up, lst):
            assert r["error"] == ["KiwiHipError", "%s: nok > %s" % (family, LAST_ERROR)], (family, r["error"])
        assert up["nsrc"] == NSRC and lst["nsrc"] == 0, family
        assert here["%s_params/on" % family]["nsrc"] == HELD, family


def test_the_fill_reaches_the_offsets_the_spectral_bootstrap_makes_up(here):
    r = here["spectral_candidates_bootstrap/on"]["result"]
    cand, group = np.arange(NDRAW) - 1, np.arange(NGROUP * NDRAW).reshape(NGROUP, NDRAW) - 1
    assert r["best_offset"] == _describe(np.where(cand >= 0, 0, -1).astype(np.int32))
    assert r["group_offset"] == _describe(np.where(group >= 0, 0, -1).astype(np.int32))


def test_derived_argtypes_are_the_typed_out_ones(recorded):
    got = argtypes(klib.load())
    for name, want in recorded["argtypes"].items():
        assert got[name] == want, name
    assert sorted(got) == sorted(recorded["argtypes"])


if __name__ == "__main__":
    open(sys.argv[1], "w").write(_dump(record(), argtypes(klib.load())))
