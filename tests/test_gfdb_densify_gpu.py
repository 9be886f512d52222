"""set_database dbpath nipx nipz on the device (kiwi_amd/csrc/kiwi_gfk.hpp): the densified database against the CPU
restatement (tests/gfk_restatement.py) bit for bit, misfits through it against the oracle, the Fortran host's parsing,
and a multi-device context."""
import numpy as np
import pytest

from kiwi_amd import synthetic
from tests import gfk_restatement as R
from tests.common import HAVE_FLANG, HAVE_HDF5, Scenario, misfit_close, oracle_misfits

pytestmark = pytest.mark.gpu


def small_gf(variant="probe", ng=8, nx=12, nz=4, missing=False):
    gf = synthetic.make_gfdb(nx=nx, nz=nz, ng=ng, L=160, center=70.0, width=25.0, variant=variant)
    if variant == "static":
        gf["data"][..., 150:] = gf["data"][..., 149:150]
    if missing:
        gf["nsamp"][3, 1, :] = 0
        gf["nsamp"][7, 2, ng - 1] = 0
        gf["nsamp"][0, 0, 2] = 0
    return gf


def installed(p):
    nx, nz, ng, maxlen, dx, dz = p.database_shape()
    first = np.zeros((nx, nz, ng), np.int32)
    nsamp = np.zeros((nx, nz, ng), np.int32)
    data = np.zeros((nx, nz, ng, max(maxlen, 1)), np.float32)
    for ix in range(nx):
        for iz in range(nz):
            for ig in range(ng):
                f, d = p.get_database_trace(ix, iz, ig)
                first[ix, iz, ig], nsamp[ix, iz, ig] = f, len(d)
                data[ix, iz, ig, :len(d)] = d
    return dict(first=first, nsamp=nsamp, data=data, dx=dx, dz=dz)


def assert_same_database(got, want):
    assert got["data"].shape[:3] == want["data"].shape[:3]
    assert np.array_equal(got["nsamp"], want["nsamp"])
    on = want["nsamp"] > 0
    assert np.array_equal(got["first"][on], want["first"][on])
    bad = []
    for idx in zip(*np.nonzero(on)):
        n = want["nsamp"][idx]
        if not np.array_equal(got["data"][idx][:n], want["data"][idx][:n]):
            bad.append(idx)
    assert not bad, "%d traces differ, first %s" % (len(bad), bad[:5])


CASES = [((2, 1), "probe", 8, False), ((1, 2), "probe", 10, True), ((2, 2), "static", 8, True), ((4, 4), "probe", 8, False),
         ((8, 8), "probe", 10, False), ((2, 4), "static", 10, False), ((4, 2), "probe", 8, True)]


@pytest.mark.exact_only
@pytest.mark.parametrize("factors,variant,ng,missing", CASES)
def test_densified_database_is_the_restatement_bit_for_bit(factors, variant, ng, missing):
    from kiwi_amd import Engine
    gf = small_gf(variant, ng, missing=missing)
    want = R.densify(gf, *factors)
    p = Engine(0)
    p.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"],
                   nipx=factors[0], nipz=factors[1])
    got = installed(p)
    assert got["dx"] == want["dx"] and got["dz"] == want["dz"]
    assert_same_database(got, want)
    # stored traces are the input
    nipx, nipz = factors
    st = got["nsamp"][::nipx, ::nipz]
    assert np.array_equal(st, gf["nsamp"])
    for idx in zip(*np.nonzero(gf["nsamp"] > 0)):
        n = gf["nsamp"][idx]
        assert np.array_equal(got["data"][idx[0] * nipx, idx[1] * nipz, idx[2], :n], gf["data"][idx][:n])
    p.close()


def test_factors_of_one_are_plain_set_database():
    from kiwi_amd import Engine
    gf = small_gf("static", 10, missing=True)
    a, b = Engine(0), Engine(0)
    args = (gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    a.set_database(*args)
    from kiwi_amd.engine import _fp, _ip
    nx, nz, ng, L = gf["data"].shape
    b._ck(b.L.kiwi_hip_set_gfdb_interpolated(b.h, 1, 1, nx, nz, ng, L, gf["dt"], gf["dx"], gf["dz"], gf["firstx"],
                                             gf["firstz"], _fp(gf["data"]), _ip(gf["first"]), _ip(gf["nsamp"])), "x")
    assert_same_database(installed(b), installed(a))
    assert a.database_shape() == b.database_shape()
    a.close()
    b.close()


@pytest.mark.exact_only
def test_zero_noise_floor_field_is_finite_and_the_restatement():
    # a band-limited field whose decimated row T/2 is exactly zero (m == 0): the bins where fC/fD is undefined get no
    # operator, on the device as in the restatement (tests/test_gfdb_densify.py builds the same field on the CPU)
    from kiwi_amd import Engine
    gf = synthetic.make_gfdb(nx=2, nz=12, ng=8, L=256, center=90.0, width=30.0, vel=6000.0, dx=2000.0)
    gf = dict(gf, data=gf["data"][:, ::2].copy(), first=gf["first"][:, ::2].copy(), nsamp=gf["nsamp"][:, ::2].copy())
    want = R.densify(gf, 1, 2)
    assert np.all(np.isfinite(want["data"]))
    p = Engine(0)
    p.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"],
                   nipx=1, nipz=2)
    got = installed(p)
    assert_same_database(got, want)
    assert np.all(np.isfinite(got["data"]))
    p.close()


def test_non_finite_interpolation_is_refused():
    from kiwi_amd import Engine, KiwiHipError
    gf = small_gf()
    gf["data"][5, 1, 0, 40] = np.nan
    p = Engine(0)
    with pytest.raises(KiwiHipError, match="non-finite sample"):
        p.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"],
                       nipx=2, nipz=1)
    p.close()


@pytest.mark.skipif(not HAVE_HDF5, reason="HDF5 reader not built")
def test_hdf5_reader_feeds_the_same_call(tmp_path):
    from kiwi_amd import Engine, gfdb_hdf5
    gf = small_gf("static", 10)
    base = str(tmp_path / "db")
    gfdb_hdf5.write(base, gf, nchunks=3)
    a, b = Engine(0), Engine(0)
    got = gfdb_hdf5.set_database(a, base, nipx=2, nipz=2)
    b.set_database(got["dt"], got["dx"], got["dz"], got["firstx"], got["firstz"], got["data"], got["first"], got["nsamp"],
                   nipx=2, nipz=2)
    assert a.database_shape()[:3] == (24, 8, 10)
    assert_same_database(installed(a), installed(b))
    a.close()
    b.close()


def test_bad_factors_are_refused():
    from kiwi_amd import Engine, KiwiHipError
    gf = small_gf()
    p = Engine(0)
    args = (gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], gf["data"], gf["first"], gf["nsamp"])
    with pytest.raises(KiwiHipError, match="nipx and nipz must be positive"):
        p.set_database(*args, nipx=0, nipz=1)
    with pytest.raises(KiwiHipError, match="power of two"):
        p.set_database(*args, nipx=3, nipz=1)


def _densified_scenario_misfits(p_factory):
    sc = Scenario(nrec=4)
    e = sc.oracle()
    sc.make_references(e)
    first, nsamp, data = sc.odb.dense_tables()
    g = sc.gf
    p = p_factory()
    p.set_database(g["dt"], g["dx"], g["dz"], g["firstx"], g["firstz"], data, first, nsamp, nipx=2, nipz=2)
    dense = installed(p)
    # the CPU oracle over the downloaded dense traces
    from oracle import ko
    nx, nz, ng = dense["nsamp"].shape
    db = ko.Gfdb(nx, nz, ng, g["dt"], dense["dx"], dense["dz"], g["firstx"], g["firstz"])
    for idx in zip(*np.nonzero(dense["nsamp"] > 0)):
        n = dense["nsamp"][idx]
        db.set_trace(idx[0] + 1, idx[1] + 1, idx[2] + 1, int(dense["first"][idx]), dense["data"][idx][:n])
    o = ko.Engine(db)
    o.set_receivers(sc.lat, sc.lon, sc.depth, sc.comps)
    o.set_source_location(40.0, 30.0, 0.0)
    o.set_effective_dt(sc.effective_dt)
    o.set_interpolation(True, 2, 2)
    sc.apply_setup(o, True)
    p.set_receivers(sc.lat, sc.lon, sc.depth, sc.comps)
    p.set_source_location(40.0, 30.0, 0.0)
    p.set_effective_dt(sc.effective_dt)
    p.set_local_interpolation("bilinear")
    p.set_spacial_undersampling(2, 2)
    sc.apply_setup(p, False)
    trials = synthetic.bilat_strike_sweep(4, step=1.5)
    m, n, gl = oracle_misfits(o, 1, trials)
    p.set_source_params("bilateral", trials)
    p.eval()
    pm, pn, pg = p.get_misfits()
    assert misfit_close(pm, m, norm=n)
    assert misfit_close(pg, gl, glob=True)
    return pm


def test_misfits_through_the_densified_database_match_the_oracle():
    from kiwi_amd import Engine
    _densified_scenario_misfits(lambda: Engine(0))


def test_multi_device_context_gives_the_same_misfits():
    from kiwi_amd import Engine
    a = _densified_scenario_misfits(lambda: Engine(0))
    b = _densified_scenario_misfits(lambda: Engine(0, ndev=1))
    assert np.array_equal(a, b)


@pytest.mark.skipif(not HAVE_FLANG, reason="amdflang not installed")
def test_fortran_host_set_database_factors(tmp_path):
    from kiwi_amd import Engine, protocol
    sc = Scenario(nrec=3)
    e = sc.oracle()
    sc.make_references(e)
    first, nsamp, data = sc.odb.dense_tables()
    gf = dict(sc.gf)
    gf.update(first=first, nsamp=nsamp, data=data)
    base = str(tmp_path / "db")
    protocol.write_flat_gfdb(base, gf)
    protocol.write_receivers(str(tmp_path / "receivers.table"), sc.lat, sc.lon, sc.comps)
    trial = synthetic.bilat_strike_sweep(1, step=1.5)[0]
    # the Python face of the same call: misfits through the densified database, references = coarse synthetics
    py = Engine(0)
    py.set_database(gf["dt"], gf["dx"], gf["dz"], gf["firstx"], gf["firstz"], data, first, nsamp, nipx=2, nipz=2)
    py.set_receivers(sc.lat, sc.lon, sc.depth, sc.comps)
    py.set_source_location(40.0, 30.0, 0.0)
    py.set_effective_dt(sc.effective_dt)
    py.set_local_interpolation("bilinear")
    sc.apply_setup(py, False)
    py.set_source_params("bilateral", trial[None, :])
    py.eval()
    want = py.get_misfits()[0][0]
    p = protocol.MinimizerProcess(protocol.build_host())
    try:
        for bad, msg in (("0 1", "nipx and nipz must be positive"), ("3 1", "power of two"), ("2 x", "failed to parse")):
            with pytest.raises(protocol.SeismosizerReturnedError, match=msg):
                p.do("set_database", base, *bad.split())

        def run(*extra):
            p.do("set_database", base, *extra)
            p.do("set_effective_dt", sc.effective_dt)
            p.do("set_local_interpolation", "bilinear")
            p.do("set_receivers", str(tmp_path / "receivers.table"))
            p.do("set_source_location", 40.0, 30.0, 0.0)
            for (ir, k), (lo, d) in sc.refs.items():
                protocol.write_table(str(tmp_path / ("ref-%d-%s.table" % (ir, sc.comps[ir - 1][k - 1]))),
                                     (lo - 1) * gf["dt"], gf["dt"], d)
            p.do("set_ref_seismograms", str(tmp_path / "ref"), "table")
            for ir, (x, y) in sc.tapers.items():
                p.do("set_misfit_taper", ir, *[v for xy in zip(x, y) for v in xy])
            p.do("set_source_params", "bilateral", *["%.9g" % v for v in trial])
            return np.array(p.do("get_misfits").split(), np.float64)[0::2]
        dense = run("2", "2")
        coarse = run()
        if HAVE_HDF5:          # the reference's own database format through the host's other reader
            from kiwi_amd import gfdb_hdf5
            hbase = str(tmp_path / "hdb")
            gfdb_hdf5.write(hbase, gf, nchunks=2)
            base = hbase
            dense_h5 = run("2", "2")
            assert p.do("get_database_format") == "hdf5"
            assert np.allclose(dense_h5, dense, rtol=1e-6, atol=0)
    finally:
        p.close()
        py.close()
    # the references went through a text file (9 significant digits)
    assert np.allclose(dense, want, rtol=2e-5, atol=1e-6 * np.abs(want).max())
    assert not np.allclose(dense, coarse, rtol=1e-6, atol=0)
