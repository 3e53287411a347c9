"""The GLM parallax correction on the GPU (tf_glm_parallax, tf_ecef, tf_geos_to_ecef of csrc/geodesy.hip through
tobac_flow_amd.geo / _lmatools / glm) against the mpmath oracles of tests/glm_parallax_cases.py.  One element per lane in
every kernel, so the counts are those around one wave and into a second workgroup; the 65 oracle cases are reused by index
modulo n, and every repeat must give the bits of its first occurrence.  The oracle results are cached per session."""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import geodesy_cases as gc
import glm_parallax_cases as pc
from tobac_flow_amd import _lmatools, geo, glm

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def dev(lib, a, dtype=np.float64):
    return lib.torch().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(lib.device())


def host(v):
    return v.cpu().numpy()


def on_device(lib, *tensors):
    return all(isinstance(v, lib.torch().Tensor) and v.is_cuda for v in tensors)


def goes_ds():
    return gc.AbiLike(*gc.scan_grid(3, 3))


def systems(sweep="x"):
    return (geo.GeosProj(gc.H_GOES, pc.LON_0, sweep=sweep), geo.GeosProj(gc.H_GOES, pc.LON_0, sweep=sweep, a=pc.LTG_RE, rf=pc.LTG_RF))


def check_repeats(pick, m, *outputs):
    """every repeated case carries the bits of its first occurrence, wherever it sits in the array"""
    for v in outputs:
        assert np.array_equal(v, v[:m][pick], equal_nan=True)


# ---- tf_glm_parallax -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_parallax_against_the_oracle(lib, n):
    """float64 in, all four outputs: within 2^-46 rad of the oracle; beyond the limb NaN offsets and +inf scan angles"""
    lat, lon, chain = pc.flashes()
    m = min(n, lat.size)
    pick = np.arange(n) % lat.size
    grid, ltg = systems()
    out = geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat[pick]), dev(lib, lon[pick]))
    assert on_device(lib, *out) and all(tuple(v.shape) == (n,) and v.dtype == lib.torch().float64 for v in out)
    dlon, dlat, x, y = (host(v) for v in out)
    check_repeats(pick, m, dlon, dlat, x, y)
    ok = pc.resolved(chain)[:m]
    assert np.array_equal(np.isnan(dlon[:m]), ~ok) and np.array_equal(np.isnan(dlat[:m]), ~ok)
    assert np.isposinf(x[:m][~ok]).all() and np.isposinf(y[:m][~ok]).all() and not np.isnan(x).any()
    err = pc.chain_errors(chain[:m], dlon, dlat, x, y)
    print("chain errors (rad): dlon, dlat, x, y", n, err)
    assert (err <= gc.VIEW_TOL).all()
    if n > pc.SUBSATELLITE:
        assert (dlon[pc.SUBSATELLITE], dlat[pc.SUBSATELLITE], x[pc.SUBSATELLITE], y[pc.SUBSATELLITE]) == (0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("n", COUNTS)
def test_parallax_float32_and_output_pairs(lib, n):
    """float32 in equals the same values in float64 bit for bit; the offsets alone and the scan angles alone equal the
    four-output launch; inputs and outputs that start 8 bytes past a 16-byte boundary give the same bits (the kernel has
    no wide-store form: this pins that it needs no alignment beyond the element's)"""
    t = lib.torch()
    lat, lon, _ = pc.flashes()
    pick = np.arange(n) % lat.size
    lat32, lon32 = lat[pick].astype(np.float32), lon[pick].astype(np.float32)
    grid, ltg = systems()
    want = [host(v) for v in geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat32.astype(np.float64)), dev(lib, lon32.astype(np.float64)))]
    got = geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat32, np.float32), dev(lib, lon32, np.float32))
    assert all(v.dtype == t.float64 for v in got)
    assert all(np.array_equal(host(a), b, equal_nan=True) for a, b in zip(got, want))
    only = geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat32, np.float32), dev(lib, lon32, np.float32), scan_angles=False)
    assert only[2] is None and only[3] is None and all(np.array_equal(host(a), b, equal_nan=True) for a, b in zip(only[:2], want[:2]))
    only = geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat32, np.float32), dev(lib, lon32, np.float32), offsets=False)
    assert only[0] is None and only[1] is None and all(np.array_equal(host(a), b, equal_nan=True) for a, b in zip(only[2:], want[2:]))
    src = t.zeros((2, n + 1), dtype=t.float64, device=lib.device())
    src[0, 1:], src[1, 1:] = dev(lib, lat32.astype(np.float64)), dev(lib, lon32.astype(np.float64))
    buf = t.full((4, n + 1), -7.0, dtype=t.float64, device=lib.device())
    assert src[0, 1:].data_ptr() % 16 == 8 or src[1, 1:].data_ptr() % 16 == 8
    g, l = grid._params(), ltg._params()
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())
    lib.check(lib.lib().tf_glm_parallax(ctypes.byref(g), ctypes.byref(l), *gc.GRS80, ptr(src[0, 1:]), ptr(src[1, 1:]), lib.TF_F64, n,
                                        ptr(buf[0, 1:]), ptr(buf[1, 1:]), ptr(buf[2, 1:]), ptr(buf[3, 1:]), lib.stream_ptr()), "tf_glm_parallax")
    shifted = host(buf)
    assert (shifted[:, 0] == -7.0).all() and all(np.array_equal(shifted[i, 1:], want[i], equal_nan=True) for i in range(4))


def test_parallax_nan_and_missed_rays(lib):
    grid, ltg = systems()
    nan_lat, nan_lon = np.array([np.nan, 10.0, np.nan, 20.0]), np.array([-80.0, np.nan, np.nan, -70.0])
    out = [host(v) for v in geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, nan_lat), dev(lib, nan_lon))]
    assert all(np.array_equal(np.isnan(v), [True, True, True, False]) for v in out)
    small = geo.GeosProj(gc.H_GOES, pc.LON_0, a=4.0e6)           # a `lightning` sphere well inside the Earth: rays can miss it
    lat, lon = np.array([0.0, 20.0, 60.0, 75.0]), np.array([-75.0, -60.0, -100.0, -75.0])
    want = [pc.oracle_chain(float(la), float(lo), ltg=(4.0e6, 0.0)) for la, lo in zip(lat, lon)]
    hit = pc.resolved(want)
    assert hit.tolist() == [True, True, False, False]
    dlon, dlat, x, y = (host(v) for v in geo.glm_parallax(grid, small, gc.GRS80, dev(lib, lat), dev(lib, lon)))
    assert np.array_equal(np.isnan(dlon), ~hit) and np.array_equal(np.isnan(dlat), ~hit)
    assert np.isposinf(x[~hit]).all() and np.isposinf(y[~hit]).all()
    assert (pc.chain_errors(want, dlon, dlat, x, y) <= gc.VIEW_TOL).all()
    with pytest.raises(ValueError, match="lon_0"):
        geo.glm_parallax(grid, geo.GeosProj(gc.H_GOES, -137.0, a=pc.LTG_RE, rf=pc.LTG_RF), gc.GRS80, dev(lib, lat), dev(lib, lon))


# ---- tf_ecef, tf_geos_to_ecef ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_ecef_both_modes(lib, n):
    X, Y, Z, want = pc.ecef_points()
    m = min(n, X.size)
    pick = np.arange(n) % X.size
    out = geo.ecef_to_geodetic(dev(lib, X[pick]), dev(lib, Y[pick]), dev(lib, Z[pick]), ellps="GRS80")
    assert on_device(lib, *out) and all(tuple(v.shape) == (n,) for v in out)
    lon, lat, alt = (host(v) for v in out)
    check_repeats(pick, m, lon, lat, alt)
    err = pc.to_geodetic_errors(want[:m], lon, lat, alt)
    print("ECEF -> geodetic: lon, lat (rad), height (m)", n, err)
    assert err[0] <= gc.ANGLE_TOL and err[1] <= gc.ANGLE_TOL and err[2] <= pc.HEIGHT_TOL
    back = [host(v) for v in geo.geodetic_to_ecef(out[0], out[1], out[2], ellps="GRS80")]
    check_repeats(pick, m, *back)
    worst = 0.0
    for k in range(m):
        exact = pc.oracle_to_ecef(lon[k], lat[k], alt[k], *gc.GRS80)
        worst = max(worst, max(abs(float(mp.mpf(float(back[i][k])) - exact[i])) for i in range(3)))
    print("geodetic -> ECEF (m)", n, worst)
    assert worst <= pc.HEIGHT_TOL


def test_ecef_edge_inputs(lib):
    a, rf = gc.GRS80
    b = a * (1 - 1 / rf)
    X = np.array([0.0, 0.0, 0.0, np.nan, 1.0, np.inf, a + 16003.0])
    Y = np.array([0.0, 0.0, 0.0, 0.0, np.nan, np.inf, 0.0])
    Z = np.array([b + 5.0, -b - 7.0, 0.0, 1.0, 1.0, np.inf, 0.0])
    lon, lat, alt = (host(v) for v in geo.ecef_to_geodetic(dev(lib, X), dev(lib, Y), dev(lib, Z), ellps="GRS80"))
    assert lon[:2].tolist() == [0.0, 0.0] and lat[:2].tolist() == [90.0, -90.0] and np.allclose(alt[:2], [5.0, 7.0], atol=1e-8)
    assert np.isnan(lon[2:6]).all() and np.isnan(lat[2:6]).all() and np.isnan(alt[2:6]).all()
    assert (lon[6], lat[6], alt[6]) == (0.0, 0.0, 16003.0)


@pytest.mark.parametrize("sweep", ["x", "y"])
@pytest.mark.parametrize("n", COUNTS)
def test_fixed_grid_to_ecef(lib, n, sweep):
    x, y, hit = pc.scan_points(sweep=sweep)
    m = min(n, x.size)
    pick = np.arange(n) % x.size
    ltg = systems(sweep)[1]
    out = ltg.to_ecef(dev(lib, x[pick]), dev(lib, y[pick]))
    assert on_device(lib, *out)
    X, Y, Z = (host(v) for v in out)
    check_repeats(pick, m, X, Y, Z)
    assert all(np.array_equal(np.isposinf(v[:m]), ~hit[:m]) and not np.isnan(v).any() for v in (X, Y, Z))
    angle, resid = pc.to_ecef_errors(x[:m], y[:m], hit[:m], X, Y, Z, sweep)
    print("fixed grid -> ECEF: backward error (rad), residual", n, sweep, angle, resid)
    assert angle <= gc.ANGLE_TOL and resid <= gc.ANGLE_TOL


# ---- device path against NumPy path ----------------------------------------------------------------------------------------
def test_device_path_against_numpy_path(lib):
    lat, lon, chain = pc.flashes()
    ds = goes_ds()
    d_off = glm.get_glm_parallax_offsets(dev(lib, lon), dev(lib, lat), ds)
    d_xy = glm.get_corrected_glm_x_y(dev(lib, lon), dev(lib, lat), ds)
    assert on_device(lib, *d_off, *d_xy)
    h_off = glm.get_glm_parallax_offsets(lon, lat, ds)
    h_xy = glm.get_corrected_glm_x_y(lon, lat, ds)
    ok = pc.resolved(chain)
    for d, h in zip(d_off, h_off):
        assert np.array_equal(np.isnan(host(d)), ~ok) and np.abs(np.radians(host(d) - h))[ok].max() <= 2 * gc.VIEW_TOL
    for d, h in zip(d_xy, h_xy):
        seen = np.isfinite(h)
        assert np.array_equal(np.isfinite(host(d)), seen) and np.abs(host(d)[seen] - h[seen]).max() <= 2 * gc.VIEW_TOL
    u = glm.get_uncorrected_glm_x_y(dev(lib, lon, np.float32), dev(lib, lat, np.float32), ds)
    assert on_device(lib, *u) and u[0].dtype == lib.torch().float64
    # the coordinate-system classes keep device tensors on the device too
    geofix_ltg, _ = _lmatools.get_GOESR_coordsys_alt_ellps(-75.0)
    _, grs80lla = _lmatools.get_GOESR_coordsys(-75.0)
    z = lib.torch().zeros(3, dtype=lib.torch().float64, device=lib.device())
    out = grs80lla.fromECEF(*geofix_ltg.toECEF(z, z, z))
    assert on_device(lib, *out) and host(out[1]).tolist() == [0.0] * 3 and np.abs(host(out[2]) - 16003.0).max() <= pc.HEIGHT_TOL


# ---- regridding and the dataset --------------------------------------------------------------------------------------------
def test_regrid_and_dataset_on_the_device(lib):
    t = lib.torch()
    c = pc.regrid_case()
    flashes = (dev(lib, c["flash_lat"], np.float32), dev(lib, c["flash_lon"], np.float32), dev(lib, c["flash_file"], np.int64))
    tail = (c["file_times"], c["ds"], c["goes_dates"], c["x_bins"], c["y_bins"])
    corrected = glm.regrid_glm_lat_lon(*flashes, *tail, corrected=True)
    assert on_device(lib, corrected) and corrected.dtype == t.int32 and np.array_equal(host(corrected), c["corrected"])
    plain = glm.regrid_glm_lat_lon(*flashes, *tail)
    assert on_device(lib, plain) and np.array_equal(host(plain), c["uncorrected"])
    from_numpy = glm.regrid_glm_lat_lon(c["flash_lat"], c["flash_lon"], c["flash_file"], *tail, corrected=True)
    assert isinstance(from_numpy, np.ndarray) and np.array_equal(from_numpy, c["corrected"])
    hist = glm.get_corrected_glm_hist(*flashes, c["file_times"], c["ds"], np.datetime64("2018-06-19T16:57:30"), np.datetime64("2018-06-19T17:02:30"))
    assert on_device(lib, hist) and hist.dtype == t.float64 and np.array_equal(host(hist), c["corrected"][0])
    ds = glm.create_gridded_flash_ds(c["ds"], *flashes, c["file_times"])
    for name in ("lat", "lon", "area", "glm_flashes", "glm_flash_count"):
        assert on_device(lib, ds[name]), name
    assert ds["glm_flashes"].dtype == t.int32 and ds.dims["glm_flashes"] == ("t", "y", "x")
    assert np.array_equal(host(ds["glm_flashes"]), c["corrected"])
    assert ds["glm_flash_count"].dtype == t.int32 and tuple(ds["glm_flash_count"].shape) == ()
    assert int(ds["glm_flash_count"]) == int(c["corrected"][c["corrected"] > 0].sum())
    on_host = glm.create_gridded_flash_ds(c["ds"], c["flash_lat"], c["flash_lon"], c["flash_file"], c["file_times"])
    assert isinstance(on_host["glm_flashes"], np.ndarray) and np.array_equal(on_host["glm_flashes"], c["corrected"])


def test_two_identical_runs(lib):
    lat, lon, _ = pc.flashes()
    pick = np.arange(4097) % lat.size
    grid, ltg = systems()

    def once():
        return [host(v) for v in geo.glm_parallax(grid, ltg, gc.GRS80, dev(lib, lat[pick]), dev(lib, lon[pick]))]
    first, second = once(), once()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, second))
