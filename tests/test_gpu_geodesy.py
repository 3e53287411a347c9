"""Geodesy on the GPU (csrc/geodesy.hip through tobac_flow_amd.geo / abi / nexrad / dataset / postprocess) against the mpmath
oracles of tests/geodesy_cases.py, at the smallest shapes at which the kernels can go wrong: grids with off-disk corners
whose width is no multiple of the four pixels a lane takes and whose last wave is ragged, point counts around one wave
and into a second workgroup, one-pixel axes for the spacing rule.  The oracle results are cached per session."""
import ctypes
import warnings

import mpmath as mp
import numpy as np
import pytest

import geodesy_cases as gc
from tobac_flow_amd import abi, geo

pytestmark = pytest.mark.gpu
GRIDS = ((37, 41), (5, 130))
COUNTS = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def dev(lib, a):
    return lib.torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(lib.device())


def host(v):
    return v.cpu().numpy()


def on_device(lib, *tensors):
    return all(isinstance(v, lib.torch().Tensor) and v.is_cuda for v in tensors)


# ---- projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", ["x", "y"])
@pytest.mark.parametrize("shape", GRIDS)
def test_inverse_grid(lib, shape, sweep):
    """backward error within 2^-48 rad, NaN exactly off the disk, float32 = float64 rounded once, the element-store form
    (outputs that start 8 bytes past a 16-byte boundary) equal to the 16-byte one"""
    H, W = shape
    x, y = gc.scan_grid(H, W)
    on = gc.grid_on_disk(H, W, sweep)
    p = geo.GeosProj(gc.H_GOES, -75.0, sweep=sweep)
    lat_d, lon_d = p.inverse_grid(dev(lib, x), dev(lib, y))
    assert on_device(lib, lat_d, lon_d) and lat_d.dtype == lib.torch().float64 and tuple(lat_d.shape) == (H, W)
    lat, lon = host(lat_d), host(lon_d)
    assert np.array_equal(np.isnan(lat), ~on) and np.array_equal(np.isnan(lon), ~on)
    worst = gc.backward_error(lat, lon, x, y, on, sweep)
    print("backward error", shape, sweep, worst)
    assert worst <= gc.ANGLE_TOL
    lat32, lon32 = p.inverse_grid(dev(lib, x), dev(lib, y), dtype=np.float32)
    assert lat32.dtype == lib.torch().float32
    assert np.array_equal(host(lat32), lat.astype(np.float32), equal_nan=True)
    assert np.array_equal(host(lon32), lon.astype(np.float32), equal_nan=True)
    lat_i, lon_i = p.inverse_grid(dev(lib, x), dev(lib, y), inf=True)
    assert np.array_equal(np.isposinf(host(lat_i)), ~on) and np.array_equal(np.isposinf(host(lon_i)), ~on)
    t = lib.torch()
    buf = t.full((2, H * W + 1), -7.0, dtype=t.float64, device=lib.device())
    geos = p._params()
    xd, yd = dev(lib, x), dev(lib, y)
    assert (buf[0, 1:].data_ptr() % 16, buf[1, 1:].data_ptr() % 16) != (0, 0)
    lib.check(lib.lib().tf_geos_inverse(ctypes.byref(geos), lib.ptr(xd), W, lib.ptr(yd), H, ctypes.c_void_p(buf[0, 1:].data_ptr()),
                                        ctypes.c_void_p(buf[1, 1:].data_ptr()), lib.TF_F64, lib.stream_ptr()), "tf_geos_inverse")
    got = host(buf)
    assert got[0, 0] == -7.0 and got[1, 0] == -7.0
    assert np.array_equal(got[0, 1:].reshape(H, W), lat, equal_nan=True) and np.array_equal(got[1, 1:].reshape(H, W), lon, equal_nan=True)


@pytest.mark.parametrize("n", COUNTS)
def test_points_forward_and_inverse(lib, n):
    """N points: the forward within 2^-48 rad of the oracle and +inf beyond the limb, the inverse equal to the grid kernel
    on the same rays"""
    p = geo.GeosProj(gc.H_GOES, -75.0)
    lat, lon = gc.forward_points(min(n, 65))
    pick = np.arange(n) % lat.size
    x, y = p.forward_points(dev(lib, lat[pick]), dev(lib, lon[pick]))
    assert on_device(lib, x, y) and tuple(x.shape) == (n,)
    x, y = host(x), host(y)
    assert np.array_equal(x, x[:lat.size][pick]) and np.array_equal(y, y[:lat.size][pick])
    beyond = np.zeros(lat.size, bool)
    beyond[::10] = True
    for k in range(min(n, lat.size)):
        if beyond[k]:
            assert np.isposinf(x[k]) and np.isposinf(y[k])
        else:
            ox, oy = gc.oracle_forward(float(lat[k]), float(lon[k]))
            assert abs(float(ox - mp.mpf(float(x[k])))) <= gc.ANGLE_TOL and abs(float(oy - mp.mpf(float(y[k])))) <= gc.ANGLE_TOL
    gx, gy = gc.scan_grid(37, 41)
    grid_lat, grid_lon = p.inverse_grid(dev(lib, gx), dev(lib, gy))
    xx, yy = np.meshgrid(gx, gy)
    pick = (np.arange(n) * 7) % xx.size
    plat, plon = p.inverse_points(dev(lib, xx.ravel()[pick]), dev(lib, yy.ravel()[pick]))
    assert on_device(lib, plat, plon)
    assert np.array_equal(host(plat), host(grid_lat).ravel()[pick], equal_nan=True)
    assert np.array_equal(host(plon), host(grid_lon).ravel()[pick], equal_nan=True)
    lon_m, lat_m = p(dev(lib, xx.ravel()[pick] * gc.H_GOES), dev(lib, yy.ravel()[pick] * gc.H_GOES), inverse=True)
    assert np.array_equal(np.isposinf(host(lat_m)), np.isnan(host(plat)))       # Proj.__call__: +inf off the disk


def test_forward_with_alt_is_map_nexrad_to_goes(lib):
    from tobac_flow_amd import nexrad
    rng = np.random.default_rng(4)
    n = 4097
    lat, lon, alt = rng.uniform(20, 55, n), rng.uniform(-125, -65, n), rng.uniform(0, 15000, n)
    lon[5] = 80.0                                                              # beyond the limb
    ds = gc.AbiLike(*gc.scan_grid(3, 3))
    x, y = nexrad.map_nexrad_to_goes(dev(lib, lat), dev(lib, lon), dev(lib, alt), ds)
    assert on_device(lib, x, y)
    wx, wy = nexrad.map_nexrad_to_goes(lat, lon, alt, ds)
    x, y = host(x), host(y)
    seen = np.isfinite(wx)
    assert not seen[5] and seen.sum() == n - 1 and np.array_equal(np.isfinite(x), seen)
    assert np.abs(x[seen] - wx[seen]).max() <= gc.ANGLE_TOL and np.abs(y[seen] - wy[seen]).max() <= gc.ANGLE_TOL
    x0, y0 = abi.get_abi_x_y(dev(lib, lat), dev(lib, lon), ds)
    assert np.abs(host(y0)[seen] - y[seen]).max() > 1e-6


# ---- geodesic inverse ------------------------------------------------------------------------------------------------------
def test_geodesic_case_list(lib):
    """distance within 1e-8 m + 1e-11 s, both azimuths within the same figure as lateral displacement, nothing lost"""
    c = gc.geodesic_cases()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = geo.Geod().inv(*(dev(lib, c[k]) for k in ("lon1", "lat1", "lon2", "lat2")))
    assert on_device(lib, *out)
    err = gc.geodesic_errors(*(host(v) for v in out))
    print("worst error / bound (distance, az12, az21):", (err[:, :3] / err[:, 3:]).max(0))
    assert np.isfinite(err).all() and (err[:, :3] <= err[:, 3:]).all()


@pytest.mark.parametrize("n", COUNTS)
def test_geodesic_counts(lib, n):
    """the tail lanes and a second workgroup: every pair gets the answer its case gets in the full list, scalars broadcast"""
    c = gc.geodesic_cases()
    m = len(c["s12"])
    pick = (np.arange(n) * 5) % m
    g = geo.Geod()
    full = [host(v) for v in g.inv(*(dev(lib, c[k]) for k in ("lon1", "lat1", "lon2", "lat2")))]
    got = g.inv(*(dev(lib, c[k][pick]) for k in ("lon1", "lat1", "lon2", "lat2")))
    for a, b in zip(got, full):
        assert tuple(a.shape) == (n,) and np.array_equal(host(a), b[pick])
    one = g.inv(float(c["lon1"][3]), float(c["lat1"][3]), dev(lib, c["lon2"][pick]), dev(lib, c["lat2"][pick]))
    k = int(np.nonzero(pick == 3)[0][0]) if (pick == 3).any() else None
    if k is not None:
        assert host(one[2])[k] == full[2][3]


def test_antipodal_pairs_and_nan_inputs(lib):
    """beyond 170 degrees every output is within the bound or NaN in all three and counted; NaN in gives NaN out uncounted"""
    near, exact = gc.antipodal_cases()
    g = geo.Geod()
    with pytest.warns(RuntimeWarning, match=r"pair\(s\) did not converge") as record:
        out = [host(v) for v in g.inv(*(dev(lib, near[k]) for k in ("lon1", "lat1", "lon2", "lat2")))]
    lost = np.isnan(out[2])
    assert np.array_equal(np.isnan(out[0]), lost) and np.array_equal(np.isnan(out[1]), lost)
    assert f"{int(lost.sum())} pair(s)" in str(record[0].message)
    err = gc.geodesic_errors(*out, cases=near)
    assert (err[~lost, :3] <= err[~lost, 3:]).all()
    with pytest.warns(RuntimeWarning, match="3 pair"):
        out = g.inv(*(dev(lib, exact[k]) for k in ("lon1", "lat1", "lon2", "lat2")))
    assert all(np.isnan(host(v)).all() for v in out)
    lon1 = np.array([0.0, np.nan, 0.0, 0.0, 0.0, 7.0, 7.0])
    lat1 = np.array([0.0, 0.0, np.nan, 0.0, 0.0, 8.0, -8.0])
    lon2 = np.array([1.0, 1.0, 1.0, np.nan, 1.0, 7.0, 7.0])
    lat2 = np.array([1.0, 1.0, 1.0, 1.0, np.nan, 8.0, -8.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                         # NaN inputs are not counted
        out = [host(v) for v in g.inv(dev(lib, lon1), dev(lib, lat1), dev(lib, lon2), dev(lib, lat2))]
    assert all(np.array_equal(np.isnan(v), [False, True, True, True, True, False, False]) for v in out)
    assert [v[5] for v in out] == [180.0, 0.0, 0.0] and [v[6] for v in out] == [0.0, -180.0, 0.0]


# ---- spacing and area ------------------------------------------------------------------------------------------------------
def _spacing_inputs(shape):
    H, W = shape
    if shape == (37, 41):
        lat, lon = geo.GeosProj(gc.H_GOES, -75.0).inverse_grid(*gc.scan_grid(H, W))
        assert np.isnan(lat[0, 0]) and np.isnan(lat[-1, -1])
        return lat, lon
    lat = 40.0 - 0.02 * np.arange(H)[:, None] - 0.001 * np.arange(W)[None, :] ** 2
    lon = -100.0 + 0.03 * np.arange(W)[None, :] + 0.002 * np.arange(H)[:, None] ** 2
    return tuple(np.ascontiguousarray(v) for v in np.broadcast_arrays(lat, lon))


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (3, 3), (37, 41)])
def test_grid_spacing(lib, shape):
    """dx, dy, area equal the reference's arithmetic (written out in NumPy) applied to the device's own raw spacings bit
    for bit, NaN pattern included, with each output left out in turn"""
    lat, lon = _spacing_inputs(shape)
    lat_d, lon_d = dev(lib, lat), dev(lib, lon)
    g = geo.Geod()
    raw_y, raw_x = np.zeros(shape), np.zeros(shape)
    if shape[0] > 1:
        raw_y[:-1] = host(g.inv(lon_d[:-1], lat_d[:-1], lon_d[1:], lat_d[1:])[2]) / 1e3
    if shape[1] > 1:
        raw_x[:, :-1] = host(g.inv(lon_d[:, :-1], lat_d[:, :-1], lon_d[:, 1:], lat_d[:, 1:])[2]) / 1e3
    want = {"dy": geo._spacing_rule(raw_y, 0), "dx": geo._spacing_rule(raw_x, 1)}
    want["area"] = want["dx"] * want["dy"]
    for names in (("dx", "dy", "area"), ("dy", "area"), ("dx", "area"), ("dx", "dy"), ("area",), ("dx",), ("dy",)):
        got = geo.grid_spacing(lat_d, lon_d, names)
        assert on_device(lib, *got)
        for name, v in zip(names, got):
            assert np.array_equal(host(v), want[name], equal_nan=True), (names, name)
    if shape == (37, 41):
        off = np.isnan(lat)
        beside = off.copy()
        beside[1:] |= off[:-1]
        beside[:-1] |= off[1:]
        assert np.isnan(want["dy"][beside]).all() and np.isfinite(want["dy"][~beside]).all()
        assert np.isfinite(want["area"]).sum() > 500
    dx, dy = geo.get_pixel_lengths(lat, lon)                                   # the NumPy path, its own raw spacings
    ok = np.isfinite(dx)
    assert np.array_equal(ok, np.isfinite(want["dx"])) and np.allclose(dx[ok], want["dx"][ok], rtol=1e-12, atol=0)


# ---- viewing angles --------------------------------------------------------------------------------------------------------
def test_view_angles(lib):
    """the four modes against the reference functions evaluated in mpmath: within 2^-46 rad"""
    def run(mode, sc, lat, lon, x, y):
        out = geo.view_angles(mode, sc, dev(lib, lat), dev(lib, lon), None if x is None else dev(lib, x), None if y is None else dev(lib, y))
        assert on_device(lib, out[0])
        return tuple(None if v is None else host(v) for v in out)
    worst = gc.view_angle_errors(run)
    print("view angle errors (rad) per mode:", worst)
    assert all(v <= gc.VIEW_TOL for v in worst.values()), worst


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_goes_grid_to_binning_stays_on_the_device(lib, monkeypatch):
    """create_new_goes_ds and get_abi_x_y feed binning with device tensors: every pixel centre falls into its own bin, and
    nothing is downloaded on the way"""
    from tobac_flow_amd import binning, dataset
    H, W = 37, 41
    x, y = gc.scan_grid(H, W)
    src = gc.AbiLike(dev(lib, x), dev(lib, y))
    src.t = np.datetime64("2018-06-19T17:05:00")
    x_edges = np.concatenate([[x[0] - (x[1] - x[0]) / 2], (x[1:] + x[:-1]) / 2, [x[-1] + (x[1] - x[0]) / 2]])
    y_edges = np.concatenate([[y[0] - (y[1] - y[0]) / 2], (y[1:] + y[:-1]) / 2, [y[-1] + (y[1] - y[0]) / 2]])

    def no_download(*a, **k):
        raise AssertionError("a device result was taken to the host")
    ds = dataset.create_new_goes_ds(src)                                       # takes the two coordinate vectors to the host, nothing else
    with monkeypatch.context() as m:
        m.setattr(lib, "to_host", no_download)
        m.setattr(lib.torch().Tensor, "cpu", no_download)
        m.setattr(lib.torch().Tensor, "numpy", no_download)
        lat64, lon64 = abi.get_abi_lat_lon(src)
        px, py = abi.get_abi_x_y(lat64, lon64, src)
        area64 = abi.get_abi_pixel_area(src)
        seen = lib.torch().isfinite(px)
        got = binning.bin_points([py[seen], px[seen]], [y_edges[::-1].copy(), x_edges], flip=(0,), outputs=("count",))["count"]
    for name in ("lat", "lon", "area"):
        assert on_device(lib, ds[name]) and ds[name].dtype == lib.torch().float32 and tuple(ds[name].shape) == (H, W)
    assert on_device(lib, area64) and np.array_equal(host(ds["area"]), host(area64).astype(np.float32), equal_nan=True)
    assert on_device(lib, px, py)
    assert on_device(lib, got)
    on = gc.grid_on_disk(H, W)
    assert np.array_equal(host(seen), on)
    assert np.array_equal(host(got).reshape(H, W), on.astype(np.int32))
    want_lat, want_lon = geo.GeosProj(gc.H_GOES, -75.0).inverse_grid(x, y)
    assert np.array_equal(host(ds["lat"]), host(lat64).astype(np.float32), equal_nan=True)
    assert np.allclose(host(ds["lat"])[on], want_lat[on], rtol=0, atol=4e-6)
    area = host(ds["area"])
    want_area = geo.get_pixel_area(want_lat, want_lon)
    ok = np.isfinite(want_area)
    assert np.array_equal(np.isfinite(area), ok) and np.allclose(area[ok], want_area[ok], rtol=1e-6)


def test_propagation_in_one_device_call(lib):
    """the third stage with device columns and the package's own inverse equals its host result"""
    import objects_cases as oc
    from tobac_flow_amd import postprocess
    base = oc.np_filter_cores(oc.np_remove_orphan_coords(oc.world()))
    g = geo.Geod()
    want = postprocess.process_core_properties(oc.to_label_dataset(base), geod_inv=g.inv)
    def column(v):
        v = np.asarray(v)
        return lib.torch().from_numpy(np.ascontiguousarray(v.view(np.int64) if v.dtype.kind in "mM" else v)).to(lib.device())
    got = postprocess.process_core_properties(oc.to_label_dataset(base, column), geod_inv=g.inv)
    for name in ("core_propagation_direction", "core_propagation_speed"):
        a, b = host(got[name]) if lib.is_tensor(got[name]) else np.asarray(got[name]), np.asarray(want[name])
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=1e-9, atol=1e-9), name


def test_two_identical_runs(lib):
    x, y = gc.scan_grid(37, 41)
    c = gc.geodesic_cases()
    p = geo.GeosProj(gc.H_GOES, -75.0)

    def once():
        lat, lon = p.inverse_grid(dev(lib, x), dev(lib, y))
        fx, fy = p.forward_points(lat, lon, lat * 100.0)
        inv = geo.Geod().inv(*(dev(lib, c[k]) for k in ("lon1", "lat1", "lon2", "lat2")))
        spacing = geo.grid_spacing(lat, lon, ("dx", "dy", "area"))
        angles = geo.view_angles(2, (0.0, -75.0, 35793.0), lat, lon)
        return [host(v) for v in (lat, lon, fx, fy, *inv, *spacing, *angles)]
    first, second = once(), once()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, second))
