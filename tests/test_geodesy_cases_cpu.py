"""CPU tests of the geodesy: the NumPy paths of tobac_flow_amd.geo / abi / utils.geo_utils / nexrad / dataset against the
mpmath oracles and known answers of tests/geodesy_cases.py, the edge rules of the grid spacing, the propagation
variables of the third stage on the package's own geodesic inverse, the C ABI's argument checks, and the kernels'
arithmetic itself compiled for the host (tools/geodesy_check)."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings
from datetime import datetime

import mpmath as mp
import numpy as np
import pytest

import geodesy_cases as gc
from tobac_flow_amd import abi, geo
from tobac_flow_amd.utils import geo_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((37, 41), (5, 130))


# ---- projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", ["x", "y"])
@pytest.mark.parametrize("shape", GRIDS)
def test_inverse_grid_backward_error_and_disk(shape, sweep):
    """the returned (lat, lon), projected forward by the geometric oracle, give both scan angles back within 2^-48 rad;
    NaN exactly where the oracle's discriminant is negative; float32 is the float64 result rounded once"""
    H, W = shape
    x, y = gc.scan_grid(H, W)
    on = gc.grid_on_disk(H, W, sweep)
    assert on.any() and not on.all()
    p = geo.GeosProj(gc.H_GOES, -75.0, sweep=sweep)
    lat, lon = p.inverse_grid(x, y)
    assert lat.shape == (H, W) and lat.dtype == np.float64
    assert np.array_equal(np.isnan(lat), ~on) and np.array_equal(np.isnan(lon), ~on)
    worst = gc.backward_error(lat, lon, x, y, on, sweep)
    print("backward error", shape, sweep, worst)
    assert worst <= gc.ANGLE_TOL
    lat32, lon32 = p.inverse_grid(x, y, dtype=np.float32)
    assert lat32.dtype == np.float32 and np.array_equal(lat32, lat.astype(np.float32), equal_nan=True)
    assert np.array_equal(lon32, lon.astype(np.float32), equal_nan=True)
    lat_i, lon_i = p.inverse_grid(x, y, inf=True)
    assert np.array_equal(np.isposinf(lat_i), ~on) and np.array_equal(np.isposinf(lon_i), ~on)


def test_known_answer_of_the_goes_r_product_guide():
    p = geo.GeosProj(h=35786023.0, lon_0=-75.0)
    lon, lat = p(-0.024052 * 35786023.0, 0.095340 * 35786023.0, inverse=True)
    assert isinstance(lat, float) and round(lat, 6) == 33.846162 and round(lon, 6) == -84.690932
    lat2, lon2 = p.inverse_points(np.array([-0.024052]), np.array([0.095340]))
    assert round(float(lat2[0]), 6) == 33.846162 and round(float(lon2[0]), 6) == -84.690932
    assert p(1e9, 1e9, inverse=True) == (np.inf, np.inf)                       # Proj.__call__ off the disk


@pytest.mark.parametrize("sweep", ["x", "y"])
def test_forward_points_against_the_oracle(sweep):
    lat, lon = gc.forward_points(65)
    p = geo.GeosProj(gc.H_GOES, -75.0, sweep=sweep)
    x, y = p.forward_points(lat, lon)
    assert np.isposinf(x[::10]).all() and np.isposinf(y[::10]).all()           # beyond the limb
    seen = np.isfinite(x)
    assert seen.sum() >= 50
    worst = 0.0
    for k in np.nonzero(seen)[0]:
        ox, oy = gc.oracle_forward(float(lat[k]), float(lon[k]), sweep=sweep)
        worst = max(worst, abs(float(ox - mp.mpf(float(x[k])))), abs(float(oy - mp.mpf(float(y[k])))))
    print("forward error", sweep, worst)
    assert worst <= gc.ANGLE_TOL
    xm, ym = p(lon, lat)                                                       # Proj.__call__: metres
    assert np.array_equal(xm, x * gc.H_GOES) and np.array_equal(ym, y * gc.H_GOES)


def test_lat_0_is_refused_and_longitudes_wrap():
    with pytest.raises(ValueError, match="lat_0"):
        geo.GeosProj(gc.H_GOES, -75.0, lat_0=1.0)
    with pytest.raises(ValueError):
        geo.GeosProj(gc.H_GOES, -75.0, sweep="z")
    west = geo.GeosProj(gc.H_GOES, -137.0)
    lat, lon = west.inverse_points(np.array([-0.12]), np.array([0.01]))
    assert 100 < lon[0] <= 180                                                 # -137 - 60 degrees comes back as +163
    x, y = west.forward_points(lat, lon)
    assert abs(x[0] + 0.12) < 1e-14 and abs(y[0] - 0.01) < 1e-14


def test_abi_functions_on_an_attribute_object():
    x, y = gc.scan_grid(9, 11)
    ds = gc.AbiLike(x, y)
    lat, lon = abi.get_abi_lat_lon(ds)
    want = geo.GeosProj(gc.H_GOES, -75.0).inverse_grid(x, y)
    assert np.array_equal(lat, want[0], equal_nan=True) and np.array_equal(lon, want[1], equal_nan=True)
    assert abi.get_abi_lat_lon(ds, dtype=np.float32)[0].dtype == np.float32
    on = np.isfinite(lat)
    px, py = abi.get_abi_x_y(lat[on], lon[on], ds)
    xx, yy = np.meshgrid(x, y)
    assert np.abs(px - xx[on]).max() < 1e-13 and np.abs(py - yy[on]).max() < 1e-13
    dx, dy = abi.get_abi_pixel_lengths(ds)
    area = abi.get_abi_pixel_area(ds)
    assert np.array_equal(area, dx * dy, equal_nan=True)
    want_dx, want_dy = geo.get_pixel_lengths(lat, lon)
    assert np.array_equal(dx, want_dx, equal_nan=True) and np.array_equal(dy, want_dy, equal_nan=True)
    assert np.array_equal(geo.get_pixel_area(lat, lon), area, equal_nan=True)
    ds.goes_imager_projection.latitude_of_projection_origin = 2.0
    with pytest.raises(ValueError, match="lat_0"):
        abi.get_abi_lat_lon(ds)


def test_map_nexrad_to_goes_is_project_shift_project():
    from tobac_flow_amd import nexrad
    rng = np.random.default_rng(2)
    lat, lon, alt = rng.uniform(25, 50, 40), rng.uniform(-120, -70, 40), rng.uniform(0, 15000, 40)
    ds = gc.AbiLike(*gc.scan_grid(3, 3))
    x, y = nexrad.map_nexrad_to_goes(lat, lon, alt, ds)
    x0, y0 = abi.get_abi_x_y(lat, lon, ds)
    dlat = np.degrees(alt * np.tan(np.radians(lat - 0.0) + y0 / gc.H_GOES) / 6.371e6)
    dlon = np.degrees(alt * np.tan(np.radians(lon - -75.0) + x0 / gc.H_GOES) / 6.371e6)
    wx, wy = abi.get_abi_x_y(lat + dlat, lon + dlon, ds)
    assert np.array_equal(x, wx) and np.array_equal(y, wy)
    assert np.abs(y - y0).max() > 1e-6                                         # the shift is there
    empty = nexrad.map_nexrad_to_goes(np.array([]), np.array([]), np.array([]), ds)
    assert empty[0].size == 0 and empty[1].size == 0


# ---- geodesic inverse ------------------------------------------------------------------------------------------------------
def test_geodesic_inverse_against_the_quadrature():
    """distance within 1e-8 m + 1e-11 s, each azimuth within the same figure as lateral displacement, no pair lost"""
    c = gc.geodesic_cases()
    assert 180 <= len(c["s12"]) <= 220
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        az12, az21, dist = geo.Geod().inv(c["lon1"], c["lat1"], c["lon2"], c["lat2"])
    err = gc.geodesic_errors(az12, az21, dist)
    print("worst error / bound (distance, az12, az21):", (err[:, :3] / err[:, 3:]).max(0))
    assert np.isfinite(err).all()
    assert (err[:, :3] <= err[:, 3:]).all()


def test_beyond_170_degrees_no_silent_error():
    """every output is within the bound or NaN in all three and counted in the warning"""
    near, exact = gc.antipodal_cases()
    with pytest.warns(RuntimeWarning, match=r"\d+ pair\(s\) did not converge") as record:
        az12, az21, dist = geo.Geod().inv(near["lon1"], near["lat1"], near["lon2"], near["lat2"])
    lost = np.isnan(dist)
    assert np.array_equal(np.isnan(az12), lost) and np.array_equal(np.isnan(az21), lost)
    assert f"{int(lost.sum())} pair(s)" in str(record[0].message)
    err = gc.geodesic_errors(az12, az21, dist, cases=near)
    assert (err[~lost, :3] <= err[~lost, 3:]).all()
    with pytest.warns(RuntimeWarning, match="3 pair"):
        out = geo.Geod().inv(exact["lon1"], exact["lat1"], exact["lon2"], exact["lat2"])
    assert all(np.isnan(v).all() for v in out)


def test_geod_inv_conventions_broadcasting_and_scalars():
    g = geo.Geod()
    assert g.inv(0.0, 0.0, 0.0, 0.0) == (180.0, 0.0, 0.0)                      # coincident: GeographicLib's answer
    assert g.inv(10.0, -5.0, 10.0, -5.0) == (0.0, -180.0, 0.0)
    az12, az21, dist = g.inv(0.0, 0.0, 0.0, 1.0)
    assert isinstance(dist, float) and az12 == 0.0 and az21 == -180.0
    assert abs(dist - 110574.38855780) < 1e-6                                  # one degree of the meridian from the equator, WGS84
    az12, az21, dist = g.inv(np.zeros((3, 1)), 0.0, np.array([1.0, 2.0]), [[0.0], [1.0], [np.nan]])
    assert az12.shape == az21.shape == dist.shape == (3, 2)
    assert np.isnan(dist[2]).all() and np.isnan(az12[2]).all() and np.isfinite(dist[:2]).all()
    assert abs(dist[0, 0] - 111319.4907932264) < 1e-6                          # one degree of the equator
    assert np.all(az12[0] == 90.0) and np.all(az21[0] == -90.0)
    sphere = geo.Geod(a=6371000.0)
    assert abs(sphere.inv(0.0, 0.0, 90.0, 0.0)[2] - 6371000.0 * np.pi / 2) < 1e-6
    grs = geo.Geod(ellps="GRS80")
    assert grs.rf == 298.257222101
    with pytest.raises(ValueError):
        geo.Geod(ellps="clarke")


def test_mean_object_azimuth_and_speed_known_answers():
    """the values of the reference's own tests/test_geo_utils.py.  The direction is compared on the circle: for the one
    azimuth 180 SciPy's circmean(high=180, low=-180) gives 180 or -180 depending on its version, the same direction."""
    f = geo_utils.get_mean_object_azimuth_and_speed

    def off(direction, want):
        return abs((direction - want + 180.0) % 360.0 - 180.0)

    direction, speed = f(np.array([0, 0]), np.array([0, 1]), np.array([0, 100e9]))
    assert off(direction, 0) < 1e-6 and abs(speed - 1100) <= 20
    direction, speed = f(np.array([0, 0]), np.array([0, -1]), np.array([0, 100e9]))
    assert off(direction, 180) < 1e-6 and abs(speed - 1100) <= 20
    direction, speed = f(np.array([0, 1]), np.array([0, 0]), np.array([0, 100e9]))
    assert off(direction, 90) < 1e-6 and abs(speed - 1100) <= 20
    direction, speed = f(np.array([0, -1]), np.array([0, 0]), np.array([0, 100e9]))
    assert off(direction, -90) < 1e-6 and abs(speed - 1100) <= 20
    direction, speed = f(np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([0, 100e9, 150e9]))
    assert off(direction, 45) <= 0.1 and abs(speed - 1650) <= 30
    assert np.isnan(f(np.array([0.0, np.nan]), np.array([0.0, 1.0]), np.array([0, 100e9]))).all()


# ---- spacing and area ------------------------------------------------------------------------------------------------------
def _reference_rule(raw_y, raw_x):
    """geo.py:230-236 as written, on given raw spacings"""
    dy, dx = np.zeros(raw_y.shape), np.zeros(raw_y.shape)
    dy[:-1] = raw_y[:-1]
    dx[:, :-1] = raw_x[:, :-1]
    dy[1:] += dy[:-1]
    dy[1:-1] /= 2
    dx[:, 1:] += dx[:, :-1]
    dx[:, 1:-1] /= 2
    return dx, dy


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (2, 2), (3, 3), (6, 5)])
def test_spacing_edge_rules(shape):
    H, W = shape
    lat = 40.0 - 0.02 * np.arange(H)[:, None] - 0.001 * np.arange(W)[None, :] ** 2
    lon = -100.0 + 0.03 * np.arange(W)[None, :] + 0.002 * np.arange(H)[:, None] ** 2
    lat, lon = np.broadcast_arrays(lat, lon)
    g = geo.Geod()
    raw_y, raw_x = np.zeros(shape), np.zeros(shape)
    raw_y[:-1] = g.inv(lon[:-1], lat[:-1], lon[1:], lat[1:])[2] / 1e3
    raw_x[:, :-1] = g.inv(lon[:, :-1], lat[:, :-1], lon[:, 1:], lat[:, 1:])[2] / 1e3
    want_dx, want_dy = _reference_rule(raw_y, raw_x)
    dx, dy = geo_utils.get_grid_spacing_from_lat_lon(lat, lon)
    assert np.array_equal(dx, want_dx) and np.array_equal(dy, want_dy)
    assert np.array_equal(geo_utils.get_area_from_lat_lon(lat, lon), want_dx * want_dy)
    if H == 1:
        assert not dy.any()
    if W == 1:
        assert not dx.any()
    if H >= 3:
        assert np.array_equal(dy[0], raw_y[0]) and np.array_equal(dy[-1], raw_y[-2]) and np.array_equal(dy[1], (raw_y[1] + raw_y[0]) / 2)
    if H == 2:
        assert np.array_equal(dy[0], dy[1])


def test_spacing_nan_propagation_matches_the_reference():
    """a pixel next to an off-disk pixel is NaN, exactly as Geod.inv followed by the reference's arithmetic gives it"""
    x, y = gc.scan_grid(9, 11)
    lat, lon = geo.GeosProj(gc.H_GOES, -75.0).inverse_grid(x, y)
    assert np.isnan(lat[0, 0]) and np.isfinite(lat[4, 5])
    g = geo.Geod()
    raw_y, raw_x = np.zeros(lat.shape), np.zeros(lat.shape)
    raw_y[:-1] = g.inv(lon[:-1], lat[:-1], lon[1:], lat[1:])[2] / 1e3
    raw_x[:, :-1] = g.inv(lon[:, :-1], lat[:, :-1], lon[:, 1:], lat[:, 1:])[2] / 1e3
    want_dx, want_dy = _reference_rule(raw_y, raw_x)
    dx, dy = geo.get_pixel_lengths(lat, lon)
    assert np.array_equal(dx, want_dx, equal_nan=True) and np.array_equal(dy, want_dy, equal_nan=True)
    off = np.isnan(lat)
    beside = np.zeros_like(off)
    beside[1:] |= off[:-1]
    beside[:-1] |= off[1:]
    assert np.isnan(dy[(off | beside)]).all() and np.isfinite(dy[~(off | beside)]).all()


def test_add_area_to_dataset_and_create_new_goes_ds():
    from tobac_flow_amd import dataset
    x, y = gc.scan_grid(9, 11)
    src = gc.AbiLike(x, y)
    src.t = np.datetime64("2018-06-19T17:05:00")
    ds = dataset.create_new_goes_ds(src, device=False)
    lat, lon = abi.get_abi_lat_lon(src)
    assert ds.dims["lat"] == ds.dims["lon"] == ds.dims["area"] == ("y", "x")
    assert ds["lat"].dtype == ds["lon"].dtype == ds["area"].dtype == np.float32
    assert np.array_equal(ds["lat"], lat.astype(np.float32), equal_nan=True)
    assert np.array_equal(ds["lon"], lon.astype(np.float32), equal_nan=True)
    assert np.array_equal(ds["area"], geo.get_pixel_area(lat, lon).astype(np.float32), equal_nan=True)
    assert np.array_equal(ds.coords["x"], x) and np.array_equal(ds.coords["y"], y) and ds.coords["t"].shape == (1,)
    assert np.array_equal(abi.get_abi_lat_lon(ds)[0], lat, equal_nan=True)     # the result is a `dataset` for abi again
    two = dataset.LabelDataset()
    two.add("lat", lat, ("y", "x"))
    two.add("lon", lon, ("y", "x"))
    geo_utils.add_area_to_dataset(two)
    assert two["area"].dtype == np.float32 and two.dims["area"] == ("y", "x")
    assert np.array_equal(two["area"], geo_utils.get_area_from_lat_lon(lat, lon).astype(np.float32), equal_nan=True)
    three = dataset.LabelDataset()
    three.add("lat", np.stack([lat, lat + 1]), ("t", "y", "x"))
    three.add("lon", np.stack([lon, lon]), ("t", "y", "x"))
    geo_utils.add_area_to_dataset(three)
    assert three["area"].shape == (2,) + lat.shape
    assert np.array_equal(three["area"][1], geo_utils.get_area_from_lat_lon(lat, lon), equal_nan=True)


# ---- viewing angles --------------------------------------------------------------------------------------------------------
def test_view_angles_against_mpmath():
    worst = gc.view_angle_errors(lambda mode, sc, lat, lon, x, y: geo.view_angles(mode, sc, lat, lon, x, y))
    print("view angle errors (rad) per mode:", worst)
    assert all(v <= gc.VIEW_TOL for v in worst.values()), worst


def test_view_angle_functions_are_the_reference_expressions():
    date = datetime(2019, 7, 14, 18, 40)
    lat, lon = gc.view_points(12)
    sza = geo.get_sza(date, lat, lon)
    assert sza.shape == lat.shape and isinstance(geo.get_sza(date, 10.0, -60.0), float)
    zen, azi = geo.get_sza_and_azi(date, lat, lon)
    assert np.abs(np.radians(zen) - sza).max() < 0.02                          # the two differ in the day number and seconds only
    zen, azi = geo.get_satellite_viewing_angles(0.0, 0.0)
    assert zen == 0.0 and isinstance(azi, float)
    zen, azi = geo.get_satellite_viewing_angles(np.array([0.0, 10.0, 0.0, 85.0]), np.array([10.0, 0.0, 170.0, 0.0]))
    assert np.allclose(azi[:2], [90.0, 0.0]) and zen[2] > 90 and 0 < zen[0] < 90
    src = gc.AbiLike(*gc.scan_grid(5, 5, span=0.1))
    src.t = np.datetime64("2019-07-14T18:40:00")
    assert np.array_equal(abi.get_goes_sza(src), geo.get_sza(date, *abi.get_abi_lat_lon(src)), equal_nan=True)
    centre = abi.get_abi_zenith_angle(src)[2, 2]
    assert 0 <= centre < 0.01


# ---- third stage -----------------------------------------------------------------------------------------------------------
def test_propagation_on_the_packages_own_inverse():
    """geod_inv=geo.Geod().inv: the propagation variables appear, from one inverse call over all pairs, and equal what
    the per-object path gives with the same inverse"""
    import objects_cases as oc
    from tobac_flow_amd import postprocess
    base = oc.np_filter_cores(oc.np_remove_orphan_coords(oc.world()))
    g = geo.Geod()
    calls = []

    original = geo.Geod.inv

    def counted(self, *args):
        calls.append(np.size(args[0]))
        return original(self, *args)

    assert "core_propagation_direction" not in postprocess.process_core_properties(oc.to_label_dataset(base))
    got = postprocess.process_core_properties(oc.to_label_dataset(base), geod_inv=g.inv)
    per_object = postprocess.process_core_properties(oc.to_label_dataset(base), geod_inv=lambda *a: g.inv(*a))
    for name in ("core_propagation_direction", "core_propagation_speed"):
        assert np.array_equal(got[name], per_object[name], equal_nan=True), name
        assert np.isfinite(got[name]).any()
    anvils = postprocess.process_thick_anvil_properties(oc.to_label_dataset(base), geod_inv=g.inv)
    assert "anvil_propagation_direction" in anvils and "anvil_propagation_speed" in anvils
    try:
        geo.Geod.inv = counted
        postprocess.process_core_properties(oc.to_label_dataset(base), geod_inv=geo.Geod().inv)
    finally:
        geo.Geod.inv = original
    assert len(calls) == 1 and calls[0] > 1


# ---- the C ABI and the kernels' arithmetic on the host ---------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_check_their_arguments():
    from tobac_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = ("tf_geos_inverse", "tf_geos_inverse_points", "tf_geos_forward", "tf_geod_inverse", "tf_geod_inverse_workspace_bytes",
             "tf_grid_spacing", "tf_grid_spacing_workspace_bytes", "tf_view_angles")
    for name in names:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS
    L = _lib.lib()
    assert L.tf_version() >= 115
    assert L.tf_geod_inverse_workspace_bytes(0) == 0 and L.tf_geod_inverse_workspace_bytes(257) >= 8
    assert L.tf_grid_spacing_workspace_bytes(3, 5) >= 2 * 15 * 8
    bad = _lib.Geos(gc.H_GOES, -75.0, 1.0, gc.GRS80[0], gc.GRS80[1], 0, 0)
    assert L.tf_geos_inverse(ctypes.byref(bad), None, 0, None, 0, None, None, _lib.TF_F64, None) == -1
    assert "lat_0" in L.tf_last_error().decode()
    assert L.tf_geos_forward(ctypes.byref(bad), None, None, None, 0, None, None, None) == -1
    ok = _lib.Geos(gc.H_GOES, -75.0, 0.0, gc.GRS80[0], gc.GRS80[1], 0, 0)
    assert L.tf_geos_inverse(ctypes.byref(ok), None, 0, None, 0, None, None, _lib.TF_F64, None) == 0       # empty grid
    assert L.tf_geos_inverse(ctypes.byref(ok), None, 4, None, 4, None, None, _lib.TF_F64, None) == -1      # null pointers
    assert L.tf_geos_inverse(ctypes.byref(ok), None, 0, None, 0, None, None, _lib.TF_I32, None) == -1
    assert L.tf_geod_inverse(-1.0, 298.0, None, None, None, None, 0, None, None, None, None, None, 0, None) == -1
    assert L.tf_view_angles(7, None, 0, None, None, 0, None, None, 1, None, None, None) == -1


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("geodesy_check") / "geodesy_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                           os.path.join(ROOT, "tools", "geodesy_check", "geodesy_check.cpp")])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = [[float.fromhex(v) if re.search(r"[xnp]", v) else float(v) for v in row.split()] for row in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return np.array(rows)
    return run


def _hex(*values):
    return " ".join(float(v).hex() for v in values)


def test_kernel_arithmetic_on_the_host_geodesic(host_check):
    """gd_geod_inverse_one, the text the device runs, against the quadrature: the same bounds"""
    c = gc.geodesic_cases()
    a, rf = gc.WGS84
    rows = host_check([f"geod {_hex(a, rf, c['lon1'][k], c['lat1'][k], c['lon2'][k], c['lat2'][k])}" for k in range(len(c["s12"]))])
    assert not rows[:, 3].any()
    err = gc.geodesic_errors(rows[:, 0], rows[:, 1], rows[:, 2])
    assert (err[:, :3] <= err[:, 3:]).all()
    near, exact = gc.antipodal_cases()
    rows = host_check([f"geod {_hex(a, rf, near['lon1'][k], near['lat1'][k], near['lon2'][k], near['lat2'][k])}" for k in range(len(near["s12"]))]
                      + [f"geod {_hex(a, rf, exact['lon1'][k], exact['lat1'][k], exact['lon2'][k], exact['lat2'][k])}" for k in range(3)]
                      + [f"geod {_hex(a, rf)} nan 0 1 1", f"geod {_hex(a, rf, 5, 6, 5, 6)}", f"geod {_hex(a, rf, 5, -6, 5, -6)}"])
    n = len(near["s12"])
    lost = rows[:n, 3] == 1
    assert np.array_equal(np.isnan(rows[:n, :3]).all(1), lost) and np.array_equal(np.isnan(rows[:n, :3]).any(1), lost)
    err = gc.geodesic_errors(rows[:n, 0], rows[:n, 1], rows[:n, 2], cases=near)
    assert (err[~lost, :3] <= err[~lost, 3:]).all()
    assert np.isnan(rows[n:n + 3, :3]).all() and (rows[n:n + 3, 3] == 1).all()             # exact antipodes: NaN and counted
    assert np.isnan(rows[n + 3, :3]).all() and rows[n + 3, 3] == 0                          # NaN in: NaN out, not counted
    assert rows[n + 4].tolist() == [180.0, 0.0, 0.0, 0.0] and rows[n + 5].tolist() == [0.0, -180.0, 0.0, 0.0]


@pytest.mark.parametrize("sweep", ["x", "y"])
def test_kernel_arithmetic_on_the_host_projection(host_check, sweep):
    H, W = 37, 41
    x, y = gc.scan_grid(H, W)
    on = gc.grid_on_disk(H, W, sweep)
    head = _hex(gc.H_GOES, -75.0, *gc.GRS80, sweep == "y")
    rows = host_check([f"inv {head} {_hex(x[j], y[i])}" for i in range(H) for j in range(W)])
    lat, lon = rows[:, 0].reshape(H, W), rows[:, 1].reshape(H, W)
    assert np.array_equal(np.isnan(lat), ~on) and np.array_equal(np.isnan(lon), ~on)
    assert gc.backward_error(lat, lon, x, y, on, sweep) <= gc.ANGLE_TOL
    plat, plon = gc.forward_points(65)
    rows = host_check([f"fwd {head} {_hex(plat[k], plon[k])}" for k in range(65)])
    assert np.isposinf(rows[::10]).all()
    for k in np.nonzero(np.isfinite(rows[:, 0]))[0]:
        ox, oy = gc.oracle_forward(float(plat[k]), float(plon[k]), sweep=sweep)
        assert abs(float(ox - mp.mpf(rows[k, 0]))) <= gc.ANGLE_TOL and abs(float(oy - mp.mpf(rows[k, 1]))) <= gc.ANGLE_TOL
    alt = np.linspace(0, 15000, 65)
    rows = host_check([f"fwdalt {head} {_hex(plat[k], plon[k], alt[k])}" for k in range(65)])
    want = geo.GeosProj(gc.H_GOES, -75.0, sweep=sweep).forward_points(plat, plon, alt)
    seen = np.isfinite(want[0])
    assert np.array_equal(np.isfinite(rows[:, 0]), seen)
    assert np.abs(rows[seen, 0] - want[0][seen]).max() <= gc.ANGLE_TOL and np.abs(rows[seen, 1] - want[1][seen]).max() <= gc.ANGLE_TOL


def test_kernel_arithmetic_on_the_host_angles_and_rule(host_check):
    def run(mode, sc, lat, lon, x, y):
        sc = list(sc) + [0.0] * (3 - len(sc))
        lat, lon = np.asarray(lat), np.asarray(lon)
        if mode == 3:
            x, y = np.meshgrid(x, y)
        else:
            x, y = np.zeros(lat.shape), np.zeros(lat.shape)
        rows = host_check([f"view {mode} {_hex(*sc, la, lo, sx, sy)}" for la, lo, sx, sy in zip(lat.ravel(), lon.ravel(), x.ravel(), y.ravel())])
        return rows[:, 0].reshape(lat.shape), rows[:, 1].reshape(lat.shape)
    worst = gc.view_angle_errors(run)
    assert all(v <= gc.VIEW_TOL for v in worst.values()), worst
    rows = host_check(["rule 0 1 0 5", "rule 0 4 0 0x1.8p1", "rule 3 4 0x1.8p1 0", "rule 2 4 3 4", "rule 1 3 nan 2", "rule 1 2 7 0"])
    assert rows[:4, 0].tolist() == [0.0, 3.0, 3.0, 3.5] and np.isnan(rows[4, 0]) and rows[5, 0] == 7.0
