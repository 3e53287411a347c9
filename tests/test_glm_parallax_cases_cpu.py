"""CPU tests of the GLM parallax correction: the NumPy paths of tobac_flow_amd.geo / _lmatools / glm and the per-element
bodies of csrc/geodesy_kernels.h compiled for the host (tools/geodesy_check), against the mpmath oracles of
tests/glm_parallax_cases.py.  The tolerances are geodesy_cases.ANGLE_TOL (2^-48 rad) for a single step and VIEW_TOL
(2^-46 rad) for the chain of four; every figure is printed before it is asserted."""
import ctypes
import os
import re
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import geodesy_cases as gc
import glm_parallax_cases as pc
from tobac_flow_amd import _lmatools, geo, glm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def systems(sweep="x", lon_0=pc.LON_0):
    grid = geo.GeosProj(gc.H_GOES, lon_0, sweep=sweep)
    ltg = geo.GeosProj(gc.H_GOES, lon_0, sweep=sweep, a=pc.LTG_RE, rf=pc.LTG_RF)
    return grid, ltg


def goes_ds(lon_0=pc.LON_0):
    return gc.AbiLike(*gc.scan_grid(3, 3), lon_0=lon_0)


def check_unresolved(chain, dlon, dlat, x, y):
    """flashes beyond the limb, and rays that miss: NaN offsets, +inf scan angles; every other flash finite offsets"""
    ok = pc.resolved(chain)
    assert not ok[::10].any() and ok.sum() >= 50
    if dlon is not None:
        assert np.array_equal(np.isnan(dlon), ~ok) and np.array_equal(np.isnan(dlat), ~ok)
    if x is not None:
        assert np.isposinf(x[~ok]).all() and np.isposinf(y[~ok]).all() and not np.isnan(x).any() and not np.isnan(y).any()


# ---- single steps, NumPy path ----------------------------------------------------------------------------------------------
def test_ecef_to_geodetic_against_findroot():
    X, Y, Z, want = pc.ecef_points()
    lon, lat, alt = geo.ecef_to_geodetic(X, Y, Z, ellps="GRS80")
    err = pc.to_geodetic_errors(want, lon, lat, alt)
    print("lon, lat error (rad), height error (m):", err)
    assert err[0] <= gc.ANGLE_TOL and err[1] <= gc.ANGLE_TOL and err[2] <= pc.HEIGHT_TOL


def test_geodetic_to_ecef_closed_form_and_round_trip():
    rng = np.random.default_rng(12)
    lon, lat, alt = rng.uniform(-180, 180, 40), rng.uniform(-90, 90, 40), rng.uniform(-1e3, 2e4, 40)
    got = geo.geodetic_to_ecef(lon, lat, alt, ellps="GRS80")
    for k in range(40):
        want = pc.oracle_to_ecef(lon[k], lat[k], alt[k], *gc.GRS80)
        assert max(abs(float(mp.mpf(float(got[i][k])) - want[i])) for i in range(3)) <= pc.HEIGHT_TOL
    lon2, lat2, alt2 = geo.ecef_to_geodetic(*got, ellps="GRS80")
    away = np.abs(lat) < 89.9                                  # at a pole the longitude means nothing
    assert np.abs(np.radians(lon2 - lon))[away].max() <= gc.ANGLE_TOL and np.abs(np.radians(lat2 - lat)).max() <= gc.ANGLE_TOL
    assert np.abs(alt2 - alt).max() <= 2 * pc.HEIGHT_TOL
    sphere = geo.geodetic_to_ecef(90.0, 0.0, 0.0, a=6371000.0)
    assert abs(sphere[1] - 6371000.0) < 1e-9 and abs(sphere[0]) < 1e-9


def test_ecef_to_geodetic_edge_inputs():
    a, rf = gc.GRS80
    b = a * (1 - 1 / rf)
    X = np.array([0.0, 0.0, 0.0, np.nan, 1.0, np.inf, a + 16003.0])
    Y = np.array([0.0, 0.0, 0.0, 0.0, np.nan, np.inf, 0.0])
    Z = np.array([b + 5.0, -b - 7.0, 0.0, 1.0, 1.0, np.inf, 0.0])
    lon, lat, alt = geo.ecef_to_geodetic(X, Y, Z, ellps="GRS80")
    assert lon[:2].tolist() == [0.0, 0.0] and lat[:2].tolist() == [90.0, -90.0] and np.allclose(alt[:2], [5.0, 7.0], atol=1e-8)
    assert np.isnan(lon[2:6]).all() and np.isnan(lat[2:6]).all() and np.isnan(alt[2:6]).all()        # origin, NaN, infinity
    assert (lon[6], lat[6], alt[6]) == (0.0, 0.0, 16003.0)


@pytest.mark.parametrize("sweep", ["x", "y"])
def test_fixed_grid_to_ecef_backward_error(sweep):
    """the point's scan angles by the oracle are the input's within 2^-48 rad, the point lies on the ellipsoid within
    2^-48, a ray misses exactly where the oracle's does and gives +inf"""
    x, y, hit = pc.scan_points(sweep=sweep)
    assert 5 <= (~hit).sum() <= 20
    ltg = systems(sweep)[1]
    X, Y, Z = ltg.to_ecef(x, y)
    assert all(np.array_equal(np.isposinf(v), ~hit) and not np.isnan(v).any() for v in (X, Y, Z))
    angle, resid = pc.to_ecef_errors(x, y, hit, X, Y, Z, sweep)
    print("backward error (rad), residual:", sweep, angle, resid)
    assert angle <= gc.ANGLE_TOL and resid <= gc.ANGLE_TOL
    assert np.isnan(ltg.to_ecef(np.array([np.nan]), np.array([0.0]))[0][0])


# ---- the chain, NumPy path -------------------------------------------------------------------------------------------------
def test_chain_against_the_oracle():
    lat, lon, chain = pc.flashes()
    ds = goes_ds()
    dlon, dlat = glm.get_glm_parallax_offsets(lon, lat, ds)
    x, y = glm.get_corrected_glm_x_y(lon, lat, ds)
    check_unresolved(chain, dlon, dlat, x, y)
    err = pc.chain_errors(chain, dlon, dlat, x, y)
    print("chain errors (rad): dlon, dlat, x, y", err)
    assert (err <= gc.VIEW_TOL).all()
    assert sum(c.get("x") == mp.inf for c in chain) >= 1         # near the limb the correction pushes a flash over it
    for k in pc.NEAR_LIMB:
        assert abs(dlon[k]) > 0.5 or abs(dlat[k]) > 0.5          # degrees: the correction is large there


def test_known_answers():
    ds = goes_ds()
    dlon, dlat = glm.get_glm_parallax_offsets(np.array([-75.0, -95.0, -130.0]), np.array([0.0, 35.0, 60.0]), ds)
    assert dlon[0] == 0.0 and dlat[0] == 0.0                     # exactly, at the sub-satellite point
    assert abs(dlon[1] - 0.0622015784) < 1e-9 and abs(dlat[1] + 0.0807507994) < 1e-9
    assert abs(dlon[2] - 0.6414194) < 1e-6 and abs(dlat[2] + 0.1974197) < 1e-6
    grid, ltg = systems()
    alt = geo._np_glm_parallax(grid, ltg, *gc.GRS80, np.array([0.0, 35.0]), np.array([-75.0, -95.0]))[4]
    assert alt[0] == 16003.0 and abs(alt[1] - 12728.4) < 0.05
    x, y = glm.get_corrected_glm_x_y(np.array([-75.0]), np.array([0.0]), ds)
    assert x[0] == 0.0 and y[0] == 0.0
    # the same through the reference's own route, its coordinate-system classes
    geofix_ltg, _ = _lmatools.get_GOESR_coordsys_alt_ellps(-75.0)
    _, grs80lla = _lmatools.get_GOESR_coordsys(-75.0)
    lon_l, lat_l, alt_l = grs80lla.fromECEF(*geofix_ltg.toECEF(np.zeros(1), np.zeros(1), np.zeros(1)))
    assert abs(lon_l[0] + 75.0) < 1e-13 and lat_l[0] == 0.0 and abs(alt_l[0] - 16003.0) <= pc.HEIGHT_TOL
    assert _lmatools.lightning_ellipse_rev == {0: (6.394140e6, 6.362755e6), 1: (6.378137e6 + 14.0e3, 6.362755e6)}
    assert (_lmatools.ltg_ellps_re, _lmatools.ltg_ellps_rp) == (6.394140e6, 6.362755e6)
    assert _lmatools.semiaxes_to_invflattening(6.394140e6, 6.362755e6) == 6.394140e6 / (6.394140e6 - 6.362755e6)
    assert geofix_ltg.proj.rf == pc.LTG_RF and geofix_ltg.h == 35786023.0 and grs80lla.rf == gc.GRS80[1]


def test_class_route_equals_the_fused_chain():
    """get_glm_parallax_offsets written with the coordinate-system classes, as the reference writes it, agrees with the
    fused form within the chain's bound away from the limb (near it the route through rounded scan angles is the worse
    conditioned of the two and is not held to it)"""
    from tobac_flow_amd import abi
    lat, lon, chain = pc.flashes()
    ds = goes_ds()
    x, y = abi.get_abi_x_y(lat, lon, ds)
    geofix_ltg, _ = _lmatools.get_GOESR_coordsys_alt_ellps(-75.0)
    _, grs80lla = _lmatools.get_GOESR_coordsys(-75.0)
    lon_l, lat_l, _ = grs80lla.fromECEF(*geofix_ltg.toECEF(x, y, np.zeros_like(x)))
    dlon, dlat = glm.get_glm_parallax_offsets(lon, lat, ds)
    inner = pc.resolved(chain)
    inner[list(pc.NEAR_LIMB)] = False
    assert np.abs(np.radians((lon_l - lon) - dlon))[inner].max() <= gc.VIEW_TOL
    assert np.abs(np.radians((lat_l - lat) - dlat))[inner].max() <= gc.VIEW_TOL
    assert np.isnan(lon_l[~pc.resolved(chain)]).all()


def test_float32_nan_and_other_inputs():
    lat, lon, chain = pc.flashes()
    ds = goes_ds()
    lat32, lon32 = lat.astype(np.float32), lon.astype(np.float32)
    got32 = glm.get_glm_parallax_offsets(lon32, lat32, ds) + glm.get_corrected_glm_x_y(lon32, lat32, ds)
    got64 = (glm.get_glm_parallax_offsets(lon32.astype(np.float64), lat32.astype(np.float64), ds)
             + glm.get_corrected_glm_x_y(lon32.astype(np.float64), lat32.astype(np.float64), ds))
    assert all(a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True) for a, b in zip(got32, got64))
    bad_lat, bad_lon = np.array([np.nan, 10.0, np.nan]), np.array([-80.0, np.nan, np.nan])
    out = glm.get_glm_parallax_offsets(bad_lon, bad_lat, ds) + glm.get_corrected_glm_x_y(bad_lon, bad_lat, ds)
    assert all(np.isnan(v).all() for v in out)
    assert all(v.size == 0 for v in glm.get_corrected_glm_x_y(np.array([]), np.array([]), ds))
    assert all(v.size == 0 for v in glm.get_uncorrected_glm_x_y(np.array([]), np.array([]), ds))
    wrapped = glm.get_glm_parallax_offsets(np.array([265.0]), np.array([35.0]), ds)                 # 265 = -95 + 360
    assert abs(wrapped[0][0] + 360.0 - 0.0622015784) < 1e-9      # the lightning longitude comes back within [-180, 180]
    late = glm.get_glm_parallax_offsets(np.array([-95.0]), np.array([35.0]), ds, ellipse_rev=1)
    assert 0.05 < late[0][0] < 0.0622 and -0.0807 < late[1][0] < -0.05                                # the lower ellipsoid of 2018
    west = glm.get_glm_parallax_offsets(np.array([-137.0]), np.array([0.0]), goes_ds(-137.0))
    assert west[0][0] == 0.0 and west[1][0] == 0.0
    with pytest.raises(ValueError, match="sweep"):
        glm.get_glm_parallax_offsets(lon, lat, gc.AbiLike(*gc.scan_grid(3, 3), sweep="y"))


def test_a_ray_that_misses_the_lightning_ellipsoid():
    """with the flight parameters no ray towards a visible point misses (the lightning ellipsoid is the larger one; the
    case builder's oracle confirms it), so the miss is built: a `lightning` sphere well inside the Earth"""
    lat, lon, chain = pc.flashes()
    assert all(c["disc"] is None or c["disc"] > 0 for c in chain)
    grid = systems()[0]
    small = geo.GeosProj(gc.H_GOES, pc.LON_0, a=4.0e6)
    lat, lon = np.array([0.0, 20.0, 60.0, 75.0]), np.array([-75.0, -60.0, -100.0, -75.0])
    want = [pc.oracle_chain(float(la), float(lo), ltg=(4.0e6, 0.0)) for la, lo in zip(lat, lon)]
    hit = pc.resolved(want)
    assert hit.tolist() == [True, True, False, False] and all(abs(c["disc"]) > 1e-9 for c in want)
    dlon, dlat, x, y = geo.glm_parallax(grid, small, gc.GRS80, lat, lon)
    assert np.array_equal(np.isnan(dlon), ~hit) and np.array_equal(np.isnan(dlat), ~hit)
    assert np.isposinf(x[~hit]).all() and np.isposinf(y[~hit]).all()
    assert (pc.chain_errors(want, dlon, dlat, x, y) <= gc.VIEW_TOL).all()


# ---- the coordinate-system classes -----------------------------------------------------------------------------------------
def test_coordinate_system_round_trips():
    rng = np.random.default_rng(13)
    lon, lat, alt = rng.uniform(-180, 180, 30), rng.uniform(-89, 89, 30), rng.uniform(0, 2e4, 30)
    for system in (_lmatools.GeographicSystem(), _lmatools.GeographicSystem(ellipse="GRS80"),
                   _lmatools.GeographicSystem(r_equator=6371000.0),
                   _lmatools.GeographicSystemAltEllps(r_equator=pc.LTG_RE, r_pole=pc.LTG_RP)):
        back = system.fromECEF(*system.toECEF(lon, lat, alt))
        assert np.abs(np.radians(back[0] - lon)).max() <= gc.ANGLE_TOL and np.abs(np.radians(back[1] - lat)).max() <= gc.ANGLE_TOL
        assert np.abs(back[2] - alt).max() <= 2 * pc.HEIGHT_TOL
    assert _lmatools.GeographicSystem().toECEF(0.0, 0.0, 0.0)[0].shape == (1,)                        # scalars: arrays of one
    assert _lmatools.GeographicSystemAltEllps(r_equator=pc.LTG_RE, r_pole=pc.LTG_RP).rf == pc.LTG_RF
    assert _lmatools.GeographicSystem(r_equator=6371000.0).rf == 0.0
    x, y, hit = pc.scan_points()
    for system in (_lmatools.get_GOESR_coordsys(-75.0)[0], _lmatools.get_GOESR_coordsys_alt_ellps(-75.0)[0],
                   _lmatools.GeostationaryFixedGridSystem(subsat_lon=9.5), _lmatools.GeostationaryFixedGridSystemAltEllipse(
                       subsat_lon=-137.0, sweep_axis="x", semimajor_axis=pc.LTG_RE, semiminor_axis=pc.LTG_RP)):
        X, Y, Z = system.toECEF(x[hit], y[hit], np.zeros(hit.sum()))
        bx, by, bz = system.fromECEF(X, Y, Z)
        assert np.abs(bx - x[hit]).max() <= gc.VIEW_TOL and np.abs(by - y[hit]).max() <= gc.VIEW_TOL
        assert np.abs(bz * system.h).max() <= pc.HEIGHT_TOL                                         # on the ellipsoid: height 0
        with pytest.raises(ValueError, match="z must be 0"):
            system.toECEF(x[:2], y[:2], np.array([0.0, 1e-3]))
    assert _lmatools.GeostationaryFixedGridSystem().proj.sweep == "y" and _lmatools.GeostationaryFixedGridSystem().h == 35785831.0
    with pytest.raises(ValueError):
        _lmatools.GeographicSystem(ellipse="clarke")


# ---- regridding and the dataset --------------------------------------------------------------------------------------------
def test_regrid_glm_lat_lon():
    c = pc.regrid_case()
    args = (c["flash_lat"], c["flash_lon"], c["flash_file"], c["file_times"], c["ds"], c["goes_dates"], c["x_bins"], c["y_bins"])
    corrected = glm.regrid_glm_lat_lon(*args, corrected=True)
    assert corrected.shape == (3, 7, 9) and corrected.dtype == np.int64
    assert np.array_equal(corrected, c["corrected"])
    assert (corrected[2] == -1).all() and (corrected[:2] >= 0).all()
    plain = glm.regrid_glm_lat_lon(*args)
    assert np.array_equal(plain, c["uncorrected"]) and not np.array_equal(plain, corrected)
    ys, xs = np.nonzero(corrected[0])
    yu, xu = np.nonzero(plain[0])
    assert abs(ys.mean() - yu.mean()) > 2                        # the correction moves the flashes by several pixels
    for f, want in ((glm.get_corrected_glm_hist, corrected), (glm.get_uncorrected_glm_hist, plain)):
        hist = f(*args[:5], np.datetime64("2018-06-19T16:57:30"), np.datetime64("2018-06-19T17:02:30"))
        assert hist.dtype == np.float64 and np.array_equal(hist, want[0])
        with pytest.raises(ValueError, match="no GLM file"):
            f(*args[:5], np.datetime64("2018-06-19T17:32:30"), np.datetime64("2018-06-19T17:47:30"))


def test_create_gridded_flash_ds():
    from tobac_flow_amd import dataset
    c = pc.regrid_case()
    ds = glm.create_gridded_flash_ds(c["ds"], c["flash_lat"], c["flash_lon"], c["flash_file"], c["file_times"])
    assert isinstance(ds, dataset.LabelDataset) and {"lat", "lon", "area", "glm_flashes", "glm_flash_count"} <= set(ds)
    assert ds["glm_flashes"].dtype == np.int32 and ds.dims["glm_flashes"] == ("t", "y", "x")
    assert np.array_equal(ds["glm_flashes"], c["corrected"])
    assert ds["glm_flash_count"].dtype == np.int32 and ds["glm_flash_count"].shape == () and ds.dims["glm_flash_count"] == ()
    assert int(ds["glm_flash_count"]) == int(c["corrected"][c["corrected"] > 0].sum()) > 0
    with pytest.raises(ValueError, match="No GLM Files"):
        glm.create_gridded_flash_ds(c["ds"], c["flash_lat"][:0], c["flash_lon"][:0], c["flash_file"][:0], c["file_times"][:0])


# ---- the C ABI and the bodies on the host ----------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_check_their_arguments():
    from tobac_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("tf_ecef", "tf_geos_to_ecef", "tf_glm_parallax"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS
    assert re.search(r"#define\s+TF_ECEF_FROM_GEODETIC\s+0", header) and re.search(r"#define\s+TF_ECEF_TO_GEODETIC\s+1", header)
    L = _lib.lib()
    assert L.tf_version() >= 116
    ok = _lib.Geos(gc.H_GOES, -75.0, 0.0, *gc.GRS80, 0, 0)
    ltg = _lib.Geos(gc.H_GOES, -75.0, 0.0, pc.LTG_RE, pc.LTG_RF, 0, 0)
    bad = _lib.Geos(gc.H_GOES, -75.0, 1.0, *gc.GRS80, 0, 0)
    ref = ctypes.byref
    a, rf = gc.GRS80
    def parallax(grid, other, n, dtype=_lib.TF_F64):
        return L.tf_glm_parallax(ref(grid), ref(other), a, rf, None, None, dtype, n, None, None, None, None, None)
    assert L.tf_geos_to_ecef(ref(bad), None, None, 0, None, None, None, None) == -1 and "lat_0" in L.tf_last_error().decode()
    assert parallax(bad, ltg, 0) == -1 and "lat_0" in L.tf_last_error().decode()
    assert parallax(ok, bad, 0) == -1 and "lat_0" in L.tf_last_error().decode()
    assert L.tf_geos_to_ecef(ref(ok), None, None, 0, None, None, None, None) == 0                        # n = 0: a successful no-op
    assert parallax(ok, ltg, 0) == 0
    assert L.tf_ecef(_lib.ECEF_TO_GEODETIC, a, rf, None, None, None, 0, None, None, None, None) == 0
    assert L.tf_ecef(_lib.ECEF_TO_GEODETIC, a, rf, None, None, None, 4, None, None, None, None) == -1    # null pointers
    assert L.tf_ecef(2, a, rf, None, None, None, 0, None, None, None, None) == -1
    assert L.tf_ecef(_lib.ECEF_FROM_GEODETIC, -1.0, rf, None, None, None, 0, None, None, None, None) == -1
    assert L.tf_geos_to_ecef(ref(ok), None, None, 4, None, None, None, None) == -1
    assert parallax(ok, ltg, 4) == -1
    assert parallax(ok, ltg, 0, _lib.TF_I32) == -1
    assert parallax(ok, _lib.Geos(gc.H_GOES, -137.0, 0.0, pc.LTG_RE, pc.LTG_RF, 0, 0), 0) == -1
    assert "lon_0" in L.tf_last_error().decode()


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


def test_bodies_on_the_host_single_steps(host_check):
    """gd_ecef_to_geodetic_one, gd_geodetic_to_ecef_one and gd_geos_to_ecef_one, the text the device runs: the same bounds"""
    X, Y, Z, want = pc.ecef_points()
    rows = host_check([f"fromecef {_hex(*gc.GRS80, X[k], Y[k], Z[k])}" for k in range(X.size)])
    err = pc.to_geodetic_errors(want, rows[:, 0], rows[:, 1], rows[:, 2])
    print("host ECEF -> geodetic:", err)
    assert err[0] <= gc.ANGLE_TOL and err[1] <= gc.ANGLE_TOL and err[2] <= pc.HEIGHT_TOL
    b = gc.GRS80[0] * (1 - 1 / gc.GRS80[1])
    rows = host_check([f"fromecef {_hex(*gc.GRS80)} {tail}" for tail in
                       (f"0 0 {(b + 5.0).hex()}", f"0 0 {(-b - 7.0).hex()}", "0 0 0", "nan 0 1", "inf inf inf", f"{(gc.GRS80[0] + 16003.0).hex()} 0 0")])
    assert rows[0, :2].tolist() == [0.0, 90.0] and rows[1, :2].tolist() == [0.0, -90.0] and abs(rows[0, 2] - 5.0) < 1e-8
    assert np.isnan(rows[2:5]).all() and rows[5].tolist() == [0.0, 0.0, 16003.0]
    rng = np.random.default_rng(12)
    lon, lat, alt = rng.uniform(-180, 180, 40), rng.uniform(-90, 90, 40), rng.uniform(-1e3, 2e4, 40)
    rows = host_check([f"toecef {_hex(*gc.GRS80, lon[k], lat[k], alt[k])}" for k in range(40)])
    for k in range(40):
        want_k = pc.oracle_to_ecef(lon[k], lat[k], alt[k], *gc.GRS80)
        assert max(abs(float(mp.mpf(rows[k, i]) - want_k[i])) for i in range(3)) <= pc.HEIGHT_TOL
    for sweep in ("x", "y"):
        x, y, hit = pc.scan_points(sweep=sweep)
        rows = host_check([f"geos2ecef {_hex(gc.H_GOES, pc.LON_0, pc.LTG_RE, pc.LTG_RF, sweep == 'y', x[k], y[k])}" for k in range(x.size)])
        assert np.array_equal(rows[:, 3] == 1, hit) and np.isposinf(rows[~hit, :3]).all()
        angle, resid = pc.to_ecef_errors(x, y, hit, rows[:, 0], rows[:, 1], rows[:, 2], sweep)
        print("host fixed grid -> ECEF:", sweep, angle, resid)
        assert angle <= gc.ANGLE_TOL and resid <= gc.ANGLE_TOL


def test_bodies_on_the_host_chain(host_check):
    lat, lon, chain = pc.flashes()
    head = _hex(gc.H_GOES, pc.LON_0, *gc.GRS80, 0, gc.H_GOES, pc.LTG_RE, pc.LTG_RF, *gc.GRS80)
    rows = host_check([f"parallax {head} {_hex(lat[k], lon[k])}" for k in range(lat.size)] + [f"parallax {head} nan 0", f"parallax {head} 0 nan"])
    n = lat.size
    dlon, dlat, x, y, alt = rows[:n, :5].T
    check_unresolved(chain, dlon, dlat, x, y)
    assert np.array_equal(rows[:n, 5] == 1, pc.resolved(chain))
    err = pc.chain_errors(chain, dlon, dlat, x, y)
    print("host chain errors (rad):", err)
    assert (err <= gc.VIEW_TOL).all()
    assert rows[pc.SUBSATELLITE, :5].tolist() == [0.0, 0.0, 0.0, 0.0, 16003.0]
    assert np.isnan(rows[n:, :5]).all()
    heights = [abs(float(mp.mpf(alt[k]) - c["alt"])) for k, c in enumerate(chain) if "alt" in c]
    assert max(heights) <= 4 * pc.HEIGHT_TOL                     # four steps
