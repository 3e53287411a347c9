"""Oracles and case builders of the geodesy tests (tests/test_geodesy_cases_cpu.py, tests/test_gpu_geodesy.py).

pyproj is not available, so the yardstick is mathematics in mpmath at 40 digits, and neither oracle restates the algorithm
under test:

  projection   geometric: geodetic -> ECEF -> satellite frame -> the two scan angles (`oracle_forward`), and the
               ray-ellipsoid discriminant of a pair of scan angles (`oracle_discriminant`).  The inverse under test is
               judged by its backward error: its (lat, lon) projected forward by the oracle must give the scan angles back.
  geodesic     the DIRECT problem by quadrature on the auxiliary sphere (`direct`): from (lat1, azimuth1, arc length) the
               second point, the distance and the azimuth there, to 40 digits.  The inverse under test gets the two points.

A module-level cache holds every mpmath result: each case is integrated once per session.
"""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 40

WGS84 = (6378137.0, 298.257223563)
GRS80 = (6378137.0, 298.257222101)
H_GOES = 35786023.0
ANGLE_TOL = 2.0 ** -48            # rad: projection, forward error and backward error
VIEW_TOL = 2.0 ** -46             # rad: viewing angles


def _deg(v):
    return mp.mpf(float(v)) * mp.pi / 180


# ---- projection ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_forward(lat, lon, h=H_GOES, lon_0=-75.0, sweep="x", a=GRS80[0], rf=GRS80[1]):
    """scan angles (x, y) in radians, as mpf, of the point at geodetic (lat, lon) degrees on the ellipsoid"""
    f = 1 / mp.mpf(rf) if rf else mp.mpf(0)
    e2 = f * (2 - f)
    phi, lam = _deg(lat), _deg(lon) - _deg(lon_0)
    nu = mp.mpf(a) / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    X, Y, Z = nu * mp.cos(phi) * mp.cos(lam), nu * mp.cos(phi) * mp.sin(lam), nu * (1 - e2) * mp.sin(phi)
    dx = mp.mpf(a) + mp.mpf(h) - X                           # from the satellite towards the Earth's centre
    if sweep == "x":
        return mp.atan2(Y, mp.hypot(Z, dx)), mp.atan2(Z, dx)
    return mp.atan2(Y, dx), mp.atan2(Z, mp.hypot(Y, dx))


@functools.lru_cache(maxsize=None)
def oracle_discriminant(x, y, h=H_GOES, sweep="x", a=GRS80[0], rf=GRS80[1]):
    """(B^2 - 4 A C) / B^2 of the intersection of the ray with scan angles (x, y) and the ellipsoid: negative off the disk"""
    f = 1 / mp.mpf(rf) if rf else mp.mpf(0)
    x, y = mp.mpf(float(x)), mp.mpf(float(y))
    if sweep == "x":
        d = (-mp.cos(x) * mp.cos(y), mp.sin(x), mp.cos(x) * mp.sin(y))
    else:
        d = (-mp.cos(y) * mp.cos(x), mp.cos(y) * mp.sin(x), mp.sin(y))
    rg = 1 + mp.mpf(h) / mp.mpf(a)
    A = d[0] ** 2 + d[1] ** 2 + d[2] ** 2 / (1 - f) ** 2
    B = 2 * rg * d[0]
    C = rg ** 2 - 1
    return (B * B - 4 * A * C) / (B * B)


def scan_grid(H, W, span=0.1518):
    """1-D scan angles (x (W), y (H)) spanning +-span rad, y descending as in an ABI file, nudged so that no pixel sits
    within 1e-9 of the limb for either sweep (asserted): the on / off decision never hangs on rounding"""
    x = np.linspace(-span, span, W) + 1.3e-5 if W > 1 else np.array([0.0213])
    y = np.linspace(span, -span, H) - 0.7e-5 if H > 1 else np.array([0.0917])
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


@functools.lru_cache(maxsize=None)
def grid_on_disk(H, W, sweep="x", span=0.1518):
    """bool (H, W): the oracle's discriminant is positive"""
    x, y = scan_grid(H, W, span)
    disc = np.array([[float(oracle_discriminant(float(xj), float(yi), sweep=sweep)) for xj in x] for yi in y])
    assert np.abs(disc).min() >= 1e-9, "a pixel of the test grid sits on the limb"
    return disc > 0


def backward_error(lat, lon, x, y, on_disk, sweep="x", lon_0=-75.0):
    """max over the on-disk pixels of |oracle_forward(lat, lon) - (x, y)| in radians; lat, lon (H, W), x (W), y (H)"""
    worst = 0.0
    for i, j in zip(*np.nonzero(on_disk)):
        ox, oy = oracle_forward(float(lat[i, j]), float(lon[i, j]), lon_0=lon_0, sweep=sweep)
        worst = max(worst, abs(float(ox - mp.mpf(float(x[j])))), abs(float(oy - mp.mpf(float(y[i])))))
    return worst


def forward_points(n, seed=5, lon_0=-75.0):
    """n (lat, lon) points in degrees: most on the visible disk, every tenth beyond the limb"""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-70, 70, n)
    lon = lon_0 + rng.uniform(-65, 65, n)
    lon[::10] = lon_0 + rng.uniform(100, 170, lon[::10].size)
    return lat, lon


# ---- geodesic --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct(lat1, lon1, az1, sig12, a=WGS84[0], rf=WGS84[1]):
    """the direct geodesic problem by quadrature on the auxiliary sphere: from (lat1, lon1) at azimuth az1 over the arc
    sig12 (all degrees) -> (lat2, lon2, az2 in degrees, s12 in the unit of a), mpf"""
    f = 1 / mp.mpf(rf) if rf else mp.mpf(0)
    b = mp.mpf(a) * (1 - f)
    ep2 = f * (2 - f) / (1 - f) ** 2
    phi1, alp1, s12 = _deg(lat1), _deg(az1), _deg(sig12)
    if abs(lat1) == 90:
        sbet1, cbet1 = mp.mpf(np.sign(lat1)), mp.mpf(0)
    else:
        bet1 = mp.atan((1 - f) * mp.tan(phi1))
        sbet1, cbet1 = mp.sin(bet1), mp.cos(bet1)
    salp0 = mp.sin(alp1) * cbet1
    calp0 = mp.hypot(mp.cos(alp1), mp.sin(alp1) * sbet1)
    sig1 = mp.atan2(sbet1, mp.cos(alp1) * cbet1)
    sig2 = sig1 + s12
    k2 = ep2 * calp0 ** 2
    root = lambda s: mp.sqrt(1 + k2 * mp.sin(s) ** 2)
    dist = b * mp.quad(root, [sig1, sig2])
    omg = lambda s: mp.atan2(salp0 * mp.sin(s), mp.cos(s))
    # the longitude on the auxiliary sphere changes by less than pi over an arc shorter than pi; a line that starts at a
    # pole runs along the meridian lon1 that its azimuth is counted from
    w12 = mp.mpf(0) if cbet1 == 0 else omg(sig2) - omg(sig1)
    w12 -= 2 * mp.pi * mp.nint(w12 / (2 * mp.pi))
    lam12 = w12 - f * salp0 * mp.quad(lambda s: (2 - f) / (1 + (1 - f) * root(s)), [sig1, sig2])
    bet2 = mp.asin(calp0 * mp.sin(sig2))
    alp2 = mp.atan2(salp0, calp0 * mp.cos(sig2))
    phi2 = mp.atan(mp.tan(bet2) / (1 - f)) if abs(calp0 * mp.sin(sig2)) < 1 else bet2
    return phi2 * 180 / mp.pi, mp.mpf(float(lon1)) + lam12 * 180 / mp.pi, alp2 * 180 / mp.pi, dist


def _case_list():
    """(lat1, lon1, az1, sig12) of about 200 lines: sig12 from 3e-4 (30 m) to 170 degrees, all azimuth quadrants, |lat1| up to
    89, meridional and equatorial lines, pairs across +-180 longitude, both poles as an end point, pixel spacings"""
    rng = np.random.default_rng(11)
    cases = []
    sigs = [3e-4, 4.5e-3, 0.02, 0.18, 1.0, 9.0, 45.0, 89.0, 91.0, 135.0, 150.0, 170.0]
    for k, sig in enumerate(sigs):
        for q in range(8):                                      # two azimuths per quadrant, another latitude per line
            az = 45.0 * q + rng.uniform(3, 42) - 180.0
            lat = [0.0, 33.0, -47.0, 71.0, -89.0, 89.0, 12.5, -5.0][(k + q) % 8]
            cases.append((lat, rng.uniform(-180, 180), az, sig))
    for sig in (3e-4, 0.05, 1.0, 30.0, 100.0, 170.0):
        cases += [(0.0, 10.0, 90.0, sig), (0.0, -20.0, -90.0, sig)]                    # equatorial
        cases += [(-30.0, 40.0, 0.0, sig), (65.0, -100.0, 180.0, sig)]                 # meridional (65 N going south; -30 going north)
        cases += [(20.0, 179.9, 70.0, max(sig, 0.2)), (-35.0, -179.95, -110.0, max(sig, 0.2))]     # across +-180
    for lat in (-60.0, 0.0, 45.0, 80.0):
        cases.append((lat, 25.0, 0.0, 90.0 - _reduced(lat)))                           # ends at the north pole
        cases.append((lat, 25.0, 180.0, 90.0 + _reduced(lat)))                         # ends at the south pole
        cases.append((90.0, -60.0, 180.0, 90.0 - _reduced(lat) if lat != 80.0 else 0.01))           # starts at the north pole
        cases.append((-90.0, 130.0, 0.0, 15.0 + lat / 10))                             # starts at the south pole
    for km in (0.5, 1.0, 2.0, 4.2, 7.7, 12.0, 20.0):                                   # neighbouring pixels
        for lat, az in ((0.0, 90.0), (35.0, 1.0), (-52.0, -91.0), (68.0, 179.0), (15.0, 45.0), (-75.0, -135.0), (40.0, 88.0)):
            cases.append((lat, rng.uniform(-180, 180), az, km / 111.2))
    return cases


def _reduced(lat):
    f = 1 / WGS84[1]
    return float(np.degrees(np.arctan((1 - f) * np.tan(np.radians(lat)))))


@functools.lru_cache(maxsize=None)
def geodesic_cases():
    """dict of float64 arrays lon1, lat1, lon2, lat2 (what the inverse under test gets, the second point rounded to
    float64 and wrapped into [-180, 180]) and of object arrays of mpf: s12, az1, az2 (degrees) and sig12 (degrees)"""
    rows = _case_list()
    out = {k: [] for k in ("lon1", "lat1", "lon2", "lat2", "s12", "az1", "az2", "sig12")}
    for lat1, lon1, az1, sig12 in rows:
        lat2, lon2, az2, s12 = direct(float(lat1), float(lon1), float(az1), float(sig12))
        lon2 = float(lon2)
        lon2 = (lon2 + 180.0) % 360.0 - 180.0 if abs(lon2) > 180.0 else lon2
        for k, v in zip(out, (lon1, lat1, lon2, min(90.0, max(-90.0, float(lat2))), s12, az1, az2, sig12)):
            out[k].append(v)
    return {k: (np.array(v, dtype=np.float64) if k in ("lon1", "lat1", "lon2", "lat2", "sig12") else v) for k, v in out.items()}


def _angle_diff(got_deg, want_deg):
    d = (mp.mpf(float(got_deg)) - want_deg) % 360
    return float(min(d, 360 - d)) * np.pi / 180


def geodesic_errors(az12, az21, dist, cases=None, a=WGS84[0]):
    """per case (|ds|, lateral error of az12, lateral error of az21, bound), all in metres: the bound is 1e-8 m + 1e-11 s
    for the distance, and for each azimuth the same figure against |d alpha| a |sin sig12|.  az21 is pyproj's back azimuth:
    the oracle's az2 turned by 180 degrees."""
    cases = cases or geodesic_cases()
    rows = []
    for k in range(len(cases["s12"])):
        s = cases["s12"][k]
        lever = a * abs(np.sin(np.radians(cases["sig12"][k])))
        rows.append((abs(float(mp.mpf(float(dist[k])) - s)), _angle_diff(az12[k], mp.mpf(cases["az1"][k])) * lever,
                     _angle_diff(az21[k], cases["az2"][k] + 180) * lever, 1e-8 + 1e-11 * float(s)))
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def antipodal_cases():
    """pairs beyond sig12 = 170 degrees, where only the no-silent-error rule applies: lines of 179.5 degrees, and exact
    antipodes (the oracle's distance for those is not used: any answer but NaN is judged against the meridional one)"""
    rows = [(10.0, 20.0, 33.0, 179.5), (-40.0, -100.0, -120.0, 179.5), (0.0, 0.0, 90.0, 179.5), (0.0, 50.0, 89.0, 179.5), (60.0, 0.0, 5.0, 179.5),
            (0.0, 0.0, 90.0, 179.9), (30.0, 10.0, 60.0, 179.95)]
    out = {k: [] for k in ("lon1", "lat1", "lon2", "lat2", "s12", "az1", "az2", "sig12")}
    for lat1, lon1, az1, sig12 in rows:
        lat2, lon2, az2, s12 = direct(lat1, lon1, az1, sig12)
        lon2 = float(lon2)
        lon2 = (lon2 + 180.0) % 360.0 - 180.0 if abs(lon2) > 180.0 else lon2
        for k, v in zip(out, (lon1, lat1, lon2, float(lat2), s12, az1, az2, sig12)):
            out[k].append(v)
    out = {k: (np.array(v, dtype=np.float64) if k in ("lon1", "lat1", "lon2", "lat2", "sig12") else v) for k, v in out.items()}
    exact = {"lon1": np.array([0.0, 30.0, -120.0]), "lat1": np.array([0.0, 45.0, -10.0]), "lon2": np.array([180.0, -150.0, 60.0]),
             "lat2": np.array([0.0, -45.0, 10.0])}
    return out, exact


# ---- viewing angles --------------------------------------------------------------------------------------------------------
def view_points(n=60, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-65, 65, n), rng.uniform(-150, 10, n)


def mp_sunh(delta, eqt, hour, lat, lon):
    delta, eqt, hour = (mp.mpf(float(v)) for v in (delta, eqt, hour))
    omega = (15 * (hour + mp.mpf(float(lon)) / 15 + eqt - 12)) * mp.pi / 180
    rl = _deg(lat)
    sunh = mp.sin(delta) * mp.sin(rl) + mp.cos(delta) * mp.cos(rl) * mp.cos(omega)
    azi = (mp.sin(delta) * mp.cos(rl) - mp.cos(delta) * mp.sin(rl) * mp.cos(omega))
    return sunh, azi


def mp_sza(delta, eqt, hour, lat, lon):
    """get_sza in mpmath: (zenith in rad, sunh)"""
    sunh, _ = mp_sunh(delta, eqt, hour, lat, lon)
    return mp.pi / 2 - mp.asin(sunh), sunh


def mp_sza_and_azi(delta, eqt, hour, lat, lon):
    """get_sza_and_azi in mpmath: (zenith deg, azimuth deg, the two clipped arguments)"""
    sunh, num = mp_sunh(delta, eqt, hour, lat, lon)
    clip = lambda v: max(mp.mpf(-1), min(mp.mpf(1), v))
    sza = mp.pi / 2 - mp.asin(clip(sunh))
    azi = num / mp.cos(mp.pi / 2 - sza)
    return sza * 180 / mp.pi, mp.acos(clip(azi)) * 180 / mp.pi, sunh, azi


def mp_satellite(lat, lon, sat_lat=0.0, sat_lon=0.0, sat_alt=35793.0):
    """get_satellite_viewing_angles in mpmath: (zenith deg, azimuth deg, the arcsin argument)"""
    re = mp.mpf(6371)
    rgeo = mp.mpf(float(sat_alt)) + re
    dlat, dlon = _deg(lat) - _deg(sat_lat), _deg(lon) - _deg(sat_lon)
    cos_beta = mp.cos(dlat) * mp.cos(dlon)
    sin_beta = mp.sin(mp.acos(cos_beta))
    dist = mp.sqrt(rgeo ** 2 + re ** 2 - 2 * rgeo * re * cos_beta)
    sin_theta = rgeo * sin_beta / dist
    zen = mp.asin(sin_theta) * 180 / mp.pi
    if not dist ** 2 < rgeo ** 2 - re ** 2:
        zen = 180 - zen
    azi = (mp.atan2(mp.cos(dlat) * mp.sin(dlon), mp.sin(dlat)) * 180 / mp.pi) % 360
    return zen, azi, sin_theta


def mp_abi_zenith(lat, lon, sx, sy, lat_0=0.0, lon_0=-75.0):
    """get_abi_zenith_angle in mpmath: (angle deg, the arccos argument)"""
    dlat, dlon = _deg(lat) - _deg(lat_0), _deg(lon) - _deg(lon_0)
    xx, yy = -mp.mpf(float(sx)), -mp.mpf(float(sy))
    dot = (mp.cos(dlon) * mp.sin(dlat) * mp.cos(xx) * mp.sin(yy) + mp.sin(dlon) * mp.sin(xx)
           + mp.cos(dlon) * mp.cos(dlat) * mp.cos(xx) * mp.cos(yy))
    return mp.acos(dot) * 180 / mp.pi, dot


def _rad_err(got_deg, want_deg):
    return abs(float(mp.mpf(float(got_deg)) - want_deg)) * np.pi / 180


def view_angle_errors(run):
    """worst error in radians per mode of `run(mode, scalars, lat, lon, x, y) -> (out0, out1)` against the reference
    functions evaluated in mpmath, over points whose arcsin / arccos arguments stay 1e-6 away from the clip points (there
    only finiteness and the clip are checked)"""
    from datetime import datetime
    from tobac_flow_amd import geo
    lat, lon = view_points()
    date = datetime(2019, 7, 14, 18, 40)
    worst = {}
    sc = geo.sza_scalars(date)
    got = run(0, sc, lat, lon, None, None)[0]
    worst[0] = max(abs(float(mp.mpf(float(got[k])) - mp_sza(*sc, lat[k], lon[k])[0])) for k in range(lat.size))
    day = int(date.strftime("%j"))
    sc = (geo._declination(2.0 * np.pi * day / 365.0), geo._equation_of_time(2.0 * np.pi * day / 366.0), 18 + 40 / 60)
    zen, azi = run(1, sc, lat, lon, None, None)
    worst[1] = 0.0
    for k in range(lat.size):
        want_zen, want_azi, sunh, arg = mp_sza_and_azi(*sc, lat[k], lon[k])
        assert np.isfinite(zen[k]) and np.isfinite(azi[k]) and 0 <= azi[k] <= 180
        if abs(abs(sunh) - 1) > 1e-6 and abs(abs(arg) - 1) > 1e-6:
            worst[1] = max(worst[1], _rad_err(zen[k], want_zen), _rad_err(azi[k], want_azi))
    sc = (0.0, -75.0, 35793.0)
    zen, azi = run(2, sc, lat, lon, None, None)
    worst[2] = 0.0
    for k in range(lat.size):
        want_zen, want_azi, arg = mp_satellite(lat[k], lon[k], *sc)
        assert np.isfinite(zen[k]) and 0 <= azi[k] < 360
        if abs(abs(arg) - 1) > 1e-6:
            worst[2] = max(worst[2], _rad_err(zen[k], want_zen), _rad_err(azi[k], want_azi))
    x, y = scan_grid(6, 7, span=0.12)
    glat, glon = geo.GeosProj(H_GOES, -75.0).inverse_grid(x, y)
    got = run(3, (0.0, -75.0), glat, glon, x, y)[0]
    worst[3] = 0.0
    for i in range(6):
        for j in range(7):
            if np.isfinite(glat[i, j]):
                want, arg = mp_abi_zenith(glat[i, j], glon[i, j], x[j], y[i])
                if abs(abs(arg) - 1) > 1e-6:
                    worst[3] = max(worst[3], _rad_err(got[i, j], want))
            else:
                assert np.isnan(got[i, j])
    return worst


class AbiLike:
    """the smallest `dataset` abi.py reads: .x, .y (scan angles, rad) and .goes_imager_projection with the CF attributes"""

    class _Projection:
        def __init__(self, h, lon_0, sweep):
            self.perspective_point_height = h
            self.longitude_of_projection_origin = lon_0
            self.latitude_of_projection_origin = 0.0
            self.sweep_angle_axis = sweep
            self.semi_major_axis = GRS80[0]
            self.inverse_flattening = GRS80[1]

    def __init__(self, x, y, h=H_GOES, lon_0=-75.0, sweep="x"):
        self.x, self.y = x, y
        self.goes_imager_projection = self._Projection(h, lon_0, sweep)
