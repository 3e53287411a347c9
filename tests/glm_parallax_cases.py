"""Oracles and case builders of the GLM parallax tests (tests/test_glm_parallax_cases_cpu.py, tests/test_gpu_glm_parallax.py).

pyproj is not available, so the yardstick is mathematics in mpmath at 40 digits, as in tests/geodesy_cases.py, and no
oracle restates the code under test:

  geodetic -> ECEF     the closed form (`oracle_to_ecef`)
  fixed grid -> ECEF   the ray from the satellite at a + h with the direction cosines of the two scan angles, intersected
                       with the ellipsoid in the satellite's frame (`oracle_ray`); the code under test is judged by its
                       backward error: the scan angles of the point it returns (`oracle_scan_angles`) and the point's
                       residual in the ellipsoid's equation (`ellipsoid_residual`)
  ECEF -> geodetic     mp.findroot on the latitude equation p tan(lat) - Z = e^2 N(lat) sin(lat) (`oracle_to_geodetic`)
  the chain            steps 1 to 6 of glm.get_glm_parallax_offsets / get_corrected_glm_x_y composed of these
                       (`oracle_chain`); nothing is rounded between the steps

A module-level cache holds every mpmath result: each case is computed once per session.
"""
import functools

import mpmath as mp
import numpy as np

import geodesy_cases as gc

mp.mp.dps = 40

LTG_RE, LTG_RP = 6.394140e6, 6.362755e6                       # lightning_ellipse_rev[0] of the reference's _lmatools.py
LTG_RF = LTG_RE / (LTG_RE - LTG_RP)
LON_0 = -75.0
HEIGHT_TOL = gc.ANGLE_TOL * gc.GRS80[0]                       # metres: 2^-48 of the semi-major axis


def _f(rf):
    return 1 / mp.mpf(rf) if rf else mp.mpf(0)


def _m(v):
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))


def _deg(v):
    return _m(v) * mp.pi / 180


# ---- single steps ----------------------------------------------------------------------------------------------------------
def oracle_to_ecef(lon, lat, alt, a, rf):
    """ECEF metres (mpf) of geodetic degrees and metres on the ellipsoid (a, rf)"""
    f = _f(rf)
    e2 = f * (2 - f)
    phi, lam, alt = _deg(lat), _deg(lon), _m(alt)
    nu = mp.mpf(a) / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    return (nu + alt) * mp.cos(phi) * mp.cos(lam), (nu + alt) * mp.cos(phi) * mp.sin(lam), (nu * (1 - e2) + alt) * mp.sin(phi)


def oracle_to_geodetic(X, Y, Z, a, rf):
    """(lon, lat) in degrees and the height in metres (mpf) of an ECEF point off the polar axis"""
    f = _f(rf)
    e2 = f * (2 - f)
    X, Y, Z = _m(X), _m(Y), _m(Z)
    p = mp.hypot(X, Y)
    nu = lambda phi: mp.mpf(a) / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    phi = mp.findroot(lambda phi: p * mp.sin(phi) - Z * mp.cos(phi) - e2 * nu(phi) * mp.sin(phi) * mp.cos(phi),
                      mp.atan2(Z, p * (1 - e2)))
    if abs(mp.cos(phi)) > mp.mpf("0.5"):
        alt = p / mp.cos(phi) - nu(phi)
    else:
        alt = Z / mp.sin(phi) - nu(phi) * (1 - e2)
    return mp.atan2(Y, X) * 180 / mp.pi, phi * 180 / mp.pi, alt


def _direction(x, y, sweep):
    """direction cosines of the ray with scan angles (x, y) in the satellite's frame: first axis from the Earth's centre
    towards the satellite, second east, third north"""
    x, y = _m(x), _m(y)
    if sweep == "x":
        return -mp.cos(x) * mp.cos(y), mp.sin(x), mp.cos(x) * mp.sin(y)
    return -mp.cos(y) * mp.cos(x), mp.cos(y) * mp.sin(x), mp.sin(y)


def oracle_ray(x, y, h, a, rf, sweep="x"):
    """`(point, disc)`: the nearer intersection, in metres in the satellite's frame, of the ray with scan angles (x, y) from
    the satellite at a + h with the ellipsoid (a, rf), or None where there is none; disc = (B^2 - 4 A C) / B^2"""
    f = _f(rf)
    d = _direction(x, y, sweep)
    s = mp.mpf(a) + mp.mpf(h)
    b = mp.mpf(a) * (1 - f)
    A = (d[0] ** 2 + d[1] ** 2) / mp.mpf(a) ** 2 + d[2] ** 2 / b ** 2
    B = 2 * s * d[0] / mp.mpf(a) ** 2
    C = s ** 2 / mp.mpf(a) ** 2 - 1
    disc = B * B - 4 * A * C
    if disc < 0:
        return None, disc / (B * B)
    t = (-B - mp.sqrt(disc)) / (2 * A)
    return (s + t * d[0], t * d[1], t * d[2]), disc / (B * B)


def _turn(point, lon_deg):
    """the satellite-frame point turned about the polar axis by lon_deg"""
    c, s = mp.cos(_deg(lon_deg)), mp.sin(_deg(lon_deg))
    return point[0] * c - point[1] * s, point[0] * s + point[1] * c, point[2]


def oracle_scan_angles(X, Y, Z, h, lon_0, a, sweep="x"):
    """the scan angles (mpf) under which the satellite at a + h over lon_0 sees the ECEF point"""
    vx, vy, vz = _turn((_m(X), _m(Y), _m(Z)), -_m(lon_0))
    dx = mp.mpf(a) + mp.mpf(h) - vx
    if sweep == "x":
        return mp.atan2(vy, mp.hypot(vz, dx)), mp.atan2(vz, dx)
    return mp.atan2(vy, dx), mp.atan2(vz, mp.hypot(vy, dx))


def ellipsoid_residual(X, Y, Z, a, rf):
    b = mp.mpf(a) * (1 - _f(rf))
    return float((_m(X) ** 2 + _m(Y) ** 2) / mp.mpf(a) ** 2 + _m(Z) ** 2 / b ** 2 - 1)


def oracle_visibility(lat, lon, h=gc.H_GOES, lon_0=LON_0, a=gc.GRS80[0], rf=gc.GRS80[1]):
    """the cosine of the angle between the ellipsoid's outward normal at (lat, lon) and the direction to the satellite:
    negative beyond the limb"""
    X, Y, Z = _turn(oracle_to_ecef(lon, lat, 0.0, a, rf), -_m(lon_0))
    phi, lam = _deg(lat), _deg(lon) - _deg(lon_0)
    n = (mp.cos(phi) * mp.cos(lam), mp.cos(phi) * mp.sin(lam), mp.sin(phi))
    to_sat = (mp.mpf(a) + mp.mpf(h) - X, -Y, -Z)
    return (n[0] * to_sat[0] + n[1] * to_sat[1] + n[2] * to_sat[2]) / mp.sqrt(sum(v * v for v in to_sat))


# ---- the chain -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_chain(lat, lon, lon_0=LON_0, h=gc.H_GOES, sweep="x", grid=gc.GRS80, ltg=(LTG_RE, LTG_RF), lla=gc.GRS80):
    """steps 1 to 6 for the flash at (lat, lon) degrees (floats, taken exactly): a dict of mpf -- dlon, dlat (degrees), x, y
    (the corrected scan angles, +inf where the corrected position is beyond the limb), alt (metres), and vis, disc,
    vis_corrected, the three decisions -- or, beyond the limb or with a ray that misses the lightning ellipsoid, the
    decisions up to there alone"""
    out = {"vis": oracle_visibility(lat, lon, h, lon_0, *grid), "disc": None}
    if out["vis"] < 0:
        return out
    x, y = gc.oracle_forward(lat, lon, h=h, lon_0=lon_0, sweep=sweep, a=grid[0], rf=grid[1])                 # 1
    point, out["disc"] = oracle_ray(x, y, h, ltg[0], ltg[1], sweep)                                           # 2
    if point is None:
        return out
    lon_l, lat_l, out["alt"] = oracle_to_geodetic(*_turn(point, lon_0), *lla)                                # 3
    out["dlon"], out["dlat"] = lon_l - _m(lon), lat_l - _m(lat)                                               # 4
    lon_c, lat_c = _m(lon) - out["dlon"], _m(lat) - out["dlat"]                                               # 5
    out["vis_corrected"] = oracle_visibility(lat_c, lon_c, h, lon_0, *grid)
    if out["vis_corrected"] < 0:                                                                              # 6
        out["x"] = out["y"] = mp.inf
    else:
        out["x"], out["y"] = _forward_mp(lat_c, lon_c, h, lon_0, sweep, *grid)
    return out


def _forward_mp(lat, lon, h, lon_0, sweep, a, rf):
    """geodesy_cases.oracle_forward for mpf arguments (that one takes floats)"""
    X, Y, Z = _turn(oracle_to_ecef(lon, lat, 0, a, rf), -_m(lon_0))
    dx = mp.mpf(a) + mp.mpf(h) - X
    if sweep == "x":
        return mp.atan2(Y, mp.hypot(Z, dx)), mp.atan2(Z, dx)
    return mp.atan2(Y, dx), mp.atan2(Z, mp.hypot(Y, dx))


def _from_nadir(angle, azimuth, lon_0=LON_0):
    """the point at `angle` degrees of arc from the sub-satellite point, `azimuth` degrees from north, on a sphere"""
    g, b = np.radians(angle), np.radians(azimuth)
    lat = np.degrees(np.arcsin(np.sin(g) * np.cos(b)))
    lon = lon_0 + np.degrees(np.arctan2(np.sin(g) * np.sin(b), np.cos(g)))
    return float(lat), float(lon)


NEAR_LIMB = {3: (80.55, 17.0), 17: (80.9, 203.0), 33: (80.45, 95.0), 47: (81.05, -61.0), 58: (80.7, 1.5)}
SUBSATELLITE = 1


@functools.lru_cache(maxsize=None)
def flashes(n=65):
    """`(lat, lon, chain)`: n flashes in float64 degrees and the oracle's result of each.  Most lie over the disk, every
    tenth beyond the limb (geodesy_cases.forward_points), number 1 at the sub-satellite point, and the NEAR_LIMB ones on
    the visible side within 1 degree of arc of the GRS80 limb: one degree further from the sub-satellite point along the
    same azimuth the oracle no longer sees them (asserted).  Whether a near-limb ray misses the lightning ellipsoid is the
    oracle's decision.  No flash lies within 1e-9 of either decision (asserted)."""
    lat, lon = (v.copy() for v in gc.forward_points(n))
    lat[SUBSATELLITE], lon[SUBSATELLITE] = 0.0, LON_0
    for k, (angle, azimuth) in NEAR_LIMB.items():
        if k < n:
            lat[k], lon[k] = _from_nadir(angle, azimuth)
            assert oracle_visibility(lat[k], lon[k]) > 0 > oracle_visibility(*_from_nadir(angle + 1.0, azimuth)), k
    chain = [oracle_chain(float(lat[k]), float(lon[k])) for k in range(n)]
    for k, c in enumerate(chain):
        assert all(abs(c[name]) >= 1e-9 for name in ("vis", "disc", "vis_corrected") if c.get(name) is not None), f"flash {k} sits on a decision"
    return lat, lon, chain


def resolved(chain):
    """bool per flash: on the disk, and its ray meets the lightning ellipsoid"""
    return np.array(["dlon" in c for c in chain])


def chain_errors(chain, dlon, dlat, x, y):
    """the worst |got - oracle| in radians over the resolved flashes: (dlon, dlat, x, y); offsets are degrees"""
    worst = np.zeros(4)
    for k, c in enumerate(chain):
        if "dlon" not in c:
            continue
        if dlon is not None:
            worst[0] = max(worst[0], abs(float((mp.mpf(float(dlon[k])) - c["dlon"]) * mp.pi / 180)))
            worst[1] = max(worst[1], abs(float((mp.mpf(float(dlat[k])) - c["dlat"]) * mp.pi / 180)))
        if x is not None and c["x"] == mp.inf:
            assert np.isposinf(x[k]) and np.isposinf(y[k]), k
        elif x is not None:
            worst[2] = max(worst[2], abs(float(mp.mpf(float(x[k])) - c["x"])))
            worst[3] = max(worst[3], abs(float(mp.mpf(float(y[k])) - c["y"])))
    return worst


# ---- single-step cases -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ecef_points(n=65, seed=8):
    """n ECEF points from the centre of the Earth's crust to 60 km above GRS80, both hemispheres, high latitudes included,
    with the oracle's geodetic coordinates on GRS80: (X, Y, Z) float64 and a list of (lon, lat, alt) mpf"""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-89.9, 89.9, n)
    lon = rng.uniform(-180, 180, n)
    alt = rng.uniform(-5e3, 6e4, n)
    lat[:4] = (89.999, -89.999, 0.0, 1e-7)
    xyz = np.array([[float(v) for v in oracle_to_ecef(lon[k], lat[k], alt[k], *gc.GRS80)] for k in range(n)])
    want = [oracle_to_geodetic(*xyz[k], *gc.GRS80) for k in range(n)]
    return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), want


@functools.lru_cache(maxsize=None)
def scan_points(n=65, sweep="x", seed=9):
    """n scan-angle pairs for the lightning system: most on its disk, every ninth off it, some close to its limb; and the
    oracle's verdict per pair (asserted to lie 1e-9 away from the decision)"""
    rng = np.random.default_rng(seed + (sweep == "y"))
    r = 0.1495 * np.sqrt(rng.uniform(0, 1, n))
    r[::9] = rng.uniform(0.156, 0.2, r[::9].size)
    r[4::13] = rng.uniform(0.1496, 0.1502, r[4::13].size)
    ang = rng.uniform(0, 2 * np.pi, n)
    x, y = r * np.cos(ang), r * np.sin(ang)
    x[1] = y[1] = 0.0
    disc = [oracle_ray(float(x[k]), float(y[k]), gc.H_GOES, LTG_RE, LTG_RF, sweep)[1] for k in range(n)]
    assert min(abs(d) for d in disc) >= 1e-9
    return x, y, np.array([d > 0 for d in disc])


def to_ecef_errors(x, y, hit, X, Y, Z, sweep="x", lon_0=LON_0, h=gc.H_GOES, a=LTG_RE, rf=LTG_RF):
    """over the rays that hit: the worst backward error of the scan angles (radians) and the worst residual in the
    ellipsoid's equation"""
    angle = resid = 0.0
    for k in np.nonzero(hit)[0]:
        ox, oy = oracle_scan_angles(X[k], Y[k], Z[k], h, lon_0, a, sweep)
        angle = max(angle, abs(float(ox - mp.mpf(float(x[k])))), abs(float(oy - mp.mpf(float(y[k])))))
        resid = max(resid, abs(ellipsoid_residual(X[k], Y[k], Z[k], a, rf)))
    return angle, resid


def to_geodetic_errors(want, lon, lat, alt):
    """worst |got - oracle|: (lon, lat) in radians, height in metres"""
    worst = np.zeros(3)
    for k, (olon, olat, oalt) in enumerate(want):
        worst[0] = max(worst[0], abs(float((mp.mpf(float(lon[k])) - olon) * mp.pi / 180)))
        worst[1] = max(worst[1], abs(float((mp.mpf(float(lat[k])) - olat) * mp.pi / 180)))
        worst[2] = max(worst[2], abs(float(mp.mpf(float(alt[k])) - oalt)))
    return worst


# ---- regridding ------------------------------------------------------------------------------------------------------------
PIXEL = 56e-6                                                 # rad: the ABI's 2 km spacing


@functools.lru_cache(maxsize=None)
def regrid_case():
    """A 3 x 7 x 9 grid at the ABI's spacing around (lat 33, lon -97), flashes in float32 like a GLM file's, in three files of
    which the last frame sees none.  Every flash's corrected position by the oracle lies at least 1e-9 rad from every bin
    edge (asserted), so the expected grids do not hang on rounding.  Returns a dict: the grid (`ds`, x, y, x_bins, y_bins,
    goes_dates), the flashes (flash_lat, flash_lon, flash_file, file_times) and the expected (3, 7, 9) int64 grids
    `corrected` and `uncorrected`: np.histogram2d per frame, flipped as glm.py:89 flips it, -1 for the frame without a file."""
    from tobac_flow_amd.utils.xarray_utils import get_coord_bin_edges
    cx, cy = (float(v) for v in gc.oracle_forward(33.0, -97.0))
    x = cx + PIXEL * (np.arange(9) - 4)
    y = cy - PIXEL * (np.arange(7) - 3)
    x_bins, y_bins = get_coord_bin_edges(x), get_coord_bin_edges(y)
    goes_dates = np.array(["2018-06-19T17:00:00", "2018-06-19T17:05:00", "2018-06-19T17:40:00"], dtype="datetime64[us]")
    file_times = np.array(["2018-06-19T17:00:20", "2018-06-19T17:01:40", "2018-06-19T17:04:00"], dtype="datetime64[us]")
    rng = np.random.default_rng(21)
    lat, lon, keep_x, keep_y, raw_x, raw_y = [], [], [], [], [], []
    centre = oracle_chain(33.0, -97.0)                        # the offsets there: 0.06 and -0.08 degrees, three to four pixels
    while len(lat) < 40:
        # spread over a little more than the grid (0.2 x 0.15 degrees) around where the correction puts them back onto it
        la = np.float32(33.0 + float(centre["dlat"]) + rng.uniform(-0.085, 0.085))
        lo = np.float32(-97.0 + float(centre["dlon"]) + rng.uniform(-0.12, 0.12))
        c = oracle_chain(float(la), float(lo))
        px, py = float(c["x"]), float(c["y"])                 # rounded to float64: 1e-17 rad, against the 1e-9 kept from the edges
        if min(np.abs(x_bins - px).min(), np.abs(y_bins - py).min()) < 1e-9:
            continue
        ux, uy = (float(v) for v in gc.oracle_forward(float(la), float(lo)))
        if min(np.abs(x_bins - ux).min(), np.abs(y_bins - uy).min()) < 1e-9:
            continue
        lat.append(la), lon.append(lo), keep_x.append(px), keep_y.append(py), raw_x.append(ux), raw_y.append(uy)
    lat, lon = np.array(lat, np.float32), np.array(lon, np.float32)
    flash_file = (np.arange(lat.size) % 3).astype(np.int64)
    frames = [(0, 1), (2,), ()]                               # the files inside 16:57:30-17:02:30, 17:02:30-17:12:30, 17:32:30-17:47:30

    def grids(px, py):
        out = np.full((3, 7, 9), -1, dtype=np.int64)
        for t, files in enumerate(frames):
            if files:
                pick = np.isin(flash_file, files)
                out[t] = np.histogram2d(np.array(py)[pick], np.array(px)[pick], bins=(y_bins[::-1], x_bins))[0][::-1]
        return out
    corrected, uncorrected = grids(keep_x, keep_y), grids(raw_x, raw_y)
    assert corrected[:2].sum() >= 20 and not np.array_equal(corrected, uncorrected)
    ds = gc.AbiLike(x, y)
    ds.t = goes_dates
    return dict(ds=ds, x=x, y=y, x_bins=x_bins, y_bins=y_bins, goes_dates=goes_dates, flash_lat=lat, flash_lon=lon,
                flash_file=flash_file, file_times=file_times, corrected=corrected, uncorrected=uncorrected)
