"""Geodesy without pyproj: the reference's tobac_flow/geo.py (get_sza, get_sza_and_azi, get_satellite_viewing_angles,
get_pixel_lengths, get_pixel_area) and the two pyproj classes it and its neighbours use, `Geod` (its `.inv`) and `Proj`
with `proj="geos"` (here `GeosProj`); and what the lmatools coordinate systems of tobac_flow/_lmatools.py take from pyproj's
Transformers: `geodetic_to_ecef`, `ecef_to_geodetic`, `GeosProj.to_ecef` / `.from_ecef`, and the chain of them that is the
GLM parallax correction, fused (`glm_parallax`).

NumPy arrays in: the NumPy float64 path, the same algorithm written in NumPy.  Device tensors (or a DeviceField) in: the
HIP kernels of csrc/geodesy.hip, device tensors out, nothing visits the host but the status word of the geodesic inverse.
The two paths run the same operations in the same order; they differ by what the two math libraries differ in, a few ulp
per call.  Formulas, accuracy contract and divergences from PROJ: DESIGN.md, "Geodesy".
"""
import ctypes
import warnings
from datetime import datetime

import numpy as np

ELLIPSOIDS = {"WGS84": (6378137.0, 298.257223563), "GRS80": (6378137.0, 298.257222101)}
MAX_ITER, TOL = 24, 1.4e-15                       # GD_MAX_ITER, GD_TOL of csrc/geodesy_kernels.h
_D2R, _R2D = np.pi / 180.0, 180.0 / np.pi


def _lib():
    from tobac_flow_amd import _lib as lib
    return lib


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def _unwrap(x):
    """a DeviceField's tensor; anything else as it is"""
    data = getattr(x, "data", None)
    return data if data is not None and _is_tensor(data) else x


def _any_tensor(*xs):
    return any(_is_tensor(x) for x in xs)


def _dev_f64(x, shape=None):
    """a float64 contiguous device tensor of x (a tensor, an array or a scalar), broadcast to `shape`"""
    lib = _lib()
    t = lib.torch()
    if not _is_tensor(x):
        x = t.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(lib.device())
    x = x.to(lib.device(), t.float64)
    if shape is not None and tuple(x.shape) != tuple(shape):
        x = x.expand(shape)
    return x.contiguous()


def _ellipsoid(ellps, a, rf):
    if a is not None:
        return float(a), float(0.0 if rf is None else rf)
    if ellps not in ELLIPSOIDS:
        raise ValueError(f"unknown ellipsoid {ellps!r}: one of {sorted(ELLIPSOIDS)}, or a= and rf=")
    return ELLIPSOIDS[ellps]


# ---- geodesic inverse ------------------------------------------------------------------------------------------------------
def _np_geod_inverse(a, f, lon1, lat1, lon2, lat2):
    """gd_geod_inverse_one of csrc/geodesy_kernels.h over arrays: (az12, az21, dist, number of pairs that did not converge)"""
    lon1, lat1, lon2, lat2 = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lon1, lat1, lon2, lat2)))
    shape = lon1.shape
    lon1, lat1, lon2, lat2 = (v.ravel() for v in (lon1, lat1, lon2, lat2))
    n = lon1.size
    az12, az21, dist = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    nan = np.isnan(lon1) | np.isnan(lat1) | np.isnan(lon2) | np.isnan(lat2)
    with np.errstate(all="ignore"):
        b = (1.0 - f) * a
        L = _ieee_remainder(lon2 - lon1, 360.0) * _D2R
        p1, p2 = lat1 * _D2R, lat2 * _D2R
        su1, cu1, su2, cu2 = (1.0 - f) * np.sin(p1), np.cos(p1), (1.0 - f) * np.sin(p2), np.cos(p2)
        n1, n2 = np.hypot(su1, cu1), np.hypot(su2, cu2)
        su1, cu1, su2, cu2 = su1 / n1, cu1 / n1, su2 / n2, cu2 / n2
        lam = L.copy()
        live = ~nan                                            # pairs still iterating
        done = np.zeros(n, bool)
        coincident = np.zeros(n, bool)
        keep = {}
        for _ in range(MAX_ITER):
            if not live.any():
                break
            sl, cl = np.sin(lam), np.cos(lam)
            t1 = cu2 * sl
            t2 = cu1 * su2 - su1 * cu2 * cl
            ss = np.sqrt(t1 * t1 + t2 * t2)
            cs = su1 * su2 + cu1 * cu2 * cl
            zero = live & (ss == 0.0)
            coincident |= zero & (cs > 0.0)
            live = live & ~zero
            sig = np.arctan2(ss, cs)
            sa = cu1 * cu2 * sl / ss
            c2a = 1.0 - sa * sa
            c2m = np.where(c2a != 0.0, cs - 2.0 * su1 * su2 / c2a, 0.0)
            C = f / 16.0 * c2a * (4.0 + f * (4.0 - 3.0 * c2a))
            nxt = L + (1.0 - C) * f * sa * (sig + C * ss * (c2m + C * cs * (-1.0 + 2.0 * c2m * c2m)))
            change = np.abs(nxt - lam)
            beyond = live & ~(np.abs(nxt) <= np.pi)
            live = live & ~beyond
            now = live & (change <= TOL)
            for name, v in (("sl", sl), ("cl", cl), ("t2", t2), ("ss", ss), ("cs", cs), ("sig", sig), ("c2a", c2a), ("c2m", c2m)):
                keep[name] = np.where(now, v, keep.get(name, 0.0))
            done |= now
            live = live & ~now
            lam = np.where(live, nxt, lam)
        if keep:
            sl, cl, t2, ss, cs, sig, c2a, c2m = (keep[k] for k in ("sl", "cl", "t2", "ss", "cs", "sig", "c2a", "c2m"))
            u2 = c2a * (a * a - b * b) / (b * b)
            A = 1.0 + u2 / 16384.0 * (4096.0 + u2 * (-768.0 + u2 * (320.0 - 175.0 * u2)))
            B = u2 / 1024.0 * (256.0 + u2 * (-128.0 + u2 * (74.0 - 47.0 * u2)))
            ds = B * ss * (c2m + B / 4.0 * (cs * (-1.0 + 2.0 * c2m * c2m)
                                            - B / 6.0 * c2m * (-3.0 + 4.0 * ss * ss) * (-3.0 + 4.0 * c2m * c2m)))
            dist = np.where(done, b * A * (sig - ds), dist)
            az12 = np.where(done, np.arctan2(cu2 * sl, t2) * _R2D, az12)
            a2 = np.arctan2(cu1 * sl, -su1 * cu2 + cu1 * su2 * cl) * _R2D
            az21 = np.where(done, np.where(a2 >= 0.0, a2 - 180.0, a2 + 180.0), az21)
        north = lat1 >= 0.0
        dist = np.where(coincident, 0.0, dist)
        az12 = np.where(coincident, np.where(north, 180.0, 0.0), az12)
        az21 = np.where(coincident, np.where(north, 0.0, -180.0), az21)
    failed = int((~nan & ~done & ~coincident).sum())
    return az12.reshape(shape), az21.reshape(shape), dist.reshape(shape), failed


def _dev_geod_inverse(a, rf, lon1, lat1, lon2, lat2):
    lib = _lib()
    t = lib.torch()
    shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in (lon1, lat1, lon2, lat2)))
    lon1, lat1, lon2, lat2 = (_dev_f64(v, shape) for v in (lon1, lat1, lon2, lat2))
    n = lon1.numel()
    out = [lib.empty(shape, t.float64) for _ in range(3)]
    status = lib.empty((1,), t.int32)
    L = lib.lib()
    nbytes = L.tf_geod_inverse_workspace_bytes(n)
    ws = lib.workspace(max(nbytes, 256), "geodesy")
    lib.check(L.tf_geod_inverse(a, rf, lib.ptr(lon1), lib.ptr(lat1), lib.ptr(lon2), lib.ptr(lat2), n, lib.ptr(out[0]),
                                lib.ptr(out[1]), lib.ptr(out[2]), lib.ptr(status), lib.ptr(ws), ws.numel(), lib.stream_ptr()),
              "tf_geod_inverse")
    return out[0], out[1], out[2], int(status.item())


def _warn_failed(failed, what):
    if failed:
        warnings.warn(f"{what}: {failed} pair(s) did not converge within {MAX_ITER} iterations (near the antipode); "
                      "their azimuths and distance are NaN", RuntimeWarning, stacklevel=3)


class Geod:
    """pyproj.Geod as far as the reference uses it: `Geod(ellps="WGS84")` (or "GRS80", or `a=` with `rf=`, the inverse
    flattening; rf 0 or None is a sphere) and `.inv`."""

    def __init__(self, ellps="WGS84", a=None, rf=None):
        self.a, self.rf = _ellipsoid(ellps, a, rf)
        self.f = 1.0 / self.rf if self.rf else 0.0

    def inv(self, lons1, lats1, lons2, lats2):
        """`(az12, az21, dist)` as pyproj's Geod.inv gives them: the forward azimuth at point 1, the back azimuth at point 2
        (the direction from point 2 back to point 1) in degrees within [-180, 180], and the distance in metres.  The inputs
        broadcast; scalars give floats.  NaN in: NaN out.  Coincident points: distance 0 and the azimuths (180, 0) north of
        or on the equator, (0, -180) south of it, which is what GeographicLib (pyproj's engine) returns.  Vincenty's
        iteration: a pair that does not converge within 24 steps -- within about 2 degrees of the antipode -- gives NaN
        in all three and a RuntimeWarning with the count, never a wrong number."""
        lons1, lats1, lons2, lats2 = (_unwrap(v) for v in (lons1, lats1, lons2, lats2))
        if _any_tensor(lons1, lats1, lons2, lats2):
            az12, az21, dist, failed = _dev_geod_inverse(self.a, self.rf, lons1, lats1, lons2, lats2)
        else:
            az12, az21, dist, failed = _np_geod_inverse(self.a, self.f, lons1, lats1, lons2, lats2)
            if az12.ndim == 0:
                az12, az21, dist = float(az12), float(az21), float(dist)
        _warn_failed(failed, "Geod.inv")
        return az12, az21, dist


# ---- geos projection -------------------------------------------------------------------------------------------------------
def _np_geos_ray(p, x, y):
    """gd_geos_ray over arrays: (dy, dz, k, det) of the rays with scan angles (x, y)"""
    ty = np.tan(y)
    if not p.sweep_y:
        vz = ty
        vy = np.tan(x) * np.hypot(1.0, ty)
    else:
        vy = np.tan(x)
        vz = ty * np.hypot(1.0, vy)
    a = vz / p._rp
    a = vy * vy + a * a + 1.0
    b = -2.0 * p._rg
    det = b * b - 4.0 * a * p._c
    return vy, vz, (-b - np.sqrt(det)) / (2.0 * a), det


def _np_geos_inverse(p, x, y):
    """gd_geos_inverse_one over arrays: scan angles (rad) -> (lat, lon) in degrees, NaN off the disk"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        vy, vz, k, det = _np_geos_ray(p, x, y)
        vx = p._rg - k
        vy = vy * k
        vz = vz * k
        lon = np.arctan2(vy, vx) * _R2D + p.lon_0
        lon = np.where(np.abs(lon) > 180.0, _ieee_remainder(lon, 360.0), lon)
        lat = np.arctan(p._rp_inv2 * vz / np.hypot(vx, vy)) * _R2D
        off = ~(det >= 0.0)
        return np.where(off, np.nan, lat), np.where(off, np.nan, lon), off & (det < 0.0)


def _ieee_remainder(v, m):
    """C's remainder(v, m), up to the sign of a result of exactly m / 2"""
    r = np.fmod(v, m)
    return np.where(r > m / 2, r - m, np.where(r < -m / 2, r + m, r))


def _np_geos_surface(p, lat, lon):
    """gd_geos_surface over arrays: the points on the ellipsoid in the satellite's frame, in units of a, and the value of
    PROJ's visibility test"""
    lam = _ieee_remainder(lon - p.lon_0, 360.0) * _D2R
    phi = np.arctan(p._rp2 * np.tan(lat * _D2R))
    cp, sp = np.cos(phi), np.sin(phi)
    r = p._rp / np.hypot(p._rp * cp, sp)
    vx, vy, vz = r * np.cos(lam) * cp, r * np.sin(lam) * cp, r * sp
    return vx, vy, vz, (p._rg - vx) * vx - vy * vy - vz * vz * p._rp_inv2


def _np_geos_forward(p, lat, lon):
    """gd_geos_forward_one over arrays: degrees -> scan angles (rad), +inf beyond the limb"""
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    with np.errstate(all="ignore"):
        vx, vy, vz, vis = _np_geos_surface(p, lat, lon)
        tmp = p._rg - vx
        if not p.sweep_y:
            x, y = np.arctan(vy / np.hypot(vz, tmp)), np.arctan(vz / tmp)
        else:
            x, y = np.arctan(vy / tmp), np.arctan(vz / np.hypot(vy, tmp))
        bad = np.where(vis < 0.0, np.inf, np.nan)
        ok = vis >= 0.0
        return np.where(ok, x, bad), np.where(ok, y, bad)


def _np_geos_forward_alt(p, lat, lon, alt):
    """gd_geos_forward_alt_one over arrays (nexrad.map_nexrad_to_goes)"""
    lat, lon, alt = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lat, lon, alt)))
    x0, y0 = _np_geos_forward(p, lat, lon)
    with np.errstate(all="ignore"):
        dlat = (alt * np.tan((lat - 0.0) * _D2R + y0 / p.h) / 6.371e6) * _R2D
        dlon = (alt * np.tan((lon - p.lon_0) * _D2R + x0 / p.h) / 6.371e6) * _R2D
    return _np_geos_forward(p, lat + dlat, lon + dlon)


# ---- ECEF ------------------------------------------------------------------------------------------------------------------
def _np_geodetic_to_ecef(a, f, lon, lat, alt):
    """gd_geodetic_to_ecef_one over arrays"""
    lon, lat, alt = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lon, lat, alt)))
    with np.errstate(all="ignore"):
        e2 = f * (2.0 - f)
        phi, lam = lat * _D2R, lon * _D2R
        sp, cp = np.sin(phi), np.cos(phi)
        n = a / np.sqrt(1.0 - e2 * sp * sp)
        return (n + alt) * cp * np.cos(lam), (n + alt) * cp * np.sin(lam), (n * (1.0 - e2) + alt) * sp


def _np_ecef_to_geodetic(a, f, X, Y, Z):
    """gd_ecef_to_geodetic_one over arrays: Bowring, two updates -> (lon, lat, alt)"""
    X, Y, Z = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (X, Y, Z)))
    with np.errstate(all="ignore"):
        p = np.hypot(X, Y)
        e2, b = f * (2.0 - f), (1.0 - f) * a
        ep2b, e2a = e2 / (1.0 - e2) * b, e2 * a
        st, ct = Z, (1.0 - f) * p
        for _ in range(2):
            n = np.hypot(st, ct)
            st, ct = st / n, ct / n
            num = Z + ep2b * st * st * st
            den = p - e2a * ct * ct * ct
            st, ct = (1.0 - f) * num, den
        n = np.hypot(num, den)
        sp, cp = num / n, den / n
        lon = np.arctan2(Y, X) * _R2D
        lat = np.arctan2(num, den) * _R2D
        alt = p * cp + Z * sp - a * np.sqrt(1.0 - e2 * sp * sp)
        axis = p == 0.0
        lon = np.where(axis, 0.0, lon)
        lat = np.where(axis, np.where(Z > 0.0, 90.0, -90.0), lat)
        alt = np.where(axis, np.abs(Z) - b, alt)
        bad = ~(np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)) | (axis & (Z == 0.0))
        return np.where(bad, np.nan, lon), np.where(bad, np.nan, lat), np.where(bad, np.nan, alt)


def _np_geos_to_ecef(p, x, y):
    """gd_geos_to_ecef_one over arrays: (X, Y, Z) in metres, +inf where the ray misses the ellipsoid"""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with np.errstate(all="ignore"):
        dy, dz, k, det = _np_geos_ray(p, x, y)
        vx, vy, vz = p._rg - k, dy * k, dz * k
        resid = vx * vx + vy * vy + vz * vz * p._rp_inv2 - 1.0
        slope = 2.0 * (vy * dy + vz * dz * p._rp_inv2 - vx)
        dk = np.where(slope < 0.0, resid / slope, 0.0)
        vx, vy, vz = vx + dk, vy - dk * dy, vz - dk * dz
        l0 = p.lon_0 * _D2R
        c0, s0 = np.cos(l0), np.sin(l0)
        out = p.a * (vx * c0 - vy * s0), p.a * (vx * s0 + vy * c0), p.a * vz
        bad = np.where(det < 0.0, np.inf, np.nan)
        return tuple(np.where(det >= 0.0, v, bad) for v in out)


def _second_ecc2(rf):
    f = 1.0 / rf if rf else 0.0
    e2 = f * (2.0 - f)
    return e2 / (1.0 - e2)


def _np_glm_parallax(grid, ltg, lla_a, lla_rf, lat, lon):
    """gd_glm_parallax_one over arrays: (dlon, dlat, x, y, alt); the constants are gd_parallax_setup's"""
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    shift = (ltg.a - grid.a) + (ltg.h - grid.h)
    shift_rel = shift / grid.a
    ke = (grid.a - ltg.a) * (grid.a + ltg.a) / (ltg.a * ltg.a)
    eg, el = _second_ecc2(grid.rf), _second_ecc2(ltg.rf)
    kp = ke + el + ke * el - eg
    me = 1.0 + ke
    mp = me * (1.0 + el)
    with np.errstate(all="ignore"):
        vx, vy, vz, vis = _np_geos_surface(grid, lat, lon)
        dx, wx = vx - grid._rg, vx + shift_rel
        C = (vx * vx + vy * vy) * ke + vz * vz * kp + (2.0 * vx * shift_rel + shift_rel * shift_rel) * me
        B = 2.0 * ((wx * dx + vy * vy) * me + vz * vz * mp)
        A = (dx * dx + vy * vy) * me + vz * vz * mp
        disc = B * B - 4.0 * A * C
        tau = np.where(C != 0.0, 2.0 * C / (np.sqrt(disc) - B), 0.0)
        qx = (grid.a * vx + shift) + tau * (grid.a * dx)
        qy = grid.a * vy + tau * (grid.a * vy)
        qz = grid.a * vz + tau * (grid.a * vz)
        lon_q, lat_q, alt = _np_ecef_to_geodetic(lla_a, 1.0 / lla_rf if lla_rf else 0.0, qx, qy, qz)
        lon_q = lon_q + grid.lon_0
        lon_q = np.where(np.abs(lon_q) > 180.0, _ieee_remainder(lon_q, 360.0), lon_q)
        hit = (vis >= 0.0) & (disc >= 0.0)
        dlon, dlat = np.where(hit, lon_q - lon, np.nan), np.where(hit, lat_q - lat, np.nan)
        x, y = _np_geos_forward(grid, lat - dlat, lon - dlon)
        bad = np.where((vis < 0.0) | (disc < 0.0), np.inf, np.nan)
        return dlon, dlat, np.where(hit, x, bad), np.where(hit, y, bad), np.where(hit, alt, np.nan)


ECEF_FROM_GEODETIC, ECEF_TO_GEODETIC = 0, 1


def _dev_ecef(mode, a, rf, v0, v1, v2):
    lib = _lib()
    t = lib.torch()
    shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in (v0, v1, v2)))
    v0, v1, v2 = (_dev_f64(v, shape) for v in (v0, v1, v2))
    out = [lib.empty(shape, t.float64) for _ in range(3)]
    lib.check(lib.lib().tf_ecef(mode, a, rf, lib.ptr(v0), lib.ptr(v1), lib.ptr(v2), v0.numel(), lib.ptr(out[0]), lib.ptr(out[1]),
                                lib.ptr(out[2]), lib.stream_ptr()), "tf_ecef")
    return tuple(out)


def geodetic_to_ecef(lon, lat, alt=0.0, ellps="WGS84", a=None, rf=None):
    """`(X, Y, Z)` in metres of geodetic longitude, latitude (degrees) and height (metres) on the ellipsoid: what pyproj's
    latlong -> geocent transform gives.  The inputs broadcast; the argument order is pyproj's."""
    a, rf = _ellipsoid(ellps, a, rf)
    lon, lat, alt = (_unwrap(v) for v in (lon, lat, alt))
    if _any_tensor(lon, lat, alt):
        return _dev_ecef(ECEF_FROM_GEODETIC, a, rf, lon, lat, alt)
    return _np_geodetic_to_ecef(a, 1.0 / rf if rf else 0.0, lon, lat, alt)


def ecef_to_geodetic(X, Y, Z, ellps="WGS84", a=None, rf=None):
    """`(lon, lat, alt)` of ECEF metres on the ellipsoid: pyproj's geocent -> latlong, by Bowring's iteration with two
    updates (within 1e-16 rad up to 160 km above the ellipsoid).  On the polar axis lon = 0 and lat = +-90; the origin,
    NaN and infinite coordinates give NaN."""
    a, rf = _ellipsoid(ellps, a, rf)
    X, Y, Z = (_unwrap(v) for v in (X, Y, Z))
    if _any_tensor(X, Y, Z):
        return _dev_ecef(ECEF_TO_GEODETIC, a, rf, X, Y, Z)
    return _np_ecef_to_geodetic(a, 1.0 / rf if rf else 0.0, X, Y, Z)


def glm_parallax(grid, ltg, lla, lat, lon, offsets=True, scan_angles=True):
    """The GLM parallax correction for flashes at (lat, lon) degrees: `(dlon, dlat, x, y)` -- the offsets of
    glm.get_glm_parallax_offsets and the scan angles of the corrected positions on `grid`; a pair that is not asked for is
    None.  grid: the GeosProj of the ABI file; ltg: the GeosProj of the lightning ellipsoid (same lon_0 and sweep);
    lla: (a, rf) of the ellipsoid the lightning point is read on.  float32 or float64 in (float32 is widened exactly),
    float64 out; device tensors in: one launch of tf_glm_parallax.  A flash beyond the limb, or whose ray misses the
    lightning ellipsoid: NaN offsets, +inf scan angles."""
    lat, lon = _unwrap(lat), _unwrap(lon)
    if ltg.lon_0 != grid.lon_0 or ltg.sweep_y != grid.sweep_y:
        raise ValueError("the lightning system shares lon_0 and the sweep axis with the grid's")
    if _any_tensor(lat, lon):
        lib = _lib()
        t = lib.torch()
        lat, lon = (v if _is_tensor(v) else t.from_numpy(np.ascontiguousarray(v)) for v in (lat, lon))
        shape = t.broadcast_shapes(tuple(lat.shape), tuple(lon.shape))
        dtype = t.float32 if lat.dtype == lon.dtype == t.float32 else t.float64
        lat, lon = (v.to(lib.device(), dtype).expand(shape).contiguous() for v in (lat, lon))
        out = [lib.empty(shape, t.float64) if want else None for want in (offsets, offsets, scan_angles, scan_angles)]
        g, l = grid._params(), ltg._params()
        lib.check(lib.lib().tf_glm_parallax(ctypes.byref(g), ctypes.byref(l), lla[0], lla[1], lib.ptr(lat), lib.ptr(lon),
                                            lib.TF_F32 if dtype == t.float32 else lib.TF_F64, lat.numel(), lib.ptr(out[0]),
                                            lib.ptr(out[1]), lib.ptr(out[2]), lib.ptr(out[3]), lib.stream_ptr()), "tf_glm_parallax")
        return tuple(out)
    dlon, dlat, x, y, _ = _np_glm_parallax(grid, ltg, lla[0], lla[1], lat, lon)
    return (dlon if offsets else None, dlat if offsets else None, x if scan_angles else None, y if scan_angles else None)


class GeosProj:
    """pyproj.Proj(proj="geos", h=, lon_0=, lat_0=, sweep=) as far as the reference uses it.  `p(x, y, inverse=True)`
    takes projection coordinates in metres (scan angle times h) and returns `(lon, lat)` in degrees, +inf off the disk;
    `p(lon, lat)` returns `(x, y)` in metres, +inf beyond the limb.  The ellipsoid is PROJ's default, GRS80 (also the
    GOES-R value), unless `ellps=` or `a=`, `rf=` say otherwise.  lat_0 must be 0, as in PROJ."""

    def __init__(self, h, lon_0=0.0, lat_0=0.0, sweep="x", ellps="GRS80", a=None, rf=None):
        if float(lat_0) != 0.0:
            raise ValueError("the geos projection takes lat_0 = 0 only (PROJ refuses any other value)")
        if sweep not in ("x", "y"):
            raise ValueError("sweep is 'x' (GOES) or 'y' (Meteosat)")
        self.h, self.lon_0, self.lat_0, self.sweep = float(h), float(lon_0), 0.0, sweep
        if not (self.h > 0 and np.isfinite(self.lon_0)):
            raise ValueError("h is positive and lon_0 finite")
        self.a, self.rf = _ellipsoid(ellps, a, rf)
        self.sweep_y = int(sweep == "y")
        f = 1.0 / self.rf if self.rf else 0.0
        one_es = (1.0 - f) * (1.0 - f)
        self._rg = 1.0 + self.h / self.a
        self._c = self._rg * self._rg - 1.0
        self._rp, self._rp2, self._rp_inv2 = 1.0 - f, one_es, 1.0 / one_es

    def _params(self, inf=False):
        lib = _lib()
        return lib.Geos(self.h, self.lon_0, 0.0, self.a, self.rf, self.sweep_y, lib.GEOS_INF if inf else 0)

    # -- scan-angle forms (radians): what abi.py works with --
    def inverse_grid(self, x, y, dtype=float, inf=False):
        """1-D scan angles x (W) and y (H) -> `(lat, lon)` on the (H, W) grid in `dtype` (float64 or float32: the float64
        result rounded once), NaN off the disk (or +inf with inf=True)"""
        x, y = _unwrap(x), _unwrap(y)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("lat and lon are float64 or float32")
        if _any_tensor(x, y):
            lib = _lib()
            t = lib.torch()
            x, y = _dev_f64(x).reshape(-1), _dev_f64(y).reshape(-1)
            tdtype = t.float64 if dtype == np.float64 else t.float32
            lat, lon = lib.empty((y.numel(), x.numel()), tdtype), lib.empty((y.numel(), x.numel()), tdtype)
            geos = self._params(inf)
            lib.check(lib.lib().tf_geos_inverse(ctypes.byref(geos), lib.ptr(x), x.numel(), lib.ptr(y), y.numel(), lib.ptr(lat),
                                                lib.ptr(lon), lib.TF_F64 if dtype == np.float64 else lib.TF_F32,
                                                lib.stream_ptr()), "tf_geos_inverse")
            return lat, lon
        xx, yy = np.meshgrid(np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1))
        lat, lon, off = _np_geos_inverse(self, xx, yy)
        if inf:
            lat, lon = np.where(off, np.inf, lat), np.where(off, np.inf, lon)
        return lat.astype(dtype), lon.astype(dtype)

    def inverse_points(self, x, y, inf=False):
        """scan angles of N points (any common shape) -> `(lat, lon)`, float64"""
        x, y = _unwrap(x), _unwrap(y)
        if _any_tensor(x, y):
            lib = _lib()
            t = lib.torch()
            shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in (x, y)))
            x, y = _dev_f64(x, shape), _dev_f64(y, shape)
            lat, lon = lib.empty(shape, t.float64), lib.empty(shape, t.float64)
            geos = self._params(inf)
            lib.check(lib.lib().tf_geos_inverse_points(ctypes.byref(geos), lib.ptr(x), lib.ptr(y), x.numel(), lib.ptr(lat),
                                                       lib.ptr(lon), lib.stream_ptr()), "tf_geos_inverse_points")
            return lat, lon
        x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        lat, lon, off = _np_geos_inverse(self, x, y)
        if inf:
            lat, lon = np.where(off, np.inf, lat), np.where(off, np.inf, lon)
        return lat, lon

    def forward_points(self, lat, lon, alt=None):
        """(lat, lon) in degrees of N points -> scan angles `(x, y)` in radians, +inf beyond the limb; with `alt` (metres)
        the parallax-corrected position of nexrad.map_nexrad_to_goes"""
        lat, lon, alt = _unwrap(lat), _unwrap(lon), _unwrap(alt)
        if _any_tensor(lat, lon, alt):
            lib = _lib()
            t = lib.torch()
            given = [v for v in (lat, lon, alt) if v is not None]
            shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in given))
            lat, lon = _dev_f64(lat, shape), _dev_f64(lon, shape)
            alt = None if alt is None else _dev_f64(alt, shape)
            x, y = lib.empty(shape, t.float64), lib.empty(shape, t.float64)
            geos = self._params()
            lib.check(lib.lib().tf_geos_forward(ctypes.byref(geos), lib.ptr(lat), lib.ptr(lon), lib.ptr(alt), lat.numel(),
                                                lib.ptr(x), lib.ptr(y), lib.stream_ptr()), "tf_geos_forward")
            return x, y
        if alt is None:
            return _np_geos_forward(self, lat, lon)
        return _np_geos_forward_alt(self, lat, lon, alt)

    def to_ecef(self, x, y):
        """scan angles (radians) -> ECEF `(X, Y, Z)` in metres of the nearer point at which the ray meets this projection's
        ellipsoid, +inf in all three where it misses: Transformer.from_crs(geos, geocent) at height 0"""
        x, y = _unwrap(x), _unwrap(y)
        if _any_tensor(x, y):
            lib = _lib()
            t = lib.torch()
            shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in (x, y)))
            x, y = _dev_f64(x, shape), _dev_f64(y, shape)
            out = [lib.empty(shape, t.float64) for _ in range(3)]
            geos = self._params()
            lib.check(lib.lib().tf_geos_to_ecef(ctypes.byref(geos), lib.ptr(x), lib.ptr(y), x.numel(), lib.ptr(out[0]),
                                                lib.ptr(out[1]), lib.ptr(out[2]), lib.stream_ptr()), "tf_geos_to_ecef")
            return tuple(out)
        return _np_geos_to_ecef(self, x, y)

    def from_ecef(self, X, Y, Z):
        """ECEF metres -> `(x, y, alt)`: the scan angles (radians) of the geodetic position on this projection's ellipsoid,
        +inf beyond the limb, and the height above it in metres"""
        lon, lat, alt = ecef_to_geodetic(X, Y, Z, a=self.a, rf=self.rf)
        x, y = self.forward_points(lat, lon)
        return x, y, alt

    def __call__(self, x, y, inverse=False):
        x, y = _unwrap(x), _unwrap(y)
        scalar = not _any_tensor(x, y) and np.ndim(x) == 0 and np.ndim(y) == 0
        if inverse:
            lat, lon = self.inverse_points(x / self.h, y / self.h, inf=True)
            out = lon, lat
        else:
            sx, sy = self.forward_points(y, x)
            out = sx * self.h, sy * self.h
        return tuple(float(v) for v in out) if scalar else out


# ---- pixel lengths and area ------------------------------------------------------------------------------------------------
def _spacing_rule(raw, axis):
    """the reference's edge rule (geo.py:230-236) along `axis` of the raw spacings (zero in the last position)"""
    d = np.moveaxis(raw.copy(), axis, 0)
    d[1:] = d[1:] + np.moveaxis(raw, axis, 0)[:-1]
    d[1:-1] = d[1:-1] / 2
    return np.moveaxis(d, 0, axis)


def _np_raw_spacings(geod, lat, lon):
    raw_y, raw_x = np.zeros(lat.shape), np.zeros(lat.shape)
    dy, fy = _np_geod_inverse(geod.a, geod.f, lon[:-1], lat[:-1], lon[1:], lat[1:])[2:]
    dx, fx = _np_geod_inverse(geod.a, geod.f, lon[:, :-1], lat[:, :-1], lon[:, 1:], lat[:, 1:])[2:]
    raw_y[:-1] = dy / 1e3
    raw_x[:, :-1] = dx / 1e3
    return raw_y, raw_x, fy + fx


def grid_spacing(lat, lon, want=("dx", "dy"), geod=None):
    """`dx`, `dy` (km) and / or `area` (km2) of a 2-D lat / lon grid, in the order of `want`: the routine the reference
    keeps three copies of (geo.py:224-246, abi.py:42-65, utils/geo_utils.py:9-34)"""
    geod = geod or Geod(ellps="WGS84")
    lat, lon = _unwrap(lat), _unwrap(lon)
    if _any_tensor(lat, lon):
        lib = _lib()
        t = lib.torch()
        lat, lon = _dev_f64(lat), _dev_f64(lon)
        if lat.dim() != 2 or lat.shape != lon.shape:
            raise ValueError("lat and lon are 2-D arrays of one shape")
        H, W = (int(v) for v in lat.shape)
        out = {name: lib.empty((H, W), t.float64) for name in want}
        status = lib.empty((1,), t.int32)
        L = lib.lib()
        ws = lib.workspace(max(L.tf_grid_spacing_workspace_bytes(H, W), 256), "geodesy")
        lib.check(L.tf_grid_spacing(geod.a, geod.rf, lib.ptr(lat), lib.ptr(lon), H, W, lib.ptr(out.get("dx")), lib.ptr(out.get("dy")),
                                    lib.ptr(out.get("area")), lib.ptr(status), lib.ptr(ws), ws.numel(), lib.stream_ptr()),
                  "tf_grid_spacing")
        _warn_failed(int(status.item()), "grid_spacing")
        return tuple(out[name] for name in want)
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    if lat.ndim != 2 or lat.shape != lon.shape:
        raise ValueError("lat and lon are 2-D arrays of one shape")
    raw_y, raw_x, failed = _np_raw_spacings(geod, lat, lon)
    _warn_failed(failed, "grid_spacing")
    out = {"dy": _spacing_rule(raw_y, 0), "dx": _spacing_rule(raw_x, 1)}
    out["area"] = out["dx"] * out["dy"]
    return tuple(out[name] for name in want)


def get_pixel_lengths(lat, lon):
    """`(dx, dy)`: the length scales in x and y of each pixel in km (reference: geo.py:224-237)"""
    return grid_spacing(lat, lon, ("dx", "dy"))


def get_pixel_area(lat, lon):
    """the area of each pixel in square km (reference: geo.py:240-246)"""
    return grid_spacing(lat, lon, ("area",))[0]


# ---- viewing angles --------------------------------------------------------------------------------------------------------
def _np_view_angles(mode, sc, lat, lon, sx=None, sy=None):
    """gd_view_angles_one over arrays"""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mode in (0, 1):
            delta, eqt, hour = sc
            omega = ((360.0 / 24.0) * (hour + lon / 15.0 + eqt - 12.0)) * _D2R
            rl = lat * _D2R
            sunh = np.sin(delta) * np.sin(rl) + np.cos(delta) * np.cos(rl) * np.cos(omega)
            if mode == 0:
                return np.pi / 2.0 - np.arcsin(sunh), None
            sza = np.pi / 2.0 - np.arcsin(np.clip(sunh, -1, 1))
            azimuth = (np.sin(delta) * np.cos(rl) - np.cos(delta) * np.sin(rl) * np.cos(omega)) / np.cos(np.pi / 2.0 - sza)
            return sza * _R2D, np.arccos(np.clip(azimuth, -1, 1)) * _R2D
        if mode == 2:
            re, rgeo = 6371.0, sc[2] + 6371.0
            dlat, dlon = (lat - sc[0]) * _D2R, (lon - sc[1]) * _D2R
            cos_beta = np.cos(dlat) * np.cos(dlon)
            sin_beta = np.sin(np.arccos(cos_beta))
            dist = np.sqrt(rgeo * rgeo + re * re - 2.0 * rgeo * re * cos_beta)
            zen = np.arcsin(rgeo * sin_beta / dist) * _R2D
            zen = np.where(dist * dist < rgeo * rgeo - re * re, zen, 180.0 - zen)
            xs, ys = np.cos(dlat) * np.sin(dlon), np.sin(dlat)
            return zen, np.where(np.isfinite(xs), np.remainder(np.arctan2(xs, ys) * _R2D, 360.0), np.nan)
        dlat, dlon = (lat - sc[0]) * _D2R, (lon - sc[1]) * _D2R
        xx, yy = -np.asarray(sx, dtype=np.float64), -np.asarray(sy, dtype=np.float64)
        dot = (np.cos(dlon) * np.sin(dlat) * (np.cos(xx) * np.sin(yy)) + (-np.sin(dlon)) * (-np.sin(xx))
               + np.cos(dlon) * np.cos(dlat) * (np.cos(xx) * np.cos(yy)))
        return np.arccos(dot) * _R2D, None


def view_angles(mode, scalars, lat, lon, x=None, y=None):
    """the four elementwise angle functions behind one dispatch: NumPy in, NumPy out; tensors in, tf_view_angles.  For
    mode 3 (the ABI zenith angle) lat and lon are (H, W) and x (W), y (H) the grid's scan angles."""
    lat, lon, x, y = (_unwrap(v) for v in (lat, lon, x, y))
    scalars = [float(v) for v in scalars]
    if _any_tensor(lat, lon, x, y):
        lib = _lib()
        t = lib.torch()
        shape = t.broadcast_shapes(*(tuple(v.shape) if hasattr(v, "shape") else () for v in (lat, lon)))
        lat, lon = _dev_f64(lat, shape), _dev_f64(lon, shape)
        W = 1
        if mode == 3:
            x, y = _dev_f64(x).reshape(-1), _dev_f64(y).reshape(-1)
            if tuple(shape) != (y.numel(), x.numel()):
                raise ValueError("lat and lon are (len(y), len(x))")
            W = x.numel()
        out0 = lib.empty(shape, t.float64)
        out1 = lib.empty(shape, t.float64) if mode in (1, 2) else None
        sc = (ctypes.c_double * len(scalars))(*scalars)
        lib.check(lib.lib().tf_view_angles(mode, sc, len(scalars), lib.ptr(lat), lib.ptr(lon), lat.numel(), lib.ptr(x) if mode == 3 else None,
                                           lib.ptr(y) if mode == 3 else None, W, lib.ptr(out0), lib.ptr(out1), lib.stream_ptr()),
                  "tf_view_angles")
        return out0, out1
    if mode == 3:
        x, y = np.meshgrid(np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1))
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64))
    return _np_view_angles(mode, scalars, lat, lon, x, y)


def _declination(eta):
    return (0.006918 - 0.399912 * np.cos(eta) - 0.006758 * np.cos(2.0 * eta) - 0.002697 * np.cos(3.0 * eta)
            + 0.070257 * np.sin(eta) + 0.000907 * np.sin(2.0 * eta) + 0.001480 * np.sin(3.0 * eta))


def _equation_of_time(et):
    return (0.0072 * np.cos(et) - 0.0528 * np.cos(2.0 * et) - 0.0012 * np.cos(3.0 * et) - 0.1229 * np.sin(et)
            - 0.1565 * np.sin(2.0 * et) - 0.0041 * np.sin(3.0 * et))


def _scalar_out(v, *inputs):
    return float(v) if not _is_tensor(v) and all(np.ndim(_unwrap(i)) == 0 for i in inputs) else v


def sza_scalars(dt):
    """the per-date scalars of get_sza (geo.py:18-70): (delta, eqt, time in hours), host Python as in the reference"""
    srd = (dt - datetime(dt.year, 1, 1)).days + 1
    utc = srd + dt.hour / 24.0 + float(dt.minute / (24.0 * 60.0))
    daynum = np.floor(utc) + 1
    delta = _declination(2.0 * np.pi * daynum / 365.0)
    eqt = _equation_of_time(2.0 * np.pi * daynum / 366.0)
    return float(delta), float(eqt), float((utc + 1.0 - daynum) * 24)


def get_sza(dt, lat, lon):
    """the solar zenith angle in radians at a time / lat / lon (reference: geo.py:14-95)"""
    return _scalar_out(view_angles(0, sza_scalars(dt), lat, lon)[0], lat, lon)


def get_sza_and_azi(date, lat, lon):
    """`(zenith, azimuth)` of the sun in degrees (reference: geo.py:98-164)"""
    day_of_year = int(date.strftime("%j"))
    hour_of_day = (date - datetime(date.year, date.month, date.day, 0, 0, 0)).total_seconds() / 3600
    declination = _declination(2.0 * np.pi * day_of_year / 365.0)
    eqt = _equation_of_time(2.0 * np.pi * day_of_year / 366.0)
    zen, azi = view_angles(1, (declination, eqt, hour_of_day), lat, lon)
    return _scalar_out(zen, lat, lon), _scalar_out(azi, lat, lon)


def get_satellite_viewing_angles(lat, lon, sat_lat=0, sat_lon=0, sat_alt=35_793):
    """`(zenith, azimuth)` of the satellite in degrees seen from the surface point (reference: geo.py:167-221); sat_alt in
    km above a 6371 km sphere"""
    zen, azi = view_angles(2, (sat_lat, sat_lon, sat_alt), lat, lon)
    return _scalar_out(zen, lat, lon), _scalar_out(azi, lat, lon)
