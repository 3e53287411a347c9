// Per-element arithmetic of geodesy.hip (tf_geos_inverse, tf_geos_forward, tf_geod_inverse, tf_grid_spacing,
// tf_view_angles, tf_ecef, tf_geos_to_ecef, tf_glm_parallax).  Kept apart from the entry points so that the same text compiles for the host:
// tools/geodesy_check/geodesy_check.cpp includes it with plain g++ and prints what it computes for the cases of
// tests/geodesy_cases.py and tests/glm_parallax_cases.py.  Everything is float64; nothing here touches the HIP runtime.  -ffp-contract=off: every
// expression rounds as written.  The formulas and their divergences from PROJ are in DESIGN.md ("Geodesy").
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/tobac_flow_hip.h"

#define GD_PI 3.14159265358979323846
#define GD_D2R (GD_PI / 180.0)                                    // np.radians / np.deg2rad multiply by this constant
#define GD_R2D (180.0 / GD_PI)                                    // np.degrees / np.rad2deg by this one
// Vincenty's iteration contracts |d lambda| by a ratio r per step.  A pair that needs more than GD_MAX_ITER steps to
// bring a change of at most pi below GD_TOL has r > 0.2; a pair that gets there has r <= 0.2 on average, so what is
// left after the last step is below GD_TOL r / (1 - r) < 4e-16 rad (2.5 nm on the ground).  The cap is therefore the
// error bound as well as the trip limit: slow pairs (all of them near the antipode) end as NaN, never as a wrong number.
#define GD_MAX_ITER 24
#define GD_TOL 1.4e-15                                            // 3 ulp of pi

struct GdGeos {                                                   // the constants of PROJ's geos set-up, in units of a
    double rg, c, rp, rp2, rp_inv2;                               // 1 + h / a, rg^2 - 1, sqrt(1 - es), 1 - es, 1 / (1 - es)
    double lon_0, h, a;
    int sweep_y, inf_off_disk;
};

__host__ __device__ inline GdGeos gd_geos_setup(const TfGeos &g)
{
    GdGeos s;
    const double f = g.rf != 0 ? 1.0 / g.rf : 0.0;
    const double one_es = (1.0 - f) * (1.0 - f);
    s.rg = 1.0 + g.h / g.a;
    s.c = s.rg * s.rg - 1.0;
    s.rp = 1.0 - f;
    s.rp2 = one_es;
    s.rp_inv2 = 1.0 / one_es;
    s.lon_0 = g.lon_0;
    s.h = g.h;
    s.a = g.a;
    s.sweep_y = g.sweep_y;
    s.inf_off_disk = (g.flags & TF_GEOS_INF) != 0;
    return s;
}

// the longitude PROJ hands back: within [-180, 180]
__host__ __device__ inline double gd_wrap180(double lon) { return fabs(lon) > 180.0 ? remainder(lon, 360.0) : lon; }

// ---- geos inverse --------------------------------------------------------------------------------------------------------
// The terms of one scan line that do not depend on the other coordinate: sweep x (GOES) scans rows, vz = tan y and
// hz = hypot(1, vz) belong to the row; sweep y (Meteosat) the other way round, vy = tan x belongs to the column.
__host__ __device__ inline void gd_geos_row_terms(const GdGeos &s, double y, double &ty, double &hy)
{
    ty = tan(y);
    hy = s.sweep_y ? 0.0 : hypot(1.0, ty);
}

// PROJ's e_inverse up to the intersection: the ray with scan angles (x, y) is S + k (-1, dy, dz) from the satellite
// S = (rg, 0, 0), in units of a, in the frame whose first axis points from the Earth's centre to the satellite, the second
// east and the third north.  Returns the discriminant of the intersection with the ellipsoid; where it is not negative, k
// belongs to the nearer of the two points.
__host__ __device__ inline double gd_geos_ray(const GdGeos &s, double x, double ty, double hy, double &dy, double &dz, double &k)
{
    if (!s.sweep_y) { dz = ty; dy = tan(x) * hy; }
    else { dy = tan(x); dz = ty * hypot(1.0, dy); }
    double a = dz / s.rp;
    a = dy * dy + a * a + 1.0;
    const double b = -2.0 * s.rg;
    const double det = b * b - 4.0 * a * s.c;
    k = (-b - sqrt(det)) / (2.0 * a);
    return det;
}

// (lat, lon) in degrees of the ray with scan angles (x, y); ty, hy from gd_geos_row_terms(y).  The latitude is taken as
// atan(Vz / ((1 - es) hypot(Vx, Vy))), which is PROJ's atan(tan(atan(Vz cos(lam) / Vx)) / (1 - es)) with
// cos(lam) = Vx / hypot(Vx, Vy) and without its three extra roundings.
__host__ __device__ inline bool gd_geos_inverse_one(const GdGeos &s, double x, double ty, double hy, double &lat, double &lon)
{
    double vy, vz, k;
    const double det = gd_geos_ray(s, x, ty, hy, vy, vz, k);
    if (!(det >= 0.0)) {                                          // off the disk (or a NaN angle)
        lat = lon = (s.inf_off_disk && det < 0.0) ? HUGE_VAL : NAN;
        return false;
    }
    const double vx = s.rg - k;
    vy *= k;
    vz *= k;
    lon = gd_wrap180(atan2(vy, vx) * GD_R2D + s.lon_0);
    lat = atan(s.rp_inv2 * vz / hypot(vx, vy)) * GD_R2D;
    return true;
}

// ---- geos forward --------------------------------------------------------------------------------------------------------
// PROJ's e_forward up to its visibility test: the point (lat, lon) in degrees on the ellipsoid as (vx, vy, vz) in units of
// a, in the frame of gd_geos_ray.  Returns the test's value: negative beyond the limb.
__host__ __device__ inline double gd_geos_surface(const GdGeos &s, double lat, double lon, double &vx, double &vy, double &vz)
{
    const double lam = remainder(lon - s.lon_0, 360.0) * GD_D2R;
    const double phi = atan(s.rp2 * tan(lat * GD_D2R));
    const double cp = cos(phi), sp = sin(phi);
    const double r = s.rp / hypot(s.rp * cp, sp);
    vx = r * cos(lam) * cp;
    vy = r * sin(lam) * cp;
    vz = r * sp;
    return (s.rg - vx) * vx - vy * vy - vz * vz * s.rp_inv2;
}

// scan angles (x, y) in radians of the point (lat, lon) in degrees: PROJ's e_forward; beyond the limb (its visibility
// test) both are +inf.
__host__ __device__ inline void gd_geos_forward_one(const GdGeos &s, double lat, double lon, double &x, double &y)
{
    double vx, vy, vz;
    const double vis = gd_geos_surface(s, lat, lon, vx, vy, vz);
    const double tmp = s.rg - vx;
    if (!(vis >= 0.0)) {
        x = y = vis < 0.0 ? HUGE_VAL : NAN;
        return;
    }
    if (!s.sweep_y) { x = atan(vy / hypot(vz, tmp)); y = atan(vz / tmp); }
    else { x = atan(vy / tmp); y = atan(vz / hypot(vy, tmp)); }
}

// nexrad.map_nexrad_to_goes (reference nexrad.py:60-77): project, shift by the parallax of a target `alt` metres up,
// project again.  The reference divides the scan angle by the height once more and uses a 6.371e6 m sphere: kept.
__host__ __device__ inline void gd_geos_forward_alt_one(const GdGeos &s, double lat, double lon, double alt, double &x, double &y)
{
    double x0, y0;
    gd_geos_forward_one(s, lat, lon, x0, y0);
    const double dlat = (alt * tan((lat - 0.0) * GD_D2R + y0 / s.h) / 6.371e6) * GD_R2D;
    const double dlon = (alt * tan((lon - s.lon_0) * GD_D2R + x0 / s.h) / 6.371e6) * GD_R2D;
    gd_geos_forward_one(s, lat + dlat, lon + dlon, x, y);
}

// ---- ECEF ----------------------------------------------------------------------------------------------------------------
// pyproj's latlong <-> geocent on the ellipsoid (a, f): degrees and metres, X towards (lat 0, lon 0), Z towards the north pole.
__host__ __device__ inline void gd_geodetic_to_ecef_one(double a, double f, double lon, double lat, double alt, double &X, double &Y,
                                                        double &Z)
{
    const double e2 = f * (2.0 - f);
    const double phi = lat * GD_D2R, lam = lon * GD_D2R;
    const double sp = sin(phi), cp = cos(phi);
    const double n = a / sqrt(1.0 - e2 * sp * sp);
    X = (n + alt) * cp * cos(lam);
    Y = (n + alt) * cp * sin(lam);
    Z = (n * (1.0 - e2) + alt) * sp;
}

// Bowring's iteration on the parametric latitude, kept as a (sine, cosine) pair so that no angle is formed before the
// last line: two updates, no test.  One update leaves up to 1.9e-13 rad of latitude at the 6 to 16 km of the lightning
// ellipsoid, two leave less than 1e-16 rad up to ten times that height.  On the polar axis lon = 0 and lat = +-90; the
// origin, a NaN and an infinite coordinate give NaN in all three.  The height is p cos(lat) + Z sin(lat) - a sqrt(1 - e2
// sin^2(lat)), which has no pole and is stationary in lat.
__host__ __device__ inline void gd_ecef_to_geodetic_one(double a, double f, double X, double Y, double Z, double &lon, double &lat,
                                                        double &alt)
{
    const double p = hypot(X, Y);
    if (!(X - X == 0.0) || !(Y - Y == 0.0) || !(Z - Z == 0.0) || (p == 0.0 && Z == 0.0)) {
        lon = lat = alt = NAN;
        return;
    }
    const double e2 = f * (2.0 - f), b = (1.0 - f) * a;
    if (p == 0.0) {
        lon = 0.0;
        lat = Z > 0.0 ? 90.0 : -90.0;
        alt = fabs(Z) - b;
        return;
    }
    const double ep2b = e2 / (1.0 - e2) * b, e2a = e2 * a;
    double st = Z, ct = (1.0 - f) * p, num = 0.0, den = 0.0;
    for (int update = 0; update < 2; update++) {
        const double n = hypot(st, ct);
        st /= n;
        ct /= n;
        num = Z + ep2b * st * st * st;
        den = p - e2a * ct * ct * ct;
        st = (1.0 - f) * num;
        ct = den;
    }
    const double n = hypot(num, den), sp = num / n, cp = den / n;
    lon = atan2(Y, X) * GD_R2D;
    lat = atan2(num, den) * GD_R2D;
    alt = p * cp + Z * sp - a * sqrt(1.0 - e2 * sp * sp);
}

// Fixed grid -> ECEF: the nearer point at which the ray with scan angles (x, y) meets the system's ellipsoid, turned from
// the satellite's frame into the Earth's by lon_0, in metres.  The root of the quadratic carries the rounding of its
// discriminant, a few 1e-15 along the ray; one Newton step on the ellipsoid's equation at the point itself, where its terms
// sum to 1 and not to rg^2, takes that out without moving the point off the ray.  False, and +inf in all three, where the
// ray misses (NaN for a NaN angle).
__host__ __device__ inline bool gd_geos_to_ecef_one(const GdGeos &s, double x, double y, double &X, double &Y, double &Z)
{
    double ty, hy, dy, dz, k;
    gd_geos_row_terms(s, y, ty, hy);
    const double det = gd_geos_ray(s, x, ty, hy, dy, dz, k);
    if (!(det >= 0.0)) {
        X = Y = Z = det < 0.0 ? HUGE_VAL : NAN;
        return false;
    }
    double vx = s.rg - k, vy = dy * k, vz = dz * k;
    const double resid = vx * vx + vy * vy + vz * vz * s.rp_inv2 - 1.0;
    const double slope = 2.0 * (vy * dy + vz * dz * s.rp_inv2 - vx);
    if (slope < 0.0) {
        const double dk = resid / slope;
        vx += dk;
        vy -= dk * dy;
        vz -= dk * dz;
    }
    const double l0 = s.lon_0 * GD_D2R, c0 = cos(l0), s0 = sin(l0);
    X = s.a * (vx * c0 - vy * s0);
    Y = s.a * (vx * s0 + vy * c0);
    Z = s.a * vz;
    return true;
}

// ---- GLM parallax --------------------------------------------------------------------------------------------------------
// glm.get_glm_parallax_offsets and get_corrected_glm_x_y (reference glm.py:25-57) for one flash: (1) the flash's point P on
// the grid's ellipsoid and the ray from the grid's satellite to it, (2) the nearer point Q at which the ray WITH THE SAME
// SCAN ANGLES from the lightning system's satellite meets the lightning ellipsoid, (3) Q's geodetic longitude and latitude
// on the third ellipsoid, (4) the offsets, (5) the flash moved back by them, (6) projected again.
//
// The two rays are parallel, a distance D = (a_ltg + h_ltg) - (a + h) apart along the first axis, so Q = P + (D, 0, 0) +
// tau d with d the ray's direction.  The scan angles of step 1 are never formed: through them, Q would be found as the
// satellite's position plus 5.6 Earth radii of ray, and every rounding of the angles or of the root moves Q by itself
// divided by the sine of the ray's elevation -- a factor of 400 one degree inside the limb.  tau is a small number (the two
// ellipsoids are 6 to 16 km apart) that stays well conditioned up to the limb: it is the smaller root of
// A tau^2 + B tau + C = 0, written 2 C / (sqrt(B^2 - 4 A C) - B), where C, the lightning ellipsoid's equation at
// P + (D, 0, 0), is evaluated from the DIFFERENCES of the two ellipsoids' coefficients (P satisfies the grid ellipsoid's
// equation by construction), and never as a sum of terms near 1.
struct GdParallax {
    GdGeos grid;
    double shift, shift_rel;                                      // D in metres and in units of the grid's a
    double me, mp;                                                // (a / a_ltg)^2 and (a / b_ltg)^2
    double ke, kp;                                                // me - 1 and mp - (a / b)^2
    double lla_a, lla_f;
};

__host__ __device__ inline double gd_second_ecc2(double f) { const double e2 = f * (2.0 - f); return e2 / (1.0 - e2); }

__host__ __device__ inline GdParallax gd_parallax_setup(const TfGeos &grid, const TfGeos &ltg, double lla_a, double lla_rf)
{
    GdParallax c;
    c.grid = gd_geos_setup(grid);
    c.shift = (ltg.a - grid.a) + (ltg.h - grid.h);
    c.shift_rel = c.shift / grid.a;
    c.ke = (grid.a - ltg.a) * (grid.a + ltg.a) / (ltg.a * ltg.a);
    const double eg = gd_second_ecc2(grid.rf != 0 ? 1.0 / grid.rf : 0.0), el = gd_second_ecc2(ltg.rf != 0 ? 1.0 / ltg.rf : 0.0);
    c.kp = c.ke + el + c.ke * el - eg;
    c.me = 1.0 + c.ke;
    c.mp = c.me * (1.0 + el);
    c.lla_a = lla_a;
    c.lla_f = lla_rf != 0 ? 1.0 / lla_rf : 0.0;
    return c;
}

// Offsets (dlon, dlat) in degrees, the corrected scan angles (x, y) and Q's height above the third ellipsoid (the
// reference discards it).  Beyond the limb in step 1, or a ray that misses the lightning ellipsoid: NaN offsets and height,
// x = y = +inf, false.  NaN in: NaN in all five.
__host__ __device__ inline bool gd_glm_parallax_one(const GdParallax &c, double lat, double lon, double &dlon, double &dlat,
                                                    double &x, double &y, double &alt)
{
    const GdGeos &s = c.grid;
    double vx, vy, vz;
    const double vis = gd_geos_surface(s, lat, lon, vx, vy, vz);
    const double dx = vx - s.rg, wx = vx + c.shift_rel;
    const double C = (vx * vx + vy * vy) * c.ke + vz * vz * c.kp + (2.0 * vx * c.shift_rel + c.shift_rel * c.shift_rel) * c.me;
    const double B = 2.0 * ((wx * dx + vy * vy) * c.me + vz * vz * c.mp);
    const double A = (dx * dx + vy * vy) * c.me + vz * vz * c.mp;
    const double disc = B * B - 4.0 * A * C;
    if (!(vis >= 0.0) || !(disc >= 0.0)) {
        dlon = dlat = alt = NAN;
        x = y = (vis < 0.0 || disc < 0.0) ? HUGE_VAL : NAN;
        return false;
    }
    const double tau = C != 0.0 ? 2.0 * C / (sqrt(disc) - B) : 0.0;
    const double qx = (s.a * vx + c.shift) + tau * (s.a * dx), qy = s.a * vy + tau * (s.a * vy), qz = s.a * vz + tau * (s.a * vz);
    double lon_q, lat_q;
    gd_ecef_to_geodetic_one(c.lla_a, c.lla_f, qx, qy, qz, lon_q, lat_q, alt);
    dlon = gd_wrap180(lon_q + s.lon_0) - lon;
    dlat = lat_q - lat;
    gd_geos_forward_one(s, lat - dlat, lon - dlon, x, y);
    return true;
}

// ---- geodesic inverse ----------------------------------------------------------------------------------------------------
struct GdInverse { double az12, az21, s; int failed; };

// Vincenty's inverse on the ellipsoid (a, f): forward azimuth at point 1, back azimuth at point 2 in pyproj's
// convention (the direction from 2 back to 1: alpha2 -+ 180), both in degrees within [-180, 180], and the distance in
// the unit of a.  NaN in: NaN out, nothing iterated.  Coincident points: distance 0 and the azimuths GeographicLib
// gives, (180, 0) for lat1 >= 0 and (0, -180) below.  failed = 1 with three NaN: no convergence within GD_MAX_ITER, a
// longitude on the auxiliary sphere beyond pi, or the exact antipode.
__host__ __device__ inline GdInverse gd_geod_inverse_one(double a, double f, double lon1, double lat1, double lon2, double lat2)
{
    GdInverse out = {NAN, NAN, NAN, 0};
    if (lon1 != lon1 || lat1 != lat1 || lon2 != lon2 || lat2 != lat2) return out;
    const double b = (1.0 - f) * a;
    const double L = remainder(lon2 - lon1, 360.0) * GD_D2R;
    const double p1 = lat1 * GD_D2R, p2 = lat2 * GD_D2R;
    double su1 = (1.0 - f) * sin(p1), cu1 = cos(p1), su2 = (1.0 - f) * sin(p2), cu2 = cos(p2);
    const double n1 = hypot(su1, cu1), n2 = hypot(su2, cu2);
    su1 /= n1; cu1 /= n1; su2 /= n2; cu2 /= n2;
    double lam = L, ss = 0, cs = 0, sig = 0, sa = 0, c2a = 0, c2m = 0, sl = 0, cl = 0, t2 = 0;
    bool done = false;
    for (int it = 0; it < GD_MAX_ITER; it++) {
        sl = sin(lam); cl = cos(lam);
        const double t1 = cu2 * sl;
        t2 = cu1 * su2 - su1 * cu2 * cl;
        ss = sqrt(t1 * t1 + t2 * t2);
        cs = su1 * su2 + cu1 * cu2 * cl;
        if (ss == 0.0) {
            if (cs > 0.0) {                                       // coincident
                out.s = 0.0;
                out.az12 = lat1 >= 0.0 ? 180.0 : 0.0;
                out.az21 = lat1 >= 0.0 ? 0.0 : -180.0;
                return out;
            }
            break;                                                // the exact antipode: every azimuth is a geodesic
        }
        sig = atan2(ss, cs);
        sa = cu1 * cu2 * sl / ss;
        c2a = 1.0 - sa * sa;
        c2m = c2a != 0.0 ? cs - 2.0 * su1 * su2 / c2a : 0.0;
        const double C = f / 16.0 * c2a * (4.0 + f * (4.0 - 3.0 * c2a));
        const double next = L + (1.0 - C) * f * sa * (sig + C * ss * (c2m + C * cs * (-1.0 + 2.0 * c2m * c2m)));
        const double change = fabs(next - lam);
        if (!(fabs(next) <= GD_PI)) break;
        if (change <= GD_TOL) { done = true; break; }             // the terms above belong to lam, within GD_TOL of next
        lam = next;
    }
    if (!done) { out.failed = 1; return out; }
    const double u2 = c2a * (a * a - b * b) / (b * b);
    const double A = 1.0 + u2 / 16384.0 * (4096.0 + u2 * (-768.0 + u2 * (320.0 - 175.0 * u2)));
    const double B = u2 / 1024.0 * (256.0 + u2 * (-128.0 + u2 * (74.0 - 47.0 * u2)));
    const double ds = B * ss * (c2m + B / 4.0 * (cs * (-1.0 + 2.0 * c2m * c2m)
                                                - B / 6.0 * c2m * (-3.0 + 4.0 * ss * ss) * (-3.0 + 4.0 * c2m * c2m)));
    out.s = b * A * (sig - ds);
    out.az12 = atan2(cu2 * sl, t2) * GD_R2D;
    const double a2 = atan2(cu1 * sl, -su1 * cu2 + cu1 * su2 * cl) * GD_R2D;
    out.az21 = a2 >= 0.0 ? a2 - 180.0 : a2 + 180.0;
    return out;
}

// ---- grid spacing --------------------------------------------------------------------------------------------------------
// The reference's edge rule along one axis of n pixels (geo.py:230-236): d = zeros; d[:-1] = raw; d[1:] += d[:-1];
// d[1:-1] /= 2 -- the first pixel keeps its own raw spacing, an interior one the mean of the two next to it, the last one
// 0 + the previous.  raw_prev, raw_here: the raw spacing towards pixel i from i - 1 and from i towards i + 1.
__host__ __device__ inline double gd_spacing_rule(int64_t i, int64_t n, double raw_prev, double raw_here)
{
    if (n == 1) return 0.0;
    if (i == 0) return raw_here;
    if (i == n - 1) return 0.0 + raw_prev;
    return (raw_here + raw_prev) / 2.0;
}

// ---- viewing angles ------------------------------------------------------------------------------------------------------
__host__ __device__ inline double gd_clip1(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }   // np.clip(v, -1, 1): NaN stays

// np.remainder(v, 360.0)
__host__ __device__ inline double gd_mod360(double v)
{
    double r = fmod(v, 360.0);
    if (r != 0.0) { if (r < 0.0) r += 360.0; }
    else r = 0.0;
    return r;
}

// One pixel of the four reference functions, operations in the reference's order.  sc: the mode's scalars
//   TF_VIEW_SZA          geo.get_sza                        sc = delta, eqt, time (hours)       out0 = sza (rad)
//   TF_VIEW_SZA_AZI      geo.get_sza_and_azi                sc = declination, eqt, hour of day  out0, out1 = zenith, azimuth (deg)
//   TF_VIEW_SATELLITE    geo.get_satellite_viewing_angles   sc = sat_lat, sat_lon, sat_alt (km) out0, out1 = zenith, azimuth (deg)
//   TF_VIEW_ABI_ZENITH   abi.get_abi_zenith_angle           sc = lat_0, lon_0; sx, sy the pixel's scan angles   out0 (deg)
__host__ __device__ inline void gd_view_angles_one(int mode, const double *sc, double lat, double lon, double sx, double sy,
                                                   double &out0, double &out1)
{
    out1 = 0.0;
    if (mode == TF_VIEW_SZA || mode == TF_VIEW_SZA_AZI) {
        const double delta = sc[0], eqt = sc[1], hour = sc[2];
        const double omega = ((360.0 / 24.0) * (hour + lon / 15.0 + eqt - 12.0)) * GD_D2R;
        const double rl = lat * GD_D2R;
        const double sunh = sin(delta) * sin(rl) + cos(delta) * cos(rl) * cos(omega);
        if (mode == TF_VIEW_SZA) { out0 = GD_PI / 2.0 - asin(sunh); return; }
        const double sza = GD_PI / 2.0 - asin(gd_clip1(sunh));
        const double azimuth = (sin(delta) * cos(rl) - cos(delta) * sin(rl) * cos(omega)) / cos(GD_PI / 2.0 - sza);
        out0 = sza * GD_R2D;
        out1 = acos(gd_clip1(azimuth)) * GD_R2D;
        return;
    }
    if (mode == TF_VIEW_SATELLITE) {
        const double re = 6371.0, rgeo = sc[2] + re;
        const double dlat = (lat - sc[0]) * GD_D2R, dlon = (lon - sc[1]) * GD_D2R;
        const double cos_beta = cos(dlat) * cos(dlon);
        const double sin_beta = sin(acos(cos_beta));
        const double dist = sqrt(rgeo * rgeo + re * re - 2.0 * rgeo * re * cos_beta);
        double zen = asin(rgeo * sin_beta / dist) * GD_R2D;
        if (!(dist * dist < rgeo * rgeo - re * re)) zen = 180.0 - zen;
        const double xs = cos(dlat) * sin(dlon), ys = sin(dlat);
        out0 = zen;
        out1 = (xs - xs == 0.0) ? gd_mod360(atan2(xs, ys) * GD_R2D) : NAN;
        return;
    }
    const double dlat = (lat - sc[0]) * GD_D2R, dlon = (lon - sc[1]) * GD_D2R;
    const double xx = -sx, yy = -sy;
    const double dot = cos(dlon) * sin(dlat) * (cos(xx) * sin(yy)) + (-sin(dlon)) * (-sin(xx)) + cos(dlon) * cos(dlat) * (cos(xx) * cos(yy));
    out0 = acos(dot) * GD_R2D;
}
