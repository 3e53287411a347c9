"""The lmatools / glmtools coordinate systems the reference keeps in tobac_flow/_lmatools.py, without pyproj: every
system converts between its own coordinates and Earth-centred, Earth-fixed metres (`toECEF`, `fromECEF`), and two of them
chained give the GLM parallax correction (tobac_flow_amd.glm, which runs that chain fused, in one launch).  Names and
constructor arguments are the reference's; the arithmetic is tobac_flow_amd.geo's: NumPy arrays in, the NumPy float64 path;
device tensors in, the kernels of csrc/geodesy.hip and device tensors out.

Ellipsoids by name are "WGS84" and "GRS80"; `datum` is accepted and, as in the reference, changes nothing.  lmatools places
a fixed-grid system's satellite `sat_ecef_height` above ITS OWN ellipsoid's equator (PROJ's geos set-up), so the lightning
system's satellite stands 16 km further out than the ABI's: the reference's results contain that, and so do these.
"""
import numpy as np

from tobac_flow_amd import geo

# equatorial and polar radius of the ellipsoid GLM navigates its flashes to: the values at launch, and the revision of late 2018
lightning_ellipse_rev = {0: (6.394140e6, 6.362755e6), 1: (6.378137e6 + 14.0e3, 6.362755e6)}
this_ellps = 0
ltg_ellps_re, ltg_ellps_rp = lightning_ellipse_rev[this_ellps]


def semiaxes_to_invflattening(semimajor, semiminor):
    """the inverse flattening of an ellipse with these semi-axes"""
    return semimajor / (semimajor - semiminor)


def _axes_to_a_rf(r_equator, r_pole):
    if r_equator is None:
        raise ValueError("r_pole needs r_equator")
    r_pole = r_equator if r_pole is None else r_pole
    return float(r_equator), (0.0 if r_pole == r_equator else float(semiaxes_to_invflattening(r_equator, r_pole)))


class CoordinateSystem:
    """a system converts to and from ECEF metres: X towards (lat 0, lon 0), Z towards the north pole"""

    def toECEF(self, x, y, z):
        raise NotImplementedError

    def fromECEF(self, x, y, z):
        raise NotImplementedError


class GeographicSystem(CoordinateSystem):
    """longitude, latitude (degrees) and height (metres) on an ellipsoid named by `ellipse`, or given by `r_equator` and
    `r_pole` (a sphere without r_pole).  NumPy scalars come back as arrays of one element."""

    def __init__(self, ellipse="WGS84", datum="WGS84", r_equator=None, r_pole=None):
        if r_equator is not None or r_pole is not None:
            self.a, self.rf = _axes_to_a_rf(r_equator, r_pole)
        else:
            self.a, self.rf = geo._ellipsoid(ellipse, None, None)

    @staticmethod
    def _operands(values):
        return tuple(v if geo._is_tensor(geo._unwrap(v)) else np.atleast_1d(v) for v in values)

    def toECEF(self, lon, lat, alt):
        lon, lat, alt = self._operands((lon, lat, alt))
        return geo.geodetic_to_ecef(lon, lat, alt, a=self.a, rf=self.rf)

    def fromECEF(self, x, y, z):
        x, y, z = self._operands((x, y, z))
        return geo.ecef_to_geodetic(x, y, z, a=self.a, rf=self.rf)


class GeographicSystemAltEllps(GeographicSystem):
    """GeographicSystem whose `r_equator`, `r_pole` go through semiaxes_to_invflattening; scalars stay scalars (0-d arrays)"""

    @staticmethod
    def _operands(values):
        return values


class GeostationaryFixedGridSystem(CoordinateSystem):
    """the fixed grid of a geostationary imager: scan angles (x, y) in radians, seen from `sat_ecef_height` above the
    ellipsoid's equator at `subsat_lon`; sweep_axis "x" is GOES, "y" Meteosat.  `toECEF(x, y, 0)` is the point where the ray
    meets the ellipsoid (+inf where it misses); the reference never passes another z, and another z is a ValueError.
    `fromECEF` gives the scan angles of the point's geodetic position and its height over sat_ecef_height."""

    def __init__(self, subsat_lon=0.0, subsat_lat=0.0, sweep_axis="y", sat_ecef_height=35785831.0, ellipse="WGS84", datum="WGS84"):
        self.h = sat_ecef_height
        self.proj = geo.GeosProj(h=sat_ecef_height, lon_0=subsat_lon, lat_0=subsat_lat, sweep=sweep_axis, ellps=ellipse)

    def toECEF(self, x, y, z):
        z = geo._unwrap(z)
        if bool((z != 0).any()) if hasattr(z, "any") else z != 0:
            raise ValueError("a fixed-grid system converts points on its ellipsoid only: z must be 0")
        return self.proj.to_ecef(x, y)

    def fromECEF(self, x, y, z):
        sx, sy, alt = self.proj.from_ecef(x, y, z)
        return sx, sy, alt / self.h


class GeostationaryFixedGridSystemAltEllipse(GeostationaryFixedGridSystem):
    """GeostationaryFixedGridSystem on the ellipsoid with the given semi-axes"""

    def __init__(self, subsat_lon=0.0, subsat_lat=0.0, sweep_axis="y", sat_ecef_height=35785831.0, semimajor_axis=None,
                 semiminor_axis=None, datum="WGS84"):
        if semimajor_axis is None or semiminor_axis is None:
            raise ValueError("semimajor_axis and semiminor_axis are both needed")
        self.h = sat_ecef_height
        self.proj = geo.GeosProj(h=sat_ecef_height, lon_0=subsat_lon, lat_0=subsat_lat, sweep=sweep_axis, a=semimajor_axis,
                                 rf=semiaxes_to_invflattening(semimajor_axis, semiminor_axis))


GOESR_SAT_ECEF_HEIGHT = 35786023.0                            # GOES-R PUG volume 3


def get_GOESR_coordsys(sat_lon_nadir=-75.0):
    """`(geofixcs, grs80lla)`: the GOES-R fixed grid on GRS80 and the geographic system on GRS80"""
    geofixcs = GeostationaryFixedGridSystem(subsat_lon=sat_lon_nadir, ellipse="GRS80", sweep_axis="x",
                                            sat_ecef_height=GOESR_SAT_ECEF_HEIGHT)
    return geofixcs, GeographicSystem(ellipse="GRS80")


def get_GOESR_coordsys_alt_ellps(sat_lon_nadir=-75.0):
    """`(geofixcs, lla)`: the same pair on the lightning ellipsoid"""
    geofixcs = GeostationaryFixedGridSystemAltEllipse(subsat_lon=sat_lon_nadir, semimajor_axis=ltg_ellps_re,
                                                      semiminor_axis=ltg_ellps_rp, sweep_axis="x",
                                                      sat_ecef_height=GOESR_SAT_ECEF_HEIGHT)
    return geofixcs, GeographicSystemAltEllps(r_equator=ltg_ellps_re, r_pole=ltg_ellps_rp)
