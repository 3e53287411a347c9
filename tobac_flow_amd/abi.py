"""The geodesy of the reference's tobac_flow/abi.py (abi.py:8-104) and get_goes_sza: the ABI fixed grid to latitude and
longitude, pixel lengths and area, the satellite zenith angle, and points onto the grid.  The RGB composites and the
channel getters of that module stay out.

`dataset` is anything with `.x`, `.y` and `.goes_imager_projection` -- an xarray Dataset where one exists, a LabelDataset
given those attributes, or a small attribute object.  Read from it: `x` and `y`, the 1-D scan angles in radians (their
`.data` or `.values` where they have one; NumPy arrays, or device tensors for the device path), and of
`goes_imager_projection` (its `.attrs` where it has them, else its attributes) `perspective_point_height`,
`longitude_of_projection_origin`, `latitude_of_projection_origin` (must be 0), `sweep_angle_axis`, and, where present,
`semi_major_axis` with `inverse_flattening` (GRS80, PROJ's default and the GOES-R value, otherwise).

x, y NumPy: the NumPy float64 path.  x, y device tensors: the kernels of csrc/geodesy.hip, device tensors out.
"""
import numpy as np

from tobac_flow_amd import geo


def _values(v):
    if isinstance(v, np.ndarray):                                 # (a datetime64 array has no buffer to offer as `.data`)
        return v
    for name in ("data", "values"):
        inner = getattr(v, name, None)
        if inner is not None and not callable(inner) and (geo._is_tensor(inner) or isinstance(inner, np.ndarray)):
            return inner
    return v if geo._is_tensor(v) else np.asarray(v)


def _projection_attr(dataset, name, default=None):
    proj = dataset.goes_imager_projection
    attrs = getattr(proj, "attrs", None)
    if attrs is not None and name in attrs:
        return attrs[name]
    value = getattr(proj, name, default)
    if value is None:
        raise AttributeError(f"goes_imager_projection has no {name}")
    return value


def get_abi_proj(dataset):
    """the geos projection of an ABI file (reference: abi.py:8-18), a geo.GeosProj"""
    return geo.GeosProj(
        h=float(_projection_attr(dataset, "perspective_point_height")),
        lon_0=float(_projection_attr(dataset, "longitude_of_projection_origin")),
        lat_0=float(_projection_attr(dataset, "latitude_of_projection_origin", 0.0)),
        sweep=str(_projection_attr(dataset, "sweep_angle_axis", "x")),
        a=float(_projection_attr(dataset, "semi_major_axis", geo.ELLIPSOIDS["GRS80"][0])),
        rf=float(_projection_attr(dataset, "inverse_flattening", geo.ELLIPSOIDS["GRS80"][1])),
    )


def get_abi_lat_lon(dataset, dtype=float):
    """`(lat, lon)` of every pixel, (H, W) in `dtype` (float64 or float32), NaN off the disk (reference: abi.py:21-39)"""
    return get_abi_proj(dataset).inverse_grid(_values(dataset.x), _values(dataset.y), dtype=dtype)


def get_abi_pixel_lengths(dataset):
    """`(dx, dy)` of every pixel in km (reference: abi.py:42-56)"""
    lat, lon = get_abi_lat_lon(dataset)
    return geo.grid_spacing(lat, lon, ("dx", "dy"))


def get_abi_pixel_area(dataset):
    """the area of every pixel in square km (reference: abi.py:59-65)"""
    lat, lon = get_abi_lat_lon(dataset)
    return geo.grid_spacing(lat, lon, ("area",))[0]


def get_abi_zenith_angle(abi_ds):
    """the satellite zenith angle of every pixel in degrees (reference: abi.py:68-89)"""
    lat, lon = get_abi_lat_lon(abi_ds)
    scalars = (float(_projection_attr(abi_ds, "latitude_of_projection_origin", 0.0)),
               float(_projection_attr(abi_ds, "longitude_of_projection_origin")))
    return geo.view_angles(3, scalars, lat, lon, _values(abi_ds.x), _values(abi_ds.y))[0]


def get_abi_x_y(lat, lon, dataset):
    """the scan angles `(x, y)` of points given by latitude and longitude, +inf beyond the limb (reference: abi.py:92-104)"""
    return get_abi_proj(dataset).forward_points(lat, lon)


def get_goes_sza(goes_ds):
    """the solar zenith angle in radians of every pixel at the file's time `goes_ds.t`, one datetime64, datetime or ISO
    string (reference: abi.py:253-256)"""
    from datetime import datetime
    t = goes_ds.t
    if isinstance(t, datetime):
        date = t
    elif isinstance(t, str):
        date = datetime.fromisoformat(t)
    else:
        date = np.asarray(_values(t)).reshape(-1)[0].astype("datetime64[us]").item()
    lat, lon = get_abi_lat_lon(goes_ds)
    return geo.get_sza(date, lat, lon)


__all__ = ("get_abi_proj", "get_abi_lat_lon", "get_abi_pixel_lengths", "get_abi_pixel_area", "get_abi_zenith_angle",
           "get_abi_x_y", "get_goes_sza")
