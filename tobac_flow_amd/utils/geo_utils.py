"""Geodesic helpers (reference: tobac_flow/utils/geo_utils.py) on the package's own geodesic inverse, tobac_flow_amd.geo.Geod.
NumPy arrays in: NumPy out.  Device tensors in: the kernels of csrc/geodesy.hip, device tensors out."""
import numpy as np

from tobac_flow_amd import geo

GEO = geo.Geod(ellps="WGS84")


def get_grid_spacing_from_lat_lon(lat, lon):
    """`(dx, dy)`: the grid spacing of each pixel in km from 2-D latitude and longitude arrays (geo_utils.py:9-23)"""
    return geo.grid_spacing(lat, lon, ("dx", "dy"), GEO)


def get_area_from_lat_lon(lat, lon):
    """the area of each pixel in square km from 2-D latitude and longitude arrays (geo_utils.py:26-34)"""
    return geo.grid_spacing(lat, lon, ("area",), GEO)[0]


def add_area_to_dataset(dataset, squeeze=False):
    """`dataset["area"]` from `dataset["lat"]` and `dataset["lon"]` of a LabelDataset (geo_utils.py:37-59).  Without a `t`
    dimension: float32 on the dimensions of lat.  With one: the area of the first time step, float64, repeated along `t`,
    or (squeeze=True, where the reference leaves its result unassigned) kept once on the remaining dimensions."""
    dims = tuple(dataset.dims["lat"])
    lat, lon = dataset["lat"], dataset["lon"]
    tensor = geo._is_tensor(lat) or geo._is_tensor(lon)
    if "t" in dims:
        axis = dims.index("t")
        first = (slice(None),) * axis + (0,)
        area = get_area_from_lat_lon(lat[first], lon[first])
        if squeeze:
            dims = dims[:axis] + dims[axis + 1:]
        else:
            n_t = int(lat.shape[axis])
            if tensor:
                area = area.unsqueeze(axis).repeat_interleave(n_t, axis)
            else:
                area = np.repeat(np.expand_dims(area, axis), n_t, axis)
    else:
        area = get_area_from_lat_lon(lat, lon)
        area = area.float() if tensor else area.astype(np.float32)
    dataset.add("area", area, dims)
    return dataset


def get_mean_object_azimuth_and_speed(lons, lats, t):
    """the average direction (degrees) and speed (m/s) of propagation of one object from its longitudes, latitudes and
    times (datetime64[ns], or integer nanoseconds) (geo_utils.py:62-84): host code, as in the reference"""
    from scipy.stats import circmean
    lons, lats, t = np.asarray(lons, dtype=np.float64), np.asarray(lats, dtype=np.float64), np.asarray(t)
    sort_args = np.argsort(t)
    lifetime_seconds = np.diff(t[sort_args]).astype(int) / 1e9
    azimuths, _, distances = GEO.inv(lons[sort_args][:-1], lats[sort_args][:-1], lons[sort_args][1:], lats[sort_args][1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        speeds = distances / lifetime_seconds
    wh_finite = np.logical_and(np.isfinite(azimuths), np.isfinite(speeds))
    if np.any(wh_finite):
        return circmean(azimuths[wh_finite], high=180, low=-180), np.mean(speeds[wh_finite])
    return np.nan, np.nan


__all__ = ("get_grid_spacing_from_lat_lon", "get_area_from_lat_lon", "add_area_to_dataset", "get_mean_object_azimuth_and_speed")
