"""Time-coordinate helpers used by the growth-rate recipes and by linking.process_file
(reference: utils/datetime_utils.py:9-166; pandas and dateutil only, xarray optional).

The three trims take a dataset.LabelDataset where the reference takes an xr.Dataset: the `t` coordinate and every variable
with a `t` dimension are cut to the dates of the file name, as `dataset.sel(t=slice(start, end - 1 s))` cuts them (both ends
inclusive).  NumPy arrays and device tensors alike become views of the originals."""
import pathlib
from datetime import datetime, timedelta

import numpy as np


def get_dates_from_filename(filename) -> tuple[datetime, datetime]:
    """Start and end date of a tobac-flow file name `..._SYYYYMMDD_HHMMSS_EYYYYMMDD_HHMMSS_...` (str or pathlib.Path;
    anything else raises ValueError)."""
    from dateutil.parser import parse as parse_date
    if isinstance(filename, str):
        name = filename.split("/")[-1]
    elif isinstance(filename, pathlib.Path):
        name = filename.name
    else:
        raise ValueError("filename parameter must be either a string or a Path object")
    start_date = parse_date(name.split("_S")[-1][:15], fuzzy=True)
    end_date = parse_date(name.split("_E")[-1][:15], fuzzy=True)
    return start_date, end_date


def _sel_t(dataset, start=None, stop=None):
    """dataset.sel(t=slice(start, stop)) on a LabelDataset (label-based: both ends inclusive)"""
    t = np.asarray(dataset.coords["t"])
    lo = 0 if start is None else int(np.searchsorted(t, np.datetime64(start), side="left"))
    hi = t.size if stop is None else int(np.searchsorted(t, np.datetime64(stop), side="right"))
    hi = max(hi, lo)
    out = type(dataset)(coords=dataset.coords)
    out.coords["t"] = t[lo:hi]
    for name, data in dataset.items():
        dims = dataset.dims.get(name)
        if dims is None and (name.endswith("_label") or name in ("bt", "wvd", "swd", "BT")):
            dims = ("t", "y", "x")                       # a volume stored without its dimension names
        if dims is not None and "t" in dims:
            index = [slice(None)] * dims.index("t") + [slice(lo, hi)]
            data = data[tuple(index)]
        out[name] = data
        if name in dataset.dims:
            out.dims[name] = dataset.dims[name]
    return out


def trim_file_start(dataset, filename):
    """Trim padding time steps from the start of a dataset"""
    return _sel_t(dataset, get_dates_from_filename(filename)[0], None)


def trim_file_end(dataset, filename):
    """Trim padding time steps from the end of a dataset"""
    return _sel_t(dataset, None, get_dates_from_filename(filename)[1] - timedelta(seconds=1))


def trim_file_start_and_end(dataset, filename):
    """Trim padding time steps from the start and end of a dataset"""
    start, end = get_dates_from_filename(filename)
    return _sel_t(dataset, start, end - timedelta(seconds=1))


def get_datetime_from_coord(coord) -> list[datetime]:
    import pandas as pd
    return pd.to_datetime(np.asarray(getattr(coord, "values", coord))).to_pydatetime().tolist()


def time_diff(datetime_list: list[datetime]) -> list[float]:
    """Centred first differences in fractional minutes, one-sided at the ends."""
    n = len(datetime_list)
    head = [(datetime_list[1] - datetime_list[0]).total_seconds() / 60]
    mid = [(datetime_list[i + 2] - datetime_list[i]).total_seconds() / 120 for i in range(n - 2)]
    tail = [(datetime_list[-1] - datetime_list[-2]).total_seconds() / 60]
    return head + mid + tail


def get_time_diff_from_coord(coord) -> np.ndarray:
    return np.array(time_diff(get_datetime_from_coord(coord)))


__all__ = ("get_dates_from_filename", "trim_file_start", "trim_file_end", "trim_file_start_and_end",
           "get_datetime_from_coord", "time_diff", "get_time_diff_from_coord")
