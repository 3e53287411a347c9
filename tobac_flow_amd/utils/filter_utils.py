"""Filters of the third stage on a dataset.LabelDataset table (reference: utils/filter_utils.py:10-289).

The reference evaluates every criterion with its own xarray.groupby over the step records; here each filter groups once
per dimension and evaluates its criteria in one tf_group_reduce call (tobac_flow_amd._groups).  Columns that are device
tensors are reduced, compared and cut on the device; the host sees the coordinates.  Times are datetime64[ns] arrays or,
on the device, their int64 nanosecond ticks.  A step record without its object, or an object without step records in a
table that is grouped, raises ValueError -- run remove_orphan_coords first, as the reference's scripts do."""
from datetime import timedelta

import numpy as np

from tobac_flow_amd import _groups, _lib
from tobac_flow_amd.utils.xarray_utils import cut_dim, cut_steps, isin_coord, mask_positions


def _ns(delta):
    return int(delta / timedelta(microseconds=1)) * 1000


def _ticks(t):
    """times as int64 nanoseconds"""
    return t if _lib.is_tensor(t) else np.asarray(t).astype("datetime64[ns]").view(np.int64)


def _coord_in_column(coord, column):
    """np.isin(coord, column): which ids of a coordinate occur in a column; on the device for a device column"""
    if _lib.is_tensor(column):
        t = _lib.torch()
        return t.isin(t.from_numpy(np.ascontiguousarray(coord)).to(column.device), column)
    return np.isin(coord, np.asarray(column))


def _flag(x, like):
    """a per-object flag variable as a boolean of the container kind of `like`"""
    if _lib.is_tensor(like):
        return (x.to(like.device) if _lib.is_tensor(x) else _lib.torch().from_numpy(np.ascontiguousarray(x)).to(like.device)) != 0
    return (_lib.to_host(x) if _lib.is_tensor(x) else np.asarray(x)) != 0


def _valid(invalid):
    return int((~invalid).sum())


def remove_orphan_coords(dataset):
    """Remove cores / anvils which don't have core / anvil steps and vice versa (an anvil needs thick AND thin steps)"""
    wh_core = _coord_in_column(dataset.coords["core"], dataset["core_step_core_index"])
    wh_anvil = _coord_in_column(dataset.coords["anvil"], dataset["thick_anvil_step_anvil_index"]) & \
        _coord_in_column(dataset.coords["anvil"], dataset["thin_anvil_step_anvil_index"])
    dataset = cut_dim(dataset, "core", mask_positions(wh_core))
    dataset = cut_dim(dataset, "anvil", mask_positions(wh_anvil))
    dataset = cut_steps(dataset, "core_step", "core_step_core_index", "core")
    dataset = cut_steps(dataset, "thick_anvil_step", "thick_anvil_step_anvil_index", "anvil")
    return cut_steps(dataset, "thin_anvil_step", "thin_anvil_step_anvil_index", "anvil")


def _first_present(dataset, *names):
    return next((n for n in names if n in dataset), None)


def filter_cores(dataset, verbose: bool = False, min_lifetime: timedelta = timedelta(minutes=14),
                 max_time_gap: timedelta = timedelta(minutes=16)):
    """Keep the cores that cool by at least 8 K from first to last step (core_step_bt_mean, else core_step_ctt_mean, else
    no such test), have no gap between consecutive steps above `max_time_gap`, live at least `min_lifetime`, never exceed
    an area of 1e4, and have no NaN step mean while flagged in core_nan_flag (any NaN step where that flag is absent);
    then drop the steps of the removed cores."""
    if verbose:
        print(f"Initial core count: {dataset.coords['core'].size}")
    groups, coord = dataset["core_step_core_index"], dataset.coords["core"]
    bt = _first_present(dataset, "core_step_bt_mean", "core_step_ctt_mean")
    t = _ticks(dataset["core_step_t"])
    ops = [("MAX_DIFF", t), ("LAST_MINUS_FIRST", t), ("MAX", dataset["core_step_area"])]
    if bt is not None:
        ops += [("FIRST_MINUS_LAST", dataset[bt]), ("ANY_NAN", dataset[bt])]
    res = _groups.reduce_groups(groups, coord, ops)
    invalid_time_diff = res[0] > _ns(max_time_gap)
    invalid_lifetime = res[1] < _ns(min_lifetime)
    invalid_area = res[2] > 1e4
    none = invalid_area & ~invalid_area
    invalid_bt = res[3] < 8 if bt is not None else none
    any_nan_step = res[4] != 0 if bt is not None else none
    if "core_nan_flag" in dataset:
        any_nan_step = any_nan_step & _flag(dataset["core_nan_flag"], any_nan_step)
    if verbose:
        print(f"Valid core cooling: {_valid(invalid_bt)}")
        print(f"Valid time gaps: {_valid(invalid_time_diff)}")
        print(f"Valid lifetime: {_valid(invalid_lifetime)}")
        print(f"Valid maximum area: {_valid(invalid_area)}")
        print(f"Valid NaN flagging: {_valid(any_nan_step)}")
    invalid = invalid_bt | invalid_time_diff | invalid_lifetime | invalid_area | any_nan_step
    dataset = cut_dim(dataset, "core", mask_positions(~invalid))
    if verbose:
        print(f"Final core count: {dataset.coords['core'].size}")
    return cut_steps(dataset, "core_step", "core_step_core_index", "core")


def _cut_anvil_steps(dataset):
    dataset = cut_steps(dataset, "thick_anvil_step", "thick_anvil_step_anvil_index", "anvil")
    return cut_steps(dataset, "thin_anvil_step", "thin_anvil_step_anvil_index", "anvil")


def filter_anvils(dataset, verbose: bool = False, min_lifetime: timedelta = timedelta(minutes=14),
                  max_time_gap: timedelta = timedelta(minutes=16)):
    """Keep the anvils that have a core, no NaN thin-anvil step mean while flagged in thin_anvil_nan_flag
    (thin_anvil_step_bt_mean, else thin_anvil_step_ctt_mean, else no such test), a thick-anvil lifetime of at least
    `min_lifetime`, no gap between thick-anvil steps above `max_time_gap`, a largest thick-anvil area above the largest
    core_max_area of their cores, and a last thick-anvil step after the last core_end_t of their cores; then drop the
    steps of the removed anvils.  Needs core_max_area and core_end_t (process_core_properties)."""
    if verbose:
        print(f"Initial anvil count: {dataset.coords['anvil'].size}")
    has_core = _coord_in_column(dataset.coords["anvil"], dataset["core_anvil_index"])
    if verbose:
        print(f"Core present: {int(has_core.sum())}")
    dataset = _cut_anvil_steps(cut_dim(dataset, "anvil", mask_positions(has_core)))
    coord = dataset.coords["anvil"]

    bt = _first_present(dataset, "thin_anvil_step_bt_mean", "thin_anvil_step_ctt_mean")
    t = _ticks(dataset["thick_anvil_step_t"])
    lifetime, max_time_diff, max_area, end_t = _groups.reduce_groups(
        dataset["thick_anvil_step_anvil_index"], coord,
        [("LAST_MINUS_FIRST", t), ("MAX_DIFF", t), ("MAX", dataset["thick_anvil_step_area"]), ("MAX", t)])
    invalid_lifetime = lifetime < _ns(min_lifetime)
    invalid_time_diff = max_time_diff > _ns(max_time_gap)
    if bt is not None:
        any_nan_step = _groups.reduce_groups(dataset["thin_anvil_step_anvil_index"], coord, [("ANY_NAN", dataset[bt])])[0] != 0
    else:
        any_nan_step = invalid_lifetime & ~invalid_lifetime
    if "thin_anvil_nan_flag" in dataset:
        any_nan_step = any_nan_step & _flag(dataset["thin_anvil_nan_flag"], any_nan_step)

    core_anvil = dataset["core_anvil_index"]
    with_anvil = mask_positions(isin_coord(core_anvil, coord))
    max_core_area, core_end_t = _groups.reduce_groups(
        core_anvil[with_anvil], coord, [("MAX", dataset["core_max_area"][with_anvil]), ("MAX", _ticks(dataset["core_end_t"])[with_anvil])])
    invalid_area = max_area <= max_core_area
    invalid_end_t = end_t <= core_end_t
    if verbose:
        print(f"Valid NaN flagging: {_valid(any_nan_step)}")
        print(f"Valid lifetime: {_valid(invalid_lifetime)}")
        print(f"Valid time gaps: {_valid(invalid_time_diff)}")
        print(f"Valid anvil area: {_valid(invalid_area)}")
        print(f"Valid anvil end time: {_valid(invalid_end_t)}")
    invalid = any_nan_step | invalid_lifetime | invalid_time_diff | invalid_area | invalid_end_t
    dataset = cut_dim(dataset, "anvil", mask_positions(~invalid))
    if verbose:
        print(f"Final anvil count: {dataset.coords['anvil'].size}")
    return _cut_anvil_steps(dataset)


__all__ = ("remove_orphan_coords", "filter_cores", "filter_anvils")
