"""The statistics helpers the drop-in scripts reach (reference: utils/stats_utils.py:11-30, :33-168 and :366-367).

The weighted_* functions and get_weighted_proportions are the per-region host forms: one region's values in, scalars
out.  tobac_flow_amd.postprocess evaluates them for all labels at once on the GPU (tf_label_wstats,
tf_label_proportions) and falls back to these for inputs the kernels do not take."""
import numpy as np


def mse(a, b):
    return np.nansum((a - b) ** 2) / np.sum(np.isfinite(a - b))


def _sorted_form(a, axis):
    """number of distinct non-zero values along `axis` on the host, for what the kernels do not take: sort the lines,
    then count the entries that are non-zero and differ from their predecessor; int32"""
    b = np.sort(np.moveaxis(np.asarray(a), axis, 0), axis=0)
    new = np.ones(b.shape, bool)
    new[1:] = b[1:] != b[:-1]
    return np.count_nonzero(new & (b != 0), axis=0).astype(np.int32)


def _stamps_fit(lo, hi, size):
    """can tf_unique_per_frame take these ids?  It keeps one int32 stamp per id up to the largest, so the ids must be
    non-negative and the table no larger than the data itself (dense label ids never exceed the voxel count; one stray
    huge id must not buy a table of its size)"""
    return lo >= 0 and hi <= size


def find_overlap_mode(x, background=0):
    """The most frequent value of `x` that is not `background`, the smallest among equally frequent ones (what
    scipy.stats.mode returns); `background` itself where there is no other value (reference: stats_utils.py:11-20).
    Passed as `func` to labeled_comprehension / apply_func_to_labels with device tensors it is recognised and evaluated
    for all labels at once on the GPU (utils/label_utils.py)."""
    x = np.asarray(x)
    kept = x[x != background]
    if kept.size == 0:
        return background
    values, counts = np.unique(kept, return_counts=True)
    return values[np.argmax(counts)]


def n_unique_along_axis(a, axis: int = 0):
    """Number of unique values along an axis of an array (reference: stats_utils.py:23-30), which is the number of
    distinct non-zero values along the axis; int32.  Integer arrays / device tensors of 2 or 3 dimensions are counted on
    the GPU.  tf_unique_along_t takes the axis moved to the front (a view or a permutation) in ONE launch and is the
    default.  tf_unique_per_frame costs one launch per line, so it takes only few long lines along the last axis -- the
    (t, y * x) view of get_label_stats: lines longer than 640 entries (beyond that the along-t kernel needs scratch of the
    array's size and searches sets that long) and no more lines than a line has entries.  Anything else (float data,
    other ranks, values beyond int32, lines of 65536 entries or more that the per-frame kernel cannot take, empty arrays)
    is counted on the host."""
    from tobac_flow_amd import _lib
    from tobac_flow_amd import label as _label
    tensor = _lib.is_tensor(a)
    if not tensor:
        a = np.asarray(a)
    ndim = a.dim() if tensor else a.ndim
    integer = (not a.dtype.is_floating_point and not a.dtype.is_complex and a.dtype != _lib.torch().bool) if tensor \
        else a.dtype.kind in "iu"
    size = a.numel() if tensor else a.size

    def on_host():
        return _sorted_form(_lib.to_host(a) if tensor else a, axis)

    if not integer or ndim not in (2, 3) or size == 0:
        return on_host()
    axis = axis % ndim
    lo, hi = int(a.min()), int(a.max())
    if lo < -2 ** 31 or hi > 2 ** 31 - 1:
        return on_host()
    shape = tuple(int(n) for n in a.shape)
    out_shape = shape[:axis] + shape[axis + 1:]
    length, lines = shape[axis], size // shape[axis]
    if axis == ndim - 1 and length > 640 and lines <= length and lines < 65536 and _stamps_fit(lo, hi, size):
        uniq, _ = _label.unique_per_frame(a.reshape(lines, length), hi)
        return uniq.reshape(out_shape)
    if length >= 65536:
        return on_host()
    moved = a.movedim(axis, 0) if tensor else np.moveaxis(a, axis, 0)
    if ndim == 2:
        moved = moved[:, None, :]
    if not tensor:
        moved = np.ascontiguousarray(moved, np.int32)
    uniq, _, _ = _label.unique_along_t(moved)
    return uniq.reshape(out_shape)


def _finite_part(data, *others, ignore_nan=True):
    """the arrays restricted to where `data` is finite (np.isfinite: NaN and both infinities go)"""
    arrays = [np.asarray(a) for a in (data,) + others]
    if not ignore_nan:
        return arrays
    keep = np.isfinite(arrays[0])
    return [a[keep] for a in arrays]


def weighted_average_and_std(data, weights, unbiased: bool = True):
    """mean = sum w x / sum w and the standard deviation about it, sqrt(sum w (x - mean)^2 / sum w / c) with Bessel's
    correction for reliability weights c = 1 - sum w^2 / (sum w)^2; NaN where c < 0 (reference: stats_utils.py:33-50,
    whose `unbiased=False` leaves std unset; here it gives the uncorrected value)."""
    data, weights = np.asarray(data), np.asarray(weights)
    total = np.sum(weights)
    mean = np.sum(weights * data) / total
    var = np.sum(weights * (data - mean) ** 2) / total
    if not unbiased:
        return mean, np.sqrt(var)
    c = 1 - np.sum(weights ** 2) / total ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(var / c) if c >= 0 else np.nan
    return mean, std


def weighted_stats(data, weights, ignore_nan: bool = True, default=np.nan):
    """(mean, std, min, max) of one region over its finite values; `default` four times unless there is a finite value
    and their weights sum to > 0 (a NaN weight makes the sum NaN).  min and max include weight-0 values (reference:
    stats_utils.py:53-73)."""
    data, weights = _finite_part(data, weights, ignore_nan=ignore_nan)
    if data.size == 0 or not np.sum(weights) > 0:
        return default, default, default, default
    mean, std = weighted_average_and_std(data, weights)
    return mean, std, np.min(data), np.max(data)


def weighted_average_uncertainty(errors, weights):
    """propagated uncertainty of a weighted mean, sqrt(sum w^2 e^2) / sum w (reference: stats_utils.py:76-86)"""
    errors, weights = np.asarray(errors), np.asarray(weights)
    if errors.size == 0 or not np.sum(weights) > 0:
        return np.nan
    return np.sqrt(np.sum(weights ** 2 * errors ** 2)) / np.sum(weights)


def weighted_uncertainties(data, errors, weights, std, ignore_nan: bool = True):
    """(uncertainty of the mean, sqrt((std / sqrt(n))^2 + uncertainty^2), error at the minimum, error at the maximum) of
    one region; the first occurrence of an extreme is taken (reference: stats_utils.py:89-117)."""
    data, errors, weights = _finite_part(data, errors, weights, ignore_nan=ignore_nan)
    if data.size == 0 or not np.sum(weights) > 0:
        return np.nan, np.nan, np.nan, np.nan
    uncertainty = weighted_average_uncertainty(errors, weights)
    combined = np.sqrt((std / np.sqrt(data.size)) ** 2 + uncertainty ** 2)
    return uncertainty, combined, errors[np.argmin(data)], errors[np.argmax(data)]


def weighted_stats_and_uncertainties(data, errors, weights, ignore_nan: bool = True):
    """weighted_stats followed by weighted_uncertainties: eight values (reference: stats_utils.py:120-154)"""
    stats = weighted_stats(data, weights, ignore_nan=ignore_nan)
    return stats + weighted_uncertainties(data, errors, weights, stats[1], ignore_nan=ignore_nan)


def get_weighted_proportions(data, weights, flag_values):
    """per flag value, the share of the region's (non-NaN) weight that lies on it; NaN throughout unless the weights sum
    to > 0.  A flag that is not listed counts towards the total only (reference: stats_utils.py:157-168)."""
    data, weights = np.asarray(data).ravel(), np.asarray(weights, float).ravel()
    flag_values = np.asarray(list(flag_values))
    total = np.nansum(weights)
    if not total > 0:
        return np.full(flag_values.size, np.nan)
    counted = np.where(np.isnan(weights), 0.0, weights)
    with np.errstate(invalid="ignore"):
        return np.array([np.nansum(np.where(data == f, counted, 0.0)) for f in flag_values]) / total


def calc_combined_mean(step_mean, step_area):
    """area-weighted mean of one object's step means over the steps where mean and area are both finite; NaN where there
    is none (reference: stats_utils.py:171-179)"""
    step_mean, step_area = np.asarray(step_mean), np.asarray(step_area)
    keep = np.isfinite(step_mean) & np.isfinite(step_area)
    if not keep.any():
        return np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum(step_mean[keep] * step_area[keep]) / np.sum(step_area[keep])


def calc_combined_std(step_std, step_mean, step_area):
    """sqrt((sum a s + sum a (m - combined mean)^2) / sum a) over the steps where all three are finite, as the reference
    writes it (the step value enters unsquared); NaN where there is none (reference: stats_utils.py:182-199)"""
    step_std, step_mean, step_area = np.asarray(step_std), np.asarray(step_mean), np.asarray(step_area)
    combined_mean = calc_combined_mean(step_mean, step_area)
    keep = np.isfinite(step_std) & np.isfinite(step_mean) & np.isfinite(step_area)
    if not keep.any():
        return np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((np.sum(step_area[keep] * step_std[keep]) + np.sum(step_area[keep] * (step_mean[keep] - combined_mean) ** 2))
                       / np.sum(step_area[keep]))


# ---- per-object reductions over step records (reference: stats_utils.py:202-349) -----------------------------------------
# Every *_groupby takes 1-D record columns, the records' `groups` column (the *_step_*_index variable) and `coord`, the
# sorted ids of the objects, and returns one value per id of `coord`: device tensors in, a device tensor out
# (tf_group_reduce); NumPy arrays in, a NumPy array out.  Members of a group are taken in record order.  Unlike the
# reference, a record whose id is missing from `coord` and a `coord` id without records raise ValueError.
def _reduce(groups, coord, *ops):
    from tobac_flow_amd import _groups
    return _groups.reduce_groups(groups, coord, list(ops))


def _take(column, pick, missing=0):
    from tobac_flow_amd import _groups
    return _groups.take(column, pick, missing)


def combined_mean_groupby(means, area, groups, coord):
    """calc_combined_mean per object"""
    return _reduce(groups, coord, ("COMBINED_MEAN", means, area))[0]


def combined_std_groupby(stds, means, area, groups, coord):
    """calc_combined_std per object"""
    return _reduce(groups, coord, ("COMBINED_STD", stds, area, means))[0]


def weighted_average_uncertainty_groupby(field, area, groups, coord):
    """weighted_average_uncertainty(errors=field, weights=area) per object"""
    return _reduce(groups, coord, ("AVERAGE_UNCERTAINTY", field, area))[0]


def weighted_average_groupby(field, area, groups, coord):
    """np.average(field, weights=area) per object (NaN propagates); NaN where the weights sum to zero, which np.average
    refuses"""
    return _reduce(groups, coord, ("WEIGHTED_AVERAGE", field, area))[0]


def argmax_groupby(field, find_max, groups, coord):
    """per object, `field` at the step where `find_max` is largest (np.argmax: the first such step, the first NaN if any)"""
    return _take(field, _reduce(groups, coord, ("PICK_ARGMAX", find_max))[0])


def argmin_groupby(field, find_min, groups, coord):
    """per object, `field` at the step where `find_min` is smallest (np.argmin: the first such step, the first NaN if any)"""
    return _take(field, _reduce(groups, coord, ("PICK_ARGMIN", find_min))[0])


def counts_groupby(groups, coord):
    """number of step records per object; int64"""
    return _reduce(groups, coord, ("COUNT",))[0]


def idxmin_groupby(steps, field, groups, coord):
    """per object, the step id (from the `steps` column, which the reference reads off the DataArray's index) at the
    smallest non-NaN `field`.  An object whose `field` is NaN throughout gets step id 0 -- step ids start at 1 -- where
    the reference would yield a float NaN."""
    return _take(steps, _reduce(groups, coord, ("PICK_IDXMIN", field))[0])


def idxmax_groupby(steps, field, groups, coord):
    """idxmin_groupby for the largest non-NaN `field`; step id 0 for an object that is NaN throughout"""
    return _take(steps, _reduce(groups, coord, ("PICK_IDXMAX", field))[0])


def cooling_rate_groupby(BT, times, groups, coord):
    """per object, -min(np.gradient(BT, times, edge_order=1)) * 6e10 with `times` in nanoseconds (datetime64[ns] or int64
    ticks, taken as float64): kelvin per minute.  NaN for an object of one step."""
    return -_reduce(groups, coord, ("GRADIENT_MIN", BT, None, times))[0] * 6e10


def idxmax_cooling_rate_groupby(steps, BT, times, groups, coord):
    """the step id at that steepest cooling; step id 0 where there is none (one step, or NaN throughout), where the
    reference would yield a float NaN"""
    return _take(steps, _reduce(groups, coord, ("GRADIENT_PICK_IDXMIN", BT, None, times))[0])


__all__ = ("mse", "find_overlap_mode", "n_unique_along_axis", "weighted_average_and_std", "weighted_stats", "weighted_average_uncertainty",
           "weighted_uncertainties", "weighted_stats_and_uncertainties", "get_weighted_proportions", "calc_combined_mean",
           "calc_combined_std", "combined_mean_groupby", "combined_std_groupby", "weighted_average_uncertainty_groupby",
           "weighted_average_groupby", "argmax_groupby", "argmin_groupby", "counts_groupby", "idxmin_groupby", "idxmax_groupby",
           "cooling_rate_groupby", "idxmax_cooling_rate_groupby")
