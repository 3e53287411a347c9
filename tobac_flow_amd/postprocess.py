"""Per-label weighted statistics, their uncertainties and flag proportions of the post-processing scripts (mirrors
tobac_flow/postprocess.py:102-310: weighted_label_stats, add_weighted_stats_to_dataset, get_weighted_proportions_da,
add_weighted_proportions_to_dataset), on `LabelDataset`, numpy arrays and device tensors.

The reference makes every one of these calls an `apply_func_to_labels`: a bincount and an argsort of the whole label
volume, then a Python function per label.  Here a call is two reads of the volume and a finish per label on the GPU
(tf_label_wstats; one read for tf_label_proportions), with weights that vary with (y, x) only kept as one plane.  The
formulas are those of utils.stats_utils (weighted_stats, weighted_stats_and_uncertainties, get_weighted_proportions),
which remain the per-region host forms and the fallback for what the kernels do not take.

xarray is not in this image: names, dimension names and values are the reference's, `attrs` are not carried, and a flag
array's `flag_values` and `name` are keyword arguments because there is no DataArray to read them from.  The `*_groupby`
helpers, `process_*_properties`, `add_cre_to_dataset` and `add_validity_flags` of the reference's module are out of scope
(DESIGN.md)."""
from functools import partial

import numpy as np

from tobac_flow_amd.utils import stats_utils

STAT_NAMES = ("mean", "std", "min", "max", "mean_uncertainty", "mean_combined_error", "min_error", "max_error")
MAX_DEVICE_FLAGS = 64


def _lib():
    from tobac_flow_amd import _lib as lib
    return lib


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def _np_dtype(x):
    return np.dtype(str(x.dtype).replace("torch.", "")) if _is_tensor(x) else np.asarray(x).dtype


def _shape(x):
    return tuple(int(n) for n in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _host(x):
    return _lib().to_host(x) if _is_tensor(x) else np.asarray(x)


def _check_index(index):
    """the ids as a 1-D int64 array; ValueError for an id < 1 (labels <= 0 are background here)"""
    ids = _host(index) if _is_tensor(index) else np.asarray(list(index) if isinstance(index, range) else index)
    if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
        raise ValueError("index must be a one-dimensional sequence of integer label ids")
    ids = ids.astype(np.int64)
    if ids.size and ids.min() < 1:
        raise ValueError("index holds an id < 1: labels <= 0 are the background and have no statistics")
    return ids


def _layout(labels, weights, *fields):
    """How the operands go to the kernels: "volume" / "plane" (the weights' layout) for a (T, H, W) label volume whose
    fields have its shape and whose weights are (T, H, W), (H, W) or (1, H, W); None where the operands merely broadcast
    (the host form takes them).  ValueError where they do not broadcast against the labels at all."""
    shape = _shape(labels)
    others = [_shape(f) for f in fields] + [_shape(weights)]
    try:
        ok = np.broadcast_shapes(shape, *others) == shape
    except ValueError:
        ok = False
    if not ok:
        raise ValueError(f"labels {shape}, fields and weights {others} do not have the same shape (or one that broadcasts "
                         "to the labels')")
    if len(shape) != 3 or 0 in shape or any(s != shape for s in others[:-1]):
        return None
    if others[-1] == shape:
        return "volume"
    return "plane" if others[-1] in (shape[1:], (1,) + shape[1:]) else None


def _host_regions(labels, fields, func, ids, n_out):
    """func(*values of the region) for every id, regions in raveled (C) order -- a stable sort of the labels, so the first
    occurrence of an extreme is the smallest raveled index; ids without voxels give NaN: (len(ids), n_out) float64"""
    arrays = np.broadcast_arrays(_host(labels), *[_host(f) for f in fields])
    flat = arrays[0].ravel()
    order = np.argsort(flat, kind="stable")
    sorted_labels = flat[order]
    starts, stops = np.searchsorted(sorted_labels, ids, "left"), np.searchsorted(sorted_labels, ids, "right")
    out = np.full((len(ids), n_out), np.nan)
    values = [f.ravel() for f in arrays[1:]]
    for k in np.flatnonzero(stops > starts):
        where = order[starts[k]:stops[k]]
        out[k] = func(*[v[where] for v in values])
    return out


def _device_labels(labels, ids):
    """int32 device volume and the number of records the kernels keep.  That is the largest requested id -- labels above
    it are background to the kernels, so the volume need not be read to size them -- unless the index holds an id larger
    than the volume has voxels (dense label ids never are): then the largest label bounds it, and ids above are NaN."""
    lib = _lib()
    lab = lib.to_dev(labels, lib.torch().int32)
    if not ids.size or not lab.numel():
        return lab, 0
    top = int(ids.max())
    return lab, (top if top <= lab.numel() else min(top, int(lab.max())))


def _scatter(records, ids, n_labels, n_out):
    out = np.full((len(ids), n_out), np.nan)
    present = ids <= n_labels
    if n_labels > 0:
        out[present] = records[ids[present] - 1]
    return out


def _label_wstats(labels, field, errors, weights, ids):
    """(len(ids), 4 or 8) float64: the columns of STAT_NAMES for every id"""
    n_out = 8 if errors is not None else 4
    fields = (field,) if errors is None else (field, errors)
    layout = _layout(labels, weights, *fields)
    kinds = [_np_dtype(a).kind for a in fields + (weights,)]
    if layout is None or _np_dtype(labels).kind not in "iu" or any(k not in "fiub" for k in kinds):
        func = stats_utils.weighted_stats if errors is None else stats_utils.weighted_stats_and_uncertainties
        promote = [_host(f).astype(np.float64) for f in fields] + [_host(weights).astype(np.float64)]
        return _host_regions(labels, promote, func, ids, n_out)
    lib = _lib()
    t, L = lib.torch(), lib.lib()
    # one float type for the three operands and nothing cast down: float32 only where all of them are
    single = all(_np_dtype(a) == np.float32 for a in fields + (weights,))
    work = t.float32 if single else t.float64
    lab, n_labels = _device_labels(labels, ids)
    if n_labels <= 0:
        return np.full((len(ids), n_out), np.nan)
    x = lib.to_dev(field, work)
    e = None if errors is None else lib.to_dev(errors, work)
    w = lib.to_dev(weights, work)
    T, hw = lab.shape[0], lab.shape[1] * lab.shape[2]
    out = lib.empty((n_labels, 10), t.float64)
    ws = lib.workspace(L.tf_label_wstats_workspace_bytes(n_labels), "label_wstats")
    lib.check(L.tf_label_wstats(lib.ptr(lab), lib.ptr(x), lib.ptr(e), lib.ptr(w), lib.TF_F32 if single else lib.TF_F64,
                                T, hw, int(layout == "plane"), n_labels, lib.ptr(out), lib.ptr(ws), ws.numel(),
                                lib.stream_ptr()), "tf_label_wstats")
    return _scatter(out.cpu().numpy()[:, 2:2 + n_out], ids, n_labels, n_out)


def weighted_label_stats(labels, weights, dataset, var, coord, dim, dim_name=None, attrs=None, uncertainty=False,
                         dtype=None):
    """Weighted mean, Bessel-corrected weighted standard deviation, minimum and maximum of `dataset[var]` over every
    label id in `coord`, and with `uncertainty` the propagated uncertainty of the mean, its combined error and the
    `dataset[f"{var}_uncertainty"]` values at the minimum and at the maximum: 4 or 8 `(name, values)` pairs named
    f"{dim_name}_{var}_mean", _std, _min, _max, _mean_uncertainty, _mean_combined_error, _min_error, _max_error
    (reference: postprocess.py:102-208; `attrs` is accepted and ignored, there are no DataArrays here).

    Values that are not finite are left out; a label is NaN throughout unless it has a finite value and the weights at
    its finite values sum to > 0 (a NaN weight there makes it NaN); min and max include weight-0 voxels.  `weights` is
    (T, H, W), (H, W) or (1, H, W) -- a plane is never repeated to the volume.  Sums are accumulated in double.

    Divergences from the reference, all on ground it leaves undefined or accidental: `coord` may hold any ids >= 1 in any
    order and an id that is absent or beyond the largest label is NaN, but an id < 1 raises ValueError (the reference
    evaluates the background as a region there); where an extreme occurs more than once the error at the smallest raveled
    index is returned (the reference's unstable argsort leaves the choice open); the result has the field's dtype
    (float64 for an integer field) or `dtype=`, where the reference returns float64 whenever an id is absent and the
    field's dtype otherwise."""
    dim_name = dim if dim_name is None else dim_name
    ids = _check_index(coord)
    field = dataset[var]
    errors = dataset[f"{var}_uncertainty"] if uncertainty else None
    stats = _label_wstats(labels, field, errors, weights, ids)
    if dtype is None:
        dtype = _np_dtype(field) if _np_dtype(field).kind == "f" else np.float64
    return tuple((f"{dim_name}_{var}_{stat}", stats[:, k].astype(dtype)) for k, stat in enumerate(STAT_NAMES[:stats.shape[1]]))


def add_weighted_stats_to_dataset(dcc_dataset, field_dataset, weights, var, dim, dim_name=None, index=None, labels=None):
    """weighted_label_stats of `field_dataset[var]` over `labels` (default `dcc_dataset[f"{dim_name}_label"]`) for the
    ids `index` (default the coordinate `dcc_dataset.coords[dim]`), each result added to `dcc_dataset` with dims (dim,);
    the four uncertainty results are added when `field_dataset` holds f"{var}_uncertainty" (reference:
    postprocess.py:211-242).  Returns `dcc_dataset`."""
    dim_name = dim if dim_name is None else dim_name
    if index is None:
        index = dcc_dataset.coords[dim]
    if labels is None:
        labels = dcc_dataset[f"{dim_name}_label"]
    results = weighted_label_stats(labels, weights, field_dataset, var, index, dim, dim_name=dim_name,
                                   uncertainty=f"{var}_uncertainty" in field_dataset)
    for name, values in results:
        dcc_dataset.add(name, values, (dim,))
    return dcc_dataset


def _device_flags(flag_da, flag_values):
    """(int32 device flags, distinct int32 values, position of every requested value among them), or None where the kernel
    does not take them: non-integral float flags or values, anything beyond int32, more than 64 distinct values"""
    lib = _lib()
    values = np.asarray(flag_values)
    if values.dtype.kind == "f" and np.all(values == np.trunc(values)):
        values = values.astype(np.int64)
    if values.dtype.kind not in "iub":
        return None
    distinct, position = np.unique(values.astype(np.int64), return_inverse=True)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    if distinct.size > MAX_DEVICE_FLAGS or distinct[0] < lo or distinct[-1] > hi:
        return None
    dt = _np_dtype(flag_da)
    if dt.kind not in "fiub":
        return None
    t = lib.torch()
    if dt.kind == "f":
        whole = bool((flag_da == flag_da.trunc()).all()) if _is_tensor(flag_da) else bool(np.all(flag_da == np.trunc(flag_da)))
        if not whole:                                             # NaN included: it equals no listed value, as on the host
            return None
    if dt.kind == "f" or (dt.kind in "iu" and dt.itemsize >= 4 and dt != np.int32):
        if int(flag_da.min()) < lo or int(flag_da.max()) > hi:
            return None
    return lib.to_dev(flag_da, t.int32), distinct.astype(np.int32), position.reshape(-1)


def get_weighted_proportions_da(flag_da, weights, labels, dim, dim_name=None, index=None, *, flag_values, name, dtype=None):
    """For every label id in `index` (default 1 .. labels.max()) and every value of `flag_values`: the share of the
    label's weight that lies on voxels whose flag has that value -- an array of shape (len(index), len(flag_values)),
    float64 unless `dtype=` (reference: postprocess.py:245-286, which returns it as the DataArray
    f"{dim_name}_{name}_proportion" on (dim, name); `flag_values` and `name` are read from the flag DataArray there and
    are keyword arguments here).  NaN weights count nowhere; a row is NaN unless the label's weights sum to > 0; a flag
    value that is not listed counts towards the total only, so rows sum to <= 1.

    On the GPU for a (T, H, W) volume with integer or bool flags of any width (or float flags whose values are all
    integral), up to 64 distinct flag values and weights of shape (T, H, W), (H, W) or (1, H, W), which the kernel reads
    as float32; everything else is evaluated on the host by utils.stats_utils.get_weighted_proportions.  The ids follow
    the rules of weighted_label_stats (an id < 1 is a ValueError, the reference's background region)."""
    flag_values = np.asarray(list(flag_values))
    if flag_values.ndim != 1:
        raise ValueError("flag_values must be a one-dimensional sequence")
    K = flag_values.size
    layout = _layout(labels, weights, flag_da)
    if index is None:
        index = np.arange(1, max(int(labels.max()), 0) + 1) if np.prod(_shape(labels)) else np.zeros(0, np.int64)
    ids = _check_index(index)
    dtype = np.float64 if dtype is None else dtype
    if K == 0 or ids.size == 0:
        return np.full((ids.size, K), np.nan, dtype)
    prepared = _device_flags(flag_da, flag_values) if layout is not None and _np_dtype(labels).kind in "iu" else None
    if prepared is None:
        func = partial(stats_utils.get_weighted_proportions, flag_values=flag_values)
        return _host_regions(labels, [flag_da, weights], func, ids, K).astype(dtype)
    flags, distinct, position = prepared
    lib = _lib()
    t, L = lib.torch(), lib.lib()
    lab, n_labels = _device_labels(labels, ids)
    if n_labels <= 0:
        return np.full((ids.size, K), np.nan, dtype)
    w = lib.to_dev(weights, t.float32)
    T, hw = lab.shape[0], lab.shape[1] * lab.shape[2]
    out = lib.empty((n_labels, distinct.size), t.float64)
    ws = lib.workspace(L.tf_label_proportions_workspace_bytes(n_labels, distinct.size), "label_proportions")
    lib.check(L.tf_label_proportions(lib.ptr(lab), lib.ptr(flags), lib.ptr(w), T, hw, int(layout == "plane"), n_labels,
                                     distinct.ctypes.data, distinct.size, lib.ptr(out), lib.ptr(ws), ws.numel(),
                                     lib.stream_ptr()), "tf_label_proportions")
    return _scatter(out.cpu().numpy()[:, position], ids, n_labels, K).astype(dtype)


def add_weighted_proportions_to_dataset(dcc_dataset, flag_da, weights, dim, dim_name=None, index=None, labels=None, *,
                                        flag_values, name):
    """get_weighted_proportions_da over `labels` (default `dcc_dataset[f"{dim_name}_label"]`) for the ids `index`
    (default `dcc_dataset.coords[dim]`), added as f"{dim_name}_{name}_proportion" with dims (dim, name); `name` becomes a
    coordinate holding `flag_values` (reference: postprocess.py:289-310).  Returns `dcc_dataset`."""
    dim_name = dim if dim_name is None else dim_name
    if index is None:
        index = dcc_dataset.coords[dim]
    if labels is None:
        labels = dcc_dataset[f"{dim_name}_label"]
    proportions = get_weighted_proportions_da(flag_da, weights, labels, dim, dim_name=dim_name, index=index,
                                              flag_values=flag_values, name=name)
    dcc_dataset.coords[name] = np.asarray(list(flag_values))
    dcc_dataset.add(f"{dim_name}_{name}_proportion", proportions, (dim, name))
    return dcc_dataset


__all__ = ("weighted_label_stats", "add_weighted_stats_to_dataset", "get_weighted_proportions_da",
           "add_weighted_proportions_to_dataset")
