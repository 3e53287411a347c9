"""Per-label weighted statistics, their uncertainties and flag proportions of the post-processing scripts (mirrors
tobac_flow/postprocess.py:102-310: weighted_label_stats, add_weighted_stats_to_dataset, get_weighted_proportions_da,
add_weighted_proportions_to_dataset), on `LabelDataset`, numpy arrays and device tensors.

The reference makes every one of these calls an `apply_func_to_labels`: a bincount and an argsort of the whole label
volume, then a Python function per label.  Here a call is two reads of the volume and a finish per label on the GPU
(tf_label_wstats; one read for tf_label_proportions), with weights that vary with (y, x) only kept as one plane.  The
formulas are those of utils.stats_utils (weighted_stats, weighted_stats_and_uncertainties, get_weighted_proportions),
which remain the per-region host forms and the fallback for what the kernels do not take.

xarray is not in this image: names, dimension names and values are the reference's, `attrs` are not carried, and a flag
array's `flag_values` and `name` are keyword arguments because there is no DataArray to read them from.

The third stage is at the end of the module: process_core_properties, process_thick_anvil_properties,
process_thin_anvil_properties and add_validity_flags (postprocess.py:313-1314) over the step records of a LabelDataset
table, as batches of tf_group_reduce operations.

The fifth stage stands between the two: get_cre and add_cre_to_dataset (postprocess.py:29-99), cloud_quality_weights and
the scripts' cloud and flux sections as add_weighted_stats_of_fields, add_cloud_properties and add_flux_properties, which
evaluate a whole set of variables in one walk of a label volume (tf_label_wstats_multi)."""
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


# ---- the fifth stage: cloud and flux properties per object (reference: postprocess.py:29-99 and the scripts) ---------------
# scripts/postprocess_seviri_nat_dcc.py:180-298 (the same text in postprocess_seviri_dcc.py:79-165 and
# relabel_postprocess_seviri_cci.py:210-330): the quality weights, eleven cloud variables and five flags, add_cre_to_dataset
# and twenty flux variables, each over the three step-label volumes.  The reference makes ~100 calls of
# add_weighted_stats_to_dataset; here the variables of a call group share the two reads of a label volume
# (tf_label_wstats_multi) and the derived fluxes of the TOA / BOA sets are formed in registers.
STEP_DIMS = ("core_step", "thick_anvil_step", "thin_anvil_step")
CLOUD_VARIABLES = ("cot", "cer", "cwp", "ctp", "ctp_corrected", "cth", "cth_corrected", "ctt", "ctt_corrected", "stemp", "dem")
CLOUD_FLAGS = ("lsflag", "lusflag", "illum", "cldtype", "phase")
FLUX_VARIABLES = ("toa_swdn", "toa_swup", "toa_swup_cre", "toa_lwup", "toa_lwup_cre", "toa_net", "toa_net_cre",
                  "boa_swdn", "boa_swdn_cre", "boa_swup", "boa_swup_cre", "boa_lwdn", "boa_lwdn_cre", "boa_lwup", "boa_lwup_cre",
                  "boa_net", "boa_net_cre", "lts", "fth", "cbh")
CRE_NAMES = ("toa_swup_cre", "toa_lwup_cre", "boa_swdn_cre", "boa_swup_cre", "boa_lwdn_cre", "boa_lwup_cre",
             "toa_net", "toa_net_cre", "boa_net", "boa_net_cre")
# the field sets of tf_label_wstats_multi: input planes and fields in the kernel's order (include/tobac_flow_hip.h)
_SET_PLANES = {"TOA": ("toa_swdn", "toa_swup", "toa_swup_clr", "toa_lwup", "toa_lwup_clr"),
               "BOA": ("boa_swdn", "boa_swup", "boa_lwdn", "boa_lwup", "boa_swdn_clr", "boa_swup_clr", "boa_lwdn_clr", "boa_lwup_clr")}
_SET_FIELDS = {"TOA": FLUX_VARIABLES[:7], "BOA": FLUX_VARIABLES[7:17]}
_CRE_PLANES = _SET_PLANES["TOA"] + _SET_PLANES["BOA"]
# where a derived variable takes its dims from
_CRE_LIKE = dict([(name, name[:-4]) for name in CRE_NAMES[:6]] + [("toa_net", "toa_swdn"), ("toa_net_cre", "toa_swup"),
                                                                   ("boa_net", "boa_swdn"), ("boa_net_cre", "boa_swdn")])
MAX_FUSED_FIELDS = 8


def get_cre(flux, clear_flux):
    """The cloud radiative effect of a flux: `flux - clear_flux` (reference: postprocess.py:29-36, whose attrs and name
    are not carried here).  NumPy arrays or device tensors, one IEEE subtraction per element in the operands' type."""
    return flux - clear_flux


# the ten variables of add_cre_to_dataset in its order, each in the reference's expression tree over g(name) (the tree is
# what fixes the rounding); the operands are NumPy arrays or tensors
_CRE_TREES = {f"{v}_cre": (lambda g, v=v: get_cre(g(v), g(f"{v}_clr"))) for v in [name[:-4] for name in CRE_NAMES[:6]]}
_CRE_TREES.update({
    "toa_net": lambda g: g("toa_swdn") - (g("toa_swup") + g("toa_lwup")),
    "toa_net_cre": lambda g: -(g("toa_swup_cre") + g("toa_lwup_cre")),
    "boa_net": lambda g: g("boa_swdn") + g("boa_lwdn") - (g("boa_swup") + g("boa_lwup")),
    "boa_net_cre": lambda g: g("boa_swdn_cre") + g("boa_lwdn_cre") - (g("boa_swup_cre") + g("boa_lwup_cre"))})


def _cre_value(name, raw, memo):
    """the derived variable `name` from the raw variables `raw(name)`; the derived ones it is made of are kept in `memo`"""
    if name not in _CRE_TREES:
        return raw(name)
    if name not in memo:
        with np.errstate(invalid="ignore", over="ignore"):
            memo[name] = _CRE_TREES[name](lambda other: _cre_value(other, raw, memo))
    return memo[name]


def _float_dtype(arrays):
    """np.float32 / np.float64 where every array has that one dtype, else None"""
    dtypes = {_np_dtype(a) for a in arrays}
    dtype = dtypes.pop()
    return dtype if not dtypes and dtype in (np.float32, np.float64) else None


def _tf_dtype(dtype):
    return _lib().TF_F32 if np.dtype(dtype) == np.float32 else _lib().TF_F64


def _pointers(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if x is None else x.data_ptr() for x in tensors])


def add_cre_to_dataset(dataset):
    """Adds toa_swup_cre, toa_lwup_cre, boa_swdn_cre, boa_swup_cre, boa_lwdn_cre, boa_lwup_cre (flux - clear-sky flux),
    toa_net, toa_net_cre, boa_net and boa_net_cre to `dataset`, a LabelDataset or any mutable mapping name -> array, in that
    order, from its thirteen raw flux variables (reference: postprocess.py:39-99; no attrs here).  Returns `dataset`.

    Every expression is evaluated in the reference's tree with each operation rounded in the variables' own type
    (toa_net = swdn - (swup + lwup), boa_net = swdn + lwdn - (swup + lwup), ...): additions, subtractions and a negation, so
    the values are NumPy's.  NumPy arrays are evaluated by NumPy; where the variables are float32 or float64 device tensors
    of one shape, ONE kernel launch (tf_flux_cre) reads the thirteen planes once and writes the ten results.  The inputs
    are not modified.  In a LabelDataset each result takes the dims of its first source variable."""
    raw = [dataset[name] for name in _CRE_PLANES]                 # KeyError names what is missing
    if any(_is_tensor(x) for x in raw):
        lib = _lib()
        dtype = _float_dtype(raw)
        if dtype is None or len({_shape(x) for x in raw}) != 1:
            raise ValueError("add_cre_to_dataset: on the device the thirteen flux variables are float32 or float64 tensors of "
                             "one dtype and one shape")
        planes = [lib.to_dev(x) for x in raw]
        n = planes[0].numel()
        outs = [lib.empty(tuple(planes[0].shape), planes[0].dtype) for _ in CRE_NAMES]
        if n:
            lib.check(lib.lib().tf_flux_cre(_pointers(planes), _pointers(outs), _tf_dtype(dtype), n, lib.stream_ptr()), "tf_flux_cre")
        values = dict(zip(CRE_NAMES, outs))
    else:
        values = {}
        for name in CRE_NAMES:
            _cre_value(name, lambda raw: np.asarray(dataset[raw]), values)
    dims =getattr(dataset, "dims", None)
    for name in CRE_NAMES:
        if hasattr(dataset, "add") and isinstance(dims, dict) and _CRE_LIKE[name] in dims:
            dataset.add(name, values[name], dims[_CRE_LIKE[name]])
        else:
            dataset[name] = values[name]
    return dataset


def cloud_quality_weights(weights, qcflag, cth, cot):
    """`weights * (qcflag == 0) * (cth < 30) * isfinite(cot)` with the three masks as float32: the weights the scripts use
    for the cloud properties (postprocess_seviri_nat_dcc.py:181-186).  `weights` is (T, H, W), (H, W) or (1, H, W), the
    others (T, H, W); the result is (T, H, W), float32 if `weights` is float32 and float64 otherwise.  The three
    multiplications are made as written: a NaN or infinite weight times 0 is NaN, a NaN `cth` compares false.  NumPy
    arrays are evaluated by NumPy; with a device tensor among the operands one kernel (tf_quality_weights) reads the
    weights as the plane or volume they are."""
    operands = (weights, qcflag, cth, cot)
    shape = _shape(cth)
    if len(shape) != 3 or _shape(qcflag) != shape or _shape(cot) != shape:
        raise ValueError(f"cloud_quality_weights: qcflag {_shape(qcflag)}, cth {shape} and cot {_shape(cot)} are (T, H, W) arrays of one shape")
    layout = "volume" if _shape(weights) == shape else "plane" if _shape(weights) in (shape[1:], (1,) + shape[1:]) else None
    if layout is None:
        raise ValueError(f"cloud_quality_weights: weights {_shape(weights)} are neither {shape} nor {shape[1:]}")
    single = _np_dtype(weights) == np.float32
    if not any(_is_tensor(x) for x in operands):
        w = np.asarray(weights)
        w = w if single else w.astype(np.float64)
        with np.errstate(invalid="ignore"):
            out = w * (np.asarray(qcflag) == 0).astype(np.float32) * (np.asarray(cth) < 30).astype(np.float32) \
                * np.isfinite(cot).astype(np.float32)
        return np.ascontiguousarray(np.broadcast_to(out, shape))
    lib = _lib()
    t = lib.torch()
    w = lib.to_dev(weights, t.float32 if single else t.float64)
    qd = _np_dtype(qcflag)
    if qd.kind in "iub" and (qd.itemsize < 4 or qd == np.int32):
        q = lib.to_dev(qcflag, t.int32)
    else:                                                         # a width int32 does not hold, or a float flag: 0 stays the only 0
        q = lib.to_dev(qcflag)
        q = (q != 0).to(t.int32)
    both32 = _np_dtype(cth) == np.float32 and _np_dtype(cot) == np.float32
    work = t.float32 if both32 else t.float64                     # widening is exact: the comparison and the test are unchanged
    h, c = lib.to_dev(cth, work), lib.to_dev(cot, work)
    out = lib.empty(shape, w.dtype)
    if out.numel():
        lib.check(lib.lib().tf_quality_weights(lib.ptr(w), lib.TF_F32 if single else lib.TF_F64, int(layout == "plane"), lib.ptr(q),
                                               lib.ptr(h), lib.ptr(c), lib.TF_F32 if both32 else lib.TF_F64, shape[0],
                                               shape[1] * shape[2], lib.ptr(out), lib.stream_ptr()), "tf_quality_weights")
    return out


def _wstats_multi(lab, n_labels, set_name, planes, errors, w, plane):
    """tf_label_wstats_multi: (fields of the set, n_labels, 10) float64 on the host.  planes / errors / w: device tensors,
    the planes (and errors) of one float dtype, errors a list with None entries or None"""
    lib = _lib()
    t, L = lib.torch(), lib.lib()
    set_id = {"PLAIN": lib.TF_FIELDS_PLAIN, "TOA": lib.TF_FIELDS_TOA, "BOA": lib.TF_FIELDS_BOA}[set_name]
    n_fields = len(planes) if set_name == "PLAIN" else len(_SET_FIELDS[set_name])
    T, hw = lab.shape[0], lab.shape[1] * lab.shape[2]
    out = lib.empty((n_fields, n_labels, 10), t.float64)
    ws = lib.workspace(L.tf_label_wstats_multi_workspace_bytes(set_id, len(planes), n_labels), "label_wstats_multi")
    e = None if errors is None or all(x is None for x in errors) else _pointers(errors)
    lib.check(L.tf_label_wstats_multi(lib.ptr(lab), set_id, _pointers(planes), e, len(planes), lib.ptr(w),
                                      _tf_dtype(_np_dtype(planes[0])), _tf_dtype(_np_dtype(w)), T, hw, int(plane), n_labels,
                                      lib.ptr(out), lib.ptr(ws), ws.numel(), lib.stream_ptr()), "tf_label_wstats_multi")
    return out.cpu().numpy()


def _stats_stage(dcc_dataset, source, weights, variables, dims, sets):
    """The loop `for var in variables: for dim in dims: add_weighted_stats_to_dataset(dcc_dataset, source, weights, var,
    dim)` with the variables of a dim evaluated together.  `sets`: the names of the field sets ("TOA", "BOA") whose
    variables are evaluated from the RAW planes of `source`; a variable of no set is `source[var]`."""
    variables, dims = list(variables), list(dims)
    set_of = {var: s for s in sets for var in _SET_FIELDS[s]}
    plans, memo = [], {}

    for var in variables:
        errors = source[f"{var}_uncertainty"] if f"{var}_uncertainty" in source else None
        s = set_of.get(var)
        if s is not None:
            for name in _SET_PLANES[s]:
                if name not in source:
                    raise KeyError(name)
            planes = [source[name] for name in _SET_PLANES[s]]
            if errors is None and _float_dtype(planes) is not None and len({_shape(x) for x in planes}) == 1:
                plans.append((var, s, planes[0], None))
            else:                                                 # non-float planes, or errors: the variable itself, one call
                plans.append((var, None, _cre_value(var, source.__getitem__, memo), errors))
        else:
            plans.append((var, None, source[var], errors))        # KeyError names what is missing
    device = {}

    def dev(x, dtype=None):                                       # every operand goes to the device once for all dims
        key = (id(x), dtype)
        if key not in device:
            device[key] = (x, _lib().to_dev(x, dtype))            # x is kept: its id cannot be given to another array meanwhile
        return device[key][1]

    results = {}
    for dim in dims:
        labels, ids = dcc_dataset[f"{dim}_label"], _check_index(dcc_dataset.coords[dim])
        fused = {"TOA": [], "BOA": [], np.dtype(np.float32): [], np.dtype(np.float64): []}
        for var, s, field, errors in plans:
            operands = (field,) if errors is None else (field, errors)
            layout = _layout(labels, weights, *operands)          # ValueError where the shapes do not broadcast
            takes = layout is not None and _np_dtype(labels).kind in "iu" and _np_dtype(weights).kind in "fiub"
            if takes and s is not None:
                fused[s].append(var)
            elif takes and _float_dtype(operands) is not None:
                fused[_np_dtype(field)].append((var, field, errors))
            else:                                                 # the per-variable call of the loop (a set's variable as an array)
                field = field if s is None else _cre_value(var, source.__getitem__, memo)
                results[var, dim] = _label_wstats(labels, field, errors, weights, ids)
        if not any(fused.values()):
            continue
        lab, n_labels = _device_labels(labels, ids)
        if n_labels > 0:
            plane = _layout(labels, weights) == "plane"
            w = dev(weights, None if _np_dtype(weights) in (np.float32, np.float64) else _lib().torch().float64)
        for s in ("TOA", "BOA"):
            if not fused[s]:
                continue
            if n_labels > 0:
                records = _wstats_multi(lab, n_labels, s, [dev(source[name]) for name in _SET_PLANES[s]], None, w, plane)
            for var in fused[s]:                                  # the set's other fields are computed and dropped
                k = _SET_FIELDS[s].index(var)
                results[var, dim] = _scatter(records[k][:, 2:6], ids, n_labels, 4) if n_labels > 0 else np.full((len(ids), 4), np.nan)
        for dtype in (np.dtype(np.float32), np.dtype(np.float64)):
            group = fused[dtype]
            for start in range(0, len(group), MAX_FUSED_FIELDS):
                part = group[start:start + MAX_FUSED_FIELDS]
                if n_labels > 0:
                    records = _wstats_multi(lab, n_labels, "PLAIN", [dev(f) for _, f, _ in part],
                                            [None if e is None else dev(e) for _, _, e in part], w, plane)
                for k, (var, _, errors) in enumerate(part):
                    n_out = 4 if errors is None else 8
                    results[var, dim] = (_scatter(records[k][:, 2:2 + n_out], ids, n_labels, n_out) if n_labels > 0
                                         else np.full((len(ids), n_out), np.nan))
    kinds = {var: _np_dtype(field) for var, _, field, _ in plans}
    for var in variables:
        dtype = kinds[var] if kinds[var].kind == "f" else np.float64
        for dim in dims:
            stats = results[var, dim]
            for k, stat in enumerate(STAT_NAMES[:stats.shape[1]]):
                dcc_dataset.add(f"{dim}_{var}_{stat}", stats[:, k].astype(dtype), (dim,))
    return dcc_dataset


def add_weighted_stats_of_fields(dcc_dataset, field_dataset, weights, variables, dims=STEP_DIMS):
    """The result of

        for var in variables:
            for dim in dims:
                add_weighted_stats_to_dataset(dcc_dataset, field_dataset, weights, var, dim)

    -- the same names f"{dim}_{var}_{stat}" in the same order of insertion with the same dims and dtypes, eight per
    variable where `field_dataset` holds f"{var}_uncertainty" and four otherwise, KeyError for a missing variable,
    ValueError for an id < 1 or shapes that do not broadcast -- evaluated with one tf_label_wstats_multi per dim and group
    of at most eight variables of one float dtype: a label volume is read twice per group instead of twice per variable,
    float32 fields meet float64 weights without a copy of either, and host arrays are uploaded once for all dims.
    The exact results (min, max, the errors at them, the NaN pattern) are those of the loop; the summed ones agree to
    the last bits of a double sum whose order of addition is not fixed.  A variable the fused kernel does not take -- a
    non-float dtype, errors of another dtype than the field's, operands that merely broadcast -- goes through the
    per-variable call of the loop; the order of the results does not depend on that.  All variables are looked up
    before the first result is added.  Returns `dcc_dataset`."""
    return _stats_stage(dcc_dataset, field_dataset, weights, variables, dims, ())


def add_cloud_properties(dataset, cld_ds, weights, variables=CLOUD_VARIABLES, *, flags, dims=STEP_DIMS):
    """The cloud section of the post-processing scripts (postprocess_seviri_nat_dcc.py:190-215): the weighted statistics of
    `variables` (default: the scripts' eleven) through add_weighted_stats_of_fields, then for every flag of `flags` and
    every dim add_weighted_proportions_to_dataset, in the mapping's order.  `flags` maps a flag variable of `cld_ds` to its
    `flag_values` (the scripts' five are CLOUD_FLAGS; the values are an attribute of the DataArray there and have to be
    given here).  `weights` are usually cloud_quality_weights(...).  Returns `dataset`."""
    add_weighted_stats_of_fields(dataset, cld_ds, weights, variables, dims)
    for name, flag_values in flags.items():
        for dim in dims:
            add_weighted_proportions_to_dataset(dataset, cld_ds[name], weights, dim, flag_values=flag_values, name=name)
    return dataset


def add_flux_properties(dataset, flx_ds, weights, variables=FLUX_VARIABLES, dims=STEP_DIMS):
    """The flux section of the post-processing scripts (postprocess_seviri_nat_dcc.py:271-298): the result of
    add_cre_to_dataset(flx_ds) followed by add_weighted_stats_of_fields(dataset, flx_ds, weights, variables, dims), with
    `variables` defaulting to the scripts' twenty -- but `flx_ds` is NOT modified and the ten derived volumes never exist:
    the variables of the TOA set (toa_swdn .. toa_net_cre) and of the BOA set (boa_swdn .. boa_net_cre) are evaluated from
    the RAW planes of `flx_ds` by tf_label_wstats_multi, which forms the derived values per voxel with add_cre_to_dataset's
    own expressions, whether or not `flx_ds` already holds the derived names (the same bits either way).  A set is
    launched when one of its variables is requested; its other fields are computed and dropped.  The remaining variables
    (lts, fth, cbh, ...) are grouped as in add_weighted_stats_of_fields.  A raw plane that a requested variable needs and
    `flx_ds` lacks is a KeyError naming it.  Returns `dataset`."""
    return _stats_stage(dataset, flx_ds, weights, variables, dims, ("TOA", "BOA"))


# ---- the third stage: object properties from step records (reference: postprocess.py:313-1314) ---------------------------
# The reference makes one xarray.groupby per variable; here every function plans its column operations first and hands
# them to _groups.reduce_groups together: one grouping per dimension, sixteen operations per tf_group_reduce call.  With
# device columns nothing but the coordinates (and, where `geod_inv` is given, its inputs) is seen by the host.
_SUFFIX_OPS = (("_mean_uncertainty", "AVERAGE_UNCERTAINTY"), ("_mean_combined_error", None), ("_min_error", "PICK_ARGMIN"),
               ("_max_error", "PICK_ARGMAX"), ("_mean", "COMBINED_MEAN"), ("_std", "COMBINED_STD"), ("_min", "MIN"), ("_max", "MAX"))


def _as_like(x, like):
    """a host array as a device tensor where the table's columns are device tensors"""
    if _is_tensor(like) and not _is_tensor(x):
        x = np.asarray(x)
        x = x.view(np.int64) if x.dtype.kind in "mM" else x
        return _lib().torch().from_numpy(np.ascontiguousarray(x)).to(like.device)
    return x


def _azimuth_and_speed(lons, lats, t, geod_inv):
    """get_mean_object_azimuth_and_speed (reference: utils/geo_utils.py:62-84) with the geodesic inverse handed in"""
    from scipy.stats import circmean
    order = np.argsort(t)
    seconds = np.diff(t[order]).astype(np.int64) / 1e9
    azimuths, _, distances = geod_inv(lons[order][:-1], lats[order][:-1], lons[order][1:], lats[order][1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        speeds = np.asarray(distances) / seconds
    keep = np.isfinite(azimuths) & np.isfinite(speeds)
    if not keep.any():
        return np.nan, np.nan
    return circmean(np.asarray(azimuths)[keep], high=180, low=-180), np.mean(speeds[keep])


def _own_geod_inv(geod_inv):
    """geod_inv is the `.inv` of the package's own Geod"""
    from tobac_flow_amd import geo
    return isinstance(getattr(geod_inv, "__self__", None), geo.Geod) and getattr(geod_inv, "__func__", None) is geo.Geod.inv


def _propagation_batched(dataset, step, index_name, parent, geod_inv):
    """_propagation with ONE inverse call over the consecutive-record pairs of all objects, records sorted by (object, t):
    on the device where the coordinate columns are device tensors.  Then the circular mean per object, as
    _azimuth_and_speed takes it."""
    from scipy.stats import circmean
    groups, coord = _host(dataset[index_name]), np.asarray(dataset.coords[parent])
    t = _host(dataset[f"{step}_t"])
    t = np.asarray(t).astype("datetime64[ns]").view(np.int64) if np.asarray(t).dtype.kind == "M" else np.asarray(t)
    order = np.lexsort((t, groups))
    g_sorted = groups[order]
    pair = np.nonzero((g_sorted[1:] == g_sorted[:-1]) & np.isin(g_sorted[:-1], coord))[0]
    first, second = order[pair], order[pair + 1]
    lons, lats = dataset[f"{step}_lon"], dataset[f"{step}_lat"]
    out = np.full((coord.size, 2), np.nan)
    if pair.size == 0:
        return out[:, 0], out[:, 1]
    if _is_tensor(lons) and _is_tensor(lats):
        torch = _lib().torch()
        ia, ib = (torch.from_numpy(np.ascontiguousarray(i)).to(lons.device) for i in (first, second))
        azimuths, _, distances = geod_inv(lons[ia], lats[ia], lons[ib], lats[ib])
        azimuths, distances = _host(azimuths), _host(distances)
    else:
        lons, lats = _host(lons), _host(lats)
        azimuths, _, distances = geod_inv(lons[first], lats[first], lons[second], lats[second])
    seconds = (t[second] - t[first]).astype(np.int64) / 1e9
    with np.errstate(divide="ignore", invalid="ignore"):
        speeds = np.asarray(distances) / seconds
    keep = np.isfinite(azimuths) & np.isfinite(speeds)
    owner = g_sorted[pair]                                        # non-decreasing
    bounds = np.searchsorted(owner, coord, side="left"), np.searchsorted(owner, coord, side="right")
    for k, (b, e) in enumerate(zip(*bounds)):
        sel = keep[b:e]
        if sel.any():
            out[k] = circmean(np.asarray(azimuths)[b:e][sel], high=180, low=-180), np.mean(speeds[b:e][sel])
    return out[:, 0], out[:, 1]


def _propagation(dataset, step, index_name, parent, geod_inv):
    if _own_geod_inv(geod_inv):
        return _propagation_batched(dataset, step, index_name, parent, geod_inv)
    groups, coord = _host(dataset[index_name]), np.asarray(dataset.coords[parent])
    lons, lats = _host(dataset[f"{step}_lon"]), _host(dataset[f"{step}_lat"])
    t = _host(dataset[f"{step}_t"])
    t = np.asarray(t).astype("datetime64[ns]").view(np.int64) if np.asarray(t).dtype.kind == "M" else np.asarray(t)
    order = np.argsort(groups, kind="stable")
    bounds = np.searchsorted(groups[order], coord, side="left"), np.searchsorted(groups[order], coord, side="right")
    out = np.full((coord.size, 2), np.nan)
    for k, (b, e) in enumerate(zip(*bounds)):
        if e - b > 1:
            members = order[b:e]
            out[k] = _azimuth_and_speed(lons[members], lats[members], t[members], geod_inv)
    return out[:, 0], out[:, 1]


def _object_properties(dataset, kind, parent, extremes, rates, geod_inv=None, propagation=None):
    from tobac_flow_amd import _groups
    step = f"{kind}_step"
    index_name = f"{step}_{parent}_index"
    groups, coord = dataset[index_name], dataset.coords[parent]
    steps = _as_like(dataset.coords[step], groups)
    t_column = dataset[f"{step}_t"]
    t, area = _groups.as_ticks(t_column), dataset[f"{step}_area"]
    ops, finish = [], []

    def plan(op, then):
        ops.append(op)
        finish.append(then)

    def put(name):
        return lambda value: dataset.add(name, value, (parent,))

    def put_at(name, column):
        return lambda pick: dataset.add(name, _groups.take(column, pick), (parent,))

    def start_end(which, op):
        def then(pick):
            if kind == "core" and which == "start":
                dataset.add("core_initial_core_step_index", _groups.take(steps, pick), (parent,))
            for c in ("x", "y", "lat", "lon", "t"):
                dataset.add(f"{kind}_{which}_{c}", _groups.take(dataset[f"{step}_{c}"], pick), (parent,))
        plan((op, t), then)

    start_end("start", "PICK_ARGMIN")
    start_end("end", "PICK_ARGMAX")
    for c in ("x", "y", "lat", "lon"):
        plan(("WEIGHTED_AVERAGE", dataset[f"{step}_{c}"], area), put(f"{kind}_average_{c}"))
    plan(("MEAN", area), put(f"{kind}_average_area"))
    plan(("SUM", area), put(f"{kind}_total_area"))
    plan(("MAX", area), put(f"{kind}_max_area"))
    plan(("PICK_ARGMAX", area), put_at(f"{kind}_max_area_t", t_column))
    plan(("PICK_IDXMAX", area), put_at(f"{kind}_max_area_{step}_index", steps))
    for field, largest, t_name in extremes:
        if f"{step}_{field}_mean" not in dataset:
            continue
        column = dataset[f"{step}_{field}_mean"]
        word = "max" if largest else "min"
        plan(("PICK_ARGMAX" if largest else "PICK_ARGMIN", column), put_at(t_name or f"{kind}_{word}_{field}_t", t_column))
        plan(("PICK_IDXMAX" if largest else "PICK_IDXMIN", column), put_at(f"{kind}_{word}_{field}_{step}_index", steps))
        if field in rates:
            falling = -column if largest else column              # a height grows where its negative cools
            plan(("GRADIENT_MIN", falling, None, t), lambda value, name=rates[field]: dataset.add(name, -value * 6e10, (parent,)))
            plan(("GRADIENT_PICK_IDXMIN", falling, None, t), put_at(f"{rates[field]}_{step}_index", steps))

    combined_errors = []
    for var in [v for v in dataset if dataset.dims.get(v) == (step,)]:
        suffix, op = next(((s, o) for s, o in _SUFFIX_OPS if var.endswith(s)), (None, None))
        if suffix is None:
            continue
        new_var = f"{kind}_" + var[len(step) + 1:]
        if suffix == "_mean":
            plan((op, dataset[var], area), put(new_var))
        elif suffix == "_std":
            plan((op, dataset[var], area, dataset[var[:-3] + "mean"]), put(new_var))
        elif suffix in ("_min", "_max"):
            plan((op, dataset[var]), put(new_var))
        elif suffix == "_mean_uncertainty":
            plan((op, dataset[var], area), put(new_var))
        elif suffix == "_mean_combined_error":
            std_var = f"{kind}_" + var[len(step) + 1:-len("_mean_combined_error")] + "_std"
            slot = {}
            plan(("AVERAGE_UNCERTAINTY", dataset[var], area), lambda value, slot=slot: slot.update(uncertainty=value))
            plan(("COUNT",), lambda value, slot=slot: slot.update(counts=value.double() if _is_tensor(value) else value.astype(np.float64)))
            combined_errors.append((new_var, std_var, slot))
        else:                                                     # _min_error / _max_error: the error at the extreme of var[:-6]
            plan((op, dataset[var[:-6]]), put_at(new_var, dataset[var]))

    for then, value in zip(finish, _groups.reduce_groups(groups, coord, ops)):
        then(value)
    dataset.add(f"{kind}_lifetime", dataset[f"{kind}_end_t"] - dataset[f"{kind}_start_t"], (parent,))
    for new_var, std_var, slot in combined_errors:
        dataset.add(new_var, ((dataset[std_var] / slot["counts"] ** 0.5) ** 2 + slot["uncertainty"] ** 2) ** 0.5, (parent,))
    if geod_inv is not None and propagation is not None:
        direction, speed = _propagation(dataset, step, index_name, parent, geod_inv)
        dataset.add(f"{propagation}_propagation_direction", _as_like(direction, groups), (parent,))
        dataset.add(f"{propagation}_propagation_speed", _as_like(speed, groups), (parent,))
    return dataset


_CORE_EXTREMES = (("bt", False, None), ("ctt", False, None), ("ctt_corrected", False, None), ("cth", True, None),
                  ("cth_corrected", True, None))
_CORE_RATES = {"bt": "core_max_cooling_rate", "ctt": "core_ctt_cooling_rate", "ctt_corrected": "core_ctt_corrected_cooling_rate",
               "cth": "core_cth_growth_rate", "cth_corrected": "core_cth_corrected_growth_rate"}


def process_core_properties(dataset, time_steps=3, *, geod_inv=None):
    """Per core, from its core_step records (reference: postprocess.py:313-640): start / end position and time, lifetime,
    area-weighted average position, average / total / max area and when it was reached; for each of bt, ctt,
    ctt_corrected, cth, cth_corrected step means present, the time and step of the extreme and the steepest cooling (or
    growth) rate in K (or height) per minute with its step; and per core_step variable, by suffix, the combined _mean and
    _std, _min, _max, _mean_uncertainty, _mean_combined_error, _min_error and _max_error.  `time_steps` is accepted and
    unused, as in the reference.  A step index is 0 where the reference would yield NaN (utils.stats_utils.idxmin_groupby).

    core_propagation_direction and core_propagation_speed need a geodesic inverse: pass `geod_inv`, a callable with
    `pyproj.Geod.inv`'s signature (lons1, lats1, lons2, lats2) -> (azimuths, back azimuths, distances); with None they
    are left out.  With `tobac_flow_amd.geo.Geod().inv` all consecutive-record pairs of all cores go into ONE inverse call
    (on the device where the columns are device tensors), followed by the circular mean per core; any other callable is
    called once per core on the host, after get_mean_object_azimuth_and_speed.  Returns `dataset`."""
    return _object_properties(dataset, "core", "core", _CORE_EXTREMES, _CORE_RATES, geod_inv, "core")


def process_thick_anvil_properties(dataset, *, geod_inv=None):
    """process_core_properties for the anvils' thick_anvil_step records, without rates (reference: postprocess.py:643-922).
    anvil_propagation_direction / _speed are written only with `geod_inv` (see process_core_properties)."""
    extremes = (("bt", False, None), ("ctt", False, None), ("ctt_corrected", False, None), ("cth", True, None),
                # the reference's one misnamed assignment (postprocess.py:808): the time of the largest cth_corrected is written
                # to thick_anvil_min_ctt_corrected_t, over the value of the ctt_corrected branch; reproduced
                ("cth_corrected", True, "thick_anvil_min_ctt_corrected_t"))
    return _object_properties(dataset, "thick_anvil", "anvil", extremes, {}, geod_inv, "anvil")


def process_thin_anvil_properties(dataset):
    """process_core_properties for the anvils' thin_anvil_step records, without rates and propagation (reference:
    postprocess.py:925-1170)"""
    return _object_properties(dataset, "thin_anvil", "anvil", _CORE_EXTREMES, {})


def add_validity_flags(dataset):
    """core_has_anvil_flag, core_anvil_removed (core_anvil_index set to 0 for those), anvil_core_count,
    anvil_initial_core_index, anvil_no_growth_flag, anvil_no_initial_core_flag, core_is_valid, anvil_invalid_core_flag,
    thick_anvil_is_valid, thin_anvil_is_valid (reference: postprocess.py:1173-1314).  Needs the outputs of
    process_core_properties and process_thick_anvil_properties; every anvil must have a core (filter_anvils)."""
    from tobac_flow_amd import _groups
    from tobac_flow_amd.utils.filter_utils import _flag
    from tobac_flow_amd.utils.xarray_utils import isin_coord, mask_positions
    anvil = dataset.coords["anvil"]
    core_anvil = dataset["core_anvil_index"]
    has_anvil = isin_coord(core_anvil, anvil)
    dataset.add("core_has_anvil_flag", has_anvil, ("core",))
    dataset.add("core_anvil_removed", ~has_anvil & (core_anvil != 0), ("core",))
    core_anvil = core_anvil * has_anvil.to(core_anvil.dtype) if _is_tensor(core_anvil) else np.where(has_anvil, core_anvil, 0)
    dataset.add("core_anvil_index", core_anvil, ("core",))

    def flag(name):
        return _flag(dataset[name], has_anvil)

    invalid_core = flag("core_edge_label_flag") | flag("core_start_label_flag") | flag("core_end_label_flag")
    if "core_nan_flag" in dataset:
        invalid_core = invalid_core | flag("core_nan_flag")
    dataset.add("core_is_valid", ~invalid_core, ("core",))

    with_anvil = mask_positions(has_anvil)
    valid = (~invalid_core)[with_anvil]
    valid = valid.to(_lib().torch().float64) if _is_tensor(valid) else valid.astype(np.float64)
    counts, first_core, all_valid = _groups.reduce_groups(
        core_anvil[with_anvil], anvil, [("COUNT",), ("PICK_ARGMIN", _groups.as_ticks(dataset["core_start_t"])[with_anvil]), ("MIN", valid)])
    dataset.add("anvil_core_count", counts, ("anvil",))
    first_core = _groups.take(with_anvil, first_core)             # position among all cores
    dataset.add("anvil_initial_core_index", _groups.take(_as_like(dataset.coords["core"], has_anvil), first_core), ("anvil",))
    no_growth = dataset["thick_anvil_max_area_t"] <= _groups.take(dataset["core_end_t"], first_core)
    no_initial_core = dataset["thick_anvil_start_t"] < _groups.take(dataset["core_start_t"], first_core)
    dataset.add("anvil_no_growth_flag", no_growth, ("anvil",))
    dataset.add("anvil_no_initial_core_flag", no_initial_core, ("anvil",))
    invalid_cores = all_valid != 1
    dataset.add("anvil_invalid_core_flag", invalid_cores, ("anvil",))
    for kind in ("thick_anvil", "thin_anvil"):
        invalid = invalid_cores | no_growth | no_initial_core | flag(f"{kind}_edge_label_flag") | flag(f"{kind}_start_label_flag") | \
            flag(f"{kind}_end_label_flag")
        if f"{kind}_nan_flag" in dataset:
            invalid = invalid | flag(f"{kind}_nan_flag")
        dataset.add(f"{kind}_is_valid", ~invalid, ("anvil",))
    return dataset


__all__ = ("weighted_label_stats", "add_weighted_stats_to_dataset", "get_weighted_proportions_da",
           "add_weighted_proportions_to_dataset", "get_cre", "add_cre_to_dataset", "cloud_quality_weights",
           "add_weighted_stats_of_fields", "add_cloud_properties", "add_flux_properties", "process_core_properties", "process_thick_anvil_properties",
           "process_thin_anvil_properties", "add_validity_flags")
