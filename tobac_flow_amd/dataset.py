"""The label contract of the detection output files, at array level (mirrors /root/reference/tobac_flow/dataset.py:189-1595).

After detection the drop-in scripts (scripts/dcc_detect_goes.py:316-330) derive, from the three label volumes
`core_label`, `thick_anvil_label`, `thin_anvil_label`, the variables every later stage (linking.py, analysis.py) reads:
`*_step_label`, the coordinates `core` / `anvil` / `*_step`, `core_anvil_index`, `anvil_core_count`, the
`*_step_*_index` arrays and the edge / start / end / NaN flags.  The reference keeps them in an xarray.Dataset and writes
NetCDF; xarray / netCDF4 are not in this image, so the container here is `LabelDataset` -- a dict of arrays with `.dims`
and `.coords` -- and writing files is out of scope.  Names, dtypes, dimension names and values are the reference's.

What the reference does per label in Python (scipy.ndimage.labeled_comprehension / apply_func_to_labels with a
bincount or a mode per label) is ONE pair-count pass over the two volumes on the GPU (tf_pair_counts, label.hip) and a
small host reduction over the distinct pairs; the per-step relabelling is tf_slice_labels; LUT applications are
tf_apply_lut.  Ties are broken as the reference's tools do (np.argmax / scipy.stats.mode: the smallest label wins).

The per-field summaries that go into the product beside the labels -- get_bulk_stats, get_spatial_stats,
get_temporal_stats (dataset.py:19-148) -- are here too: a device field is reduced in HBM by tf_field_stats.
"""
import numpy as np

from tobac_flow_amd import _lib
from tobac_flow_amd import label as _label

_KINDS = (("core", "core"), ("thick_anvil", "anvil"), ("thin_anvil", "anvil"))


class LabelDataset(dict):
    """name -> array (numpy, or a device tensor for the label volumes); `.dims[name]` = dimension names, `.coords` =
    coordinate name -> 1-D numpy array.  Stands in for the xr.Dataset of the reference's scripts."""

    def __init__(self, *args, coords=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.coords = dict(coords or {})
        self.dims = {}

    def add(self, name, data, dims, dtype=None):
        """add_dataarray_to_ds(create_dataarray(data, dims, name, dtype=dtype), ds) (dataset.py:20-60)"""
        if dtype is not None and not _lib.is_tensor(data):
            data = np.asarray(data).astype(dtype)
        self[name] = data
        self.dims[name] = tuple(dims)
        return data


def _host(x):
    return _lib.to_host(x) if _lib.is_tensor(x) else np.asarray(x)


def _like(result_dev, template):
    """device result in the container kind of `template` (numpy in -> numpy out)"""
    return result_dev if _lib.is_tensor(template) else _lib.to_host(result_dev)


def _apply_lut(labels_dev, lut):
    """lut[labels] for a device int32 volume and a host int32 table (tf_apply_lut; ids outside the table -> 0)"""
    t = _lib.torch()
    lab = labels_dev.contiguous()
    lut_t = t.from_numpy(np.ascontiguousarray(lut, np.int32)).to(lab.device)
    out = t.empty_like(lab)
    _lib.check(_lib.lib().tf_apply_lut(_lib.ptr(lab), lab.numel(), _lib.ptr(lut_t), lut_t.numel(), _lib.ptr(out),
                                       _lib.stream_ptr()), "tf_apply_lut")
    return out


def _present_ids(*volumes):
    """sorted non-zero label values of the volumes (np.unique minus 0), int32"""
    ids = np.zeros(0, np.int64)
    for v in volumes:
        sizes = _label.label_sizes(v)
        ids = np.union1d(ids, np.nonzero(sizes)[0])
    return ids[ids != 0].astype(np.int32)


def create_new_goes_ds(goes_ds, device=None):
    """A LabelDataset on the grid of an ABI file with `lat`, `lon` (degrees, NaN off the disk) and `area` (km2), float32 on
    (y, x) (reference: dataset.py:151-186).  goes_ds: anything with `.t`, `.y`, `.x` (scan angles) and
    `.goes_imager_projection`, as tobac_flow_amd.abi reads them, and optionally `.y_image`, `.x_image`; the projection and
    the host coordinates are kept on the result as attributes of the same names, so that it can be handed to
    tobac_flow_amd.abi again (the coordinate vectors are host arrays, as in every LabelDataset).  lat and lon are computed in float64 and rounded once, the area from the float64 values.
    device: None -- on the GPU when x and y are device tensors (device tensors out) or when a HIP device is visible (NumPy
    out); False -- the NumPy path; True -- the GPU, device tensors out."""
    from tobac_flow_amd import abi, geo
    x, y = abi._values(goes_ds.x), abi._values(goes_ds.y)
    tensors_in = _lib.is_tensor(x) or _lib.is_tensor(y)
    on_device = tensors_in or device is True or (device is None and _lib.torch().cuda.is_available())
    coords = {"t": np.atleast_1d(np.asarray(abi._values(goes_ds.t))), "y": _host(y), "x": _host(x)}
    for name in ("y_image", "x_image"):
        if getattr(goes_ds, name, None) is not None:
            coords[name] = np.asarray(abi._values(getattr(goes_ds, name)))
    new_ds = LabelDataset(coords=coords)
    new_ds.goes_imager_projection = goes_ds.goes_imager_projection
    new_ds.t, new_ds.y, new_ds.x = coords["t"], coords["y"], coords["x"]
    proj = abi.get_abi_proj(goes_ds)
    if on_device:
        x, y = _lib.to_dev(x), _lib.to_dev(y)
    lat, lon = proj.inverse_grid(x, y)
    area = geo.grid_spacing(lat, lon, ("area",))[0]
    keep_dev = tensors_in or device is True
    for name, value in (("lat", lat), ("lon", lon), ("area", area)):
        if on_device:
            value = value.float()
            value = value if keep_dev else _lib.to_host(value)
        else:
            value = value.astype(np.float32)
        new_ds.add(name, value, ("y", "x"))
    return new_ds


def add_step_labels(dataset):
    """`core_step_label`, `thick_anvil_step_label`, `thin_anvil_step_label` = slice_labels of the three label volumes,
    int32 on (t, y, x) (reference: dataset.py:189-229)."""
    for kind, _ in _KINDS:
        src = dataset[kind + "_label"]
        step, _n = _label.slice_labels_dev(src)
        dataset.add(kind + "_step_label", _like(step, src), ("t", "y", "x"))


def add_label_coords(dataset):
    """Coordinates `core`, `anvil` (thick and thin anvils share it) and, where the step labels exist, `core_step`,
    `thick_anvil_step`, `thin_anvil_step`: the sorted non-zero labels, int32.  Variables already indexed by one of these
    coordinates are cut down to the labels that remain (the reference's `dataset.sel`) (reference: dataset.py:232-292)."""
    new = {"core": _present_ids(dataset["core_label"]),
           "anvil": _present_ids(dataset["thick_anvil_label"], dataset["thin_anvil_label"])}
    for kind, _ in _KINDS:
        if kind + "_step_label" in dataset:
            new[kind + "_step"] = _present_ids(dataset[kind + "_step_label"])
    for name, values in new.items():
        if name in dataset.coords:
            old = np.asarray(dataset.coords[name])
            pos = np.searchsorted(old, values)
            if np.any(pos >= old.size) or np.any(old[np.minimum(pos, old.size - 1)] != values):
                raise KeyError(f"not all values found in index '{name}'")
            for var, dims in dataset.dims.items():
                if name in dims:
                    dataset[var] = np.take(_host(dataset[var]), pos, axis=dims.index(name))
    dataset.coords.update(new)
    return dataset


def _best_partner(a, b, index, atol=0):
    """for every id in `index`: the b-label with the largest pair count among the pixels where a == id (b > 0 only),
    the smallest such label on ties, 0 if there is none or its count is below atol"""
    ia, ib, cnt = _label.pair_counts(a, b)
    out = np.zeros(len(index), np.int64)
    if ia.size:
        # pairs are sorted by (a, b): a stable sort by descending count inside each a keeps the smallest b first
        order = np.lexsort((ib, -cnt, ia))
        first = np.ones(order.size, bool)
        first[1:] = ia[order][1:] != ia[order][:-1]
        top_a, top_b, top_c = ia[order][first], ib[order][first], cnt[order][first]
        pos = np.searchsorted(top_a, index)
        ok = (pos < top_a.size)
        ok[ok] = top_a[pos[ok]] == np.asarray(index)[ok]
        sel = pos[ok]
        out[ok] = np.where(top_c[sel] >= atol, top_b[sel], 0)
    return out


def find_max_overlap(x, atol, max_label):
    """(reference: dataset.py:294-301; the per-label callback, kept for API parity)"""
    overlap_counts = np.bincount(x, minlength=max_label + 1)
    overlap_counts[0] = 0
    wh_overlap = np.argmax(overlap_counts)
    return wh_overlap if overlap_counts[wh_overlap] >= atol else 0


def link_cores_and_anvils(dataset, atol: int = 5, add_cores_to_anvils: bool = True):
    """`core_anvil_index` (core,): the thick anvil a core overlaps most (>= atol pixels, else 0); with
    add_cores_to_anvils the core's pixels are written into both anvil volumes under that anvil's label;
    `anvil_core_count` (anvil,) (reference: dataset.py:303-366)."""
    t = _lib.torch()
    core, anvil = np.asarray(dataset.coords["core"]), np.asarray(dataset.coords["anvil"])
    core_dev = _lib.to_dev(dataset["core_label"], t.int32)
    index = _best_partner(core_dev, dataset["thick_anvil_label"], core, atol)
    dataset.add("core_anvil_index", index, ("core",), np.int32)
    if add_cores_to_anvils and core.size:
        top = max(int(core.max()), int(core_dev.max()), index.size)
        lut = np.zeros(top + 1, np.int32)
        lut[core] = index
        remapped = _apply_lut(core_dev, lut)
        wh = remapped != 0
        for name in ("thick_anvil_label", "thin_anvil_label"):
            src = dataset[name]
            merged = t.where(wh, remapped.to(_lib.to_dev(src).dtype), _lib.to_dev(src))
            if _lib.is_tensor(src):
                src.copy_(merged)
            else:
                src[...] = merged.cpu().numpy()
    counts = np.bincount(index[index > 0], minlength=int(anvil.max()) + 1 if anvil.size else 1)
    dataset.add("anvil_core_count", counts[anvil] if anvil.size else np.zeros(0), ("anvil",), np.int32)


def link_step_labels(dataset):
    """`core_step_core_index`, `thick_anvil_step_anvil_index`, `thin_anvil_step_anvil_index`: for every step label the
    mode of the parent labels under it, background excluded (reference: dataset.py:369-457, stats_utils.py:11-20)."""
    for kind, parent, name in (("core", "core_label", "core_step_core_index"),
                               ("thick_anvil", "thick_anvil_label", "thick_anvil_step_anvil_index"),
                               ("thin_anvil", "thin_anvil_label", "thin_anvil_step_anvil_index")):
        index = np.asarray(dataset.coords[kind + "_step"])
        dataset.add(name, _best_partner(dataset[kind + "_step_label"], dataset[parent], index), (kind + "_step",), np.int32)


def _flags(label_dim, ids):
    ids = np.asarray(ids)
    ids = ids[ids != 0] if ids.size and ids[0] == 0 else ids
    label_dim = np.asarray(label_dim)
    pos = np.searchsorted(label_dim, ids)
    if np.any(pos >= label_dim.size) or np.any(label_dim[np.minimum(pos, max(label_dim.size - 1, 0))] != ids):
        raise KeyError("label not found in the label coordinate")
    flag = np.zeros(label_dim.size, bool)
    flag[pos] = True
    return flag


def _unique_of(*pieces):
    return np.unique(np.concatenate([_host(p).ravel() for p in pieces]))


def find_edge_labels(labels, label_dim, t=None, start_date=None, end_date=None, max_time_gap=900):
    """Flags over `label_dim`: labels touching the sides of the domain; labels present at the start (first frame, or all
    frames up to `start_date` when the volume begins before it) and, with the reference's own pairing, before a time
    gap; labels present at the end (last frame / frames from `end_date` on) and after a gap.  `t`: datetime64
    coordinate of the frames (reference: dataset.py:460-517)."""
    edge = _unique_of(labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1])
    t = None if t is None else np.asarray(t)
    if start_date is not None and t is not None and t[0] < np.datetime64(start_date):
        start = _unique_of(labels[: int(np.searchsorted(t, np.datetime64(start_date), side="right"))])
    else:
        start = _unique_of(labels[0])
    if end_date is not None and t is not None and t[-1] > np.datetime64(end_date):
        end = _unique_of(labels[int(np.searchsorted(t, np.datetime64(end_date), side="left")):])
    else:
        end = _unique_of(labels[-1])
    if t is not None and t.size > 1:
        gaps = np.where(np.diff(t).astype("timedelta64[ns]").astype(np.int64) / 1e9 > max_time_gap)[0]
        if gaps.size:
            start = _unique_of(start, *[labels[int(g)] for g in gaps])
            end = _unique_of(end, *[labels[int(g) + 1] for g in gaps])
    return _flags(label_dim, edge), _flags(label_dim, start), _flags(label_dim, end)


def flag_edge_labels(dataset, start_date=None, end_date=None, max_time_gap=900):
    """`{core,thick_anvil,thin_anvil}_{edge,start,end}_label_flag` (reference: dataset.py:520-640)."""
    for kind, dim in _KINDS:
        e, s, n = find_edge_labels(dataset[kind + "_label"], dataset.coords[dim], dataset.coords.get("t"),
                                   start_date, end_date, max_time_gap)
        dataset.add(kind + "_edge_label_flag", e, (dim,), bool)
        dataset.add(kind + "_start_label_flag", s, (dim,), bool)
        dataset.add(kind + "_end_label_flag", n, (dim,), bool)


def flag_nan_adjacent_labels(dataset, da):
    """`core_nan_flag`, `thick_anvil_nan_flag`, `thin_anvil_nan_flag`: labels with a pixel within one pixel (3 x 3 x 3
    box) of a missing value of `da` (reference: dataset.py:643-702)."""
    from tobac_flow_amd import ndimage_dev
    t = _lib.torch()
    nan = t.isnan(_lib.to_dev(da, t.float32) if not _lib.is_tensor(da) else da)
    near = None
    if bool(nan.any()):
        near = ndimage_dev.binary_dilation(nan, structure=np.ones((3, 3, 3), bool)).to(t.int32)
    for kind, dim in _KINDS:
        ids = np.zeros(0, np.int64)
        if near is not None:
            ids = np.unique(_label.pair_counts(dataset[kind + "_label"], near)[0])
        dataset.add(kind + "_nan_flag", _flags(dataset.coords[dim], ids), (dim,), bool)


def _group_heads(order, parent_sorted, parents):
    """position (in the step arrays) of the first entry of every parent's group in `order`; ValueError for a parent
    without a group, as the reference's argmax / nanmin of an empty selection raises"""
    parents = np.asarray(parents)
    head = np.ones(order.size, bool)
    head[1:] = parent_sorted[1:] != parent_sorted[:-1]
    group_parent, group_first = parent_sorted[head], order[head]
    pos = np.searchsorted(group_parent, parents)
    ok = pos < group_parent.size
    ok[ok] = group_parent[pos[ok]] == parents[ok]
    if not np.all(ok):
        raise ValueError(f"attempt to reduce over an empty sequence: label {int(parents[~ok][0])} has no step")
    return group_first[pos]


def _first_max_step(step_ids, step_parent, step_area, parents):
    """For every id in `parents`: the position in the step arrays of its step of maximal area, chosen as
    `step[parent == i][np.argmax(area[parent == i])]` chooses on an ascending step coordinate (dataset.py:771-778): a NaN
    area wins, the one with the smallest step id first; otherwise the smallest step id among the maxima."""
    step_ids, step_parent = np.asarray(step_ids), np.asarray(step_parent)
    area = np.asarray(step_area, np.float64)
    nan = np.isnan(area)
    order = np.lexsort((step_ids, -np.where(nan, 0.0, area), ~nan, step_parent))
    return _group_heads(order, step_parent[order], parents)


def _first_step(step_ids, step_parent, parents):
    """For every id in `parents`: the position of its step with the smallest step id (dataset.py:1334-1339)."""
    step_ids, step_parent = np.asarray(step_ids), np.asarray(step_parent)
    order = np.lexsort((step_ids, step_parent))
    return _group_heads(order, step_parent[order], parents)


def _props_inputs(dataset):
    """the operands of calculate_label_properties, checked before anything touches the device"""
    def need(container, name):
        if name not in container:
            raise KeyError(name)
        return container[name]

    area = np.asarray(need(dataset, "area"))
    lat, lon = np.asarray(need(dataset, "lat")), np.asarray(need(dataset, "lon"))
    x, y, t = (np.asarray(need(dataset.coords, c)) for c in ("x", "y", "t"))
    for kind, dim in _KINDS:
        need(dataset, kind + "_label")
        need(dataset, kind + "_step_label")
        need(dataset.coords, dim)
        need(dataset.coords, kind + "_step")
    need(dataset, "core_step_core_index")
    if lat.ndim == 1 and lon.ndim == 1:
        lon, lat = np.meshgrid(lon, lat)                          # dataset.py:1256-1259
    elif not (lat.ndim == 2 and lon.ndim == 2):
        raise ValueError(f"lat and lon must both be 2-D or both 1-D (got {lat.ndim}-D and {lon.ndim}-D)")
    shape = (y.size, x.size)
    for name, a in (("area", area), ("lat", lat), ("lon", lon)):
        if a.shape != shape:
            raise ValueError(f"{name} has shape {a.shape}, expected (y, x) = {shape}")
    t = t.astype("datetime64[ns]")
    if np.any(np.isnat(t)):
        raise ValueError("calculate_label_properties: the t coordinate holds NaT")
    return area, lat, lon, x, y, t


def calculate_label_properties(dataset):
    """Pixel counts, areas, start / end times, lifetimes and area-weighted locations of the cores, anvils and their steps
    (reference: dataset.py:705-1595; the variables it has commented out stay out).  Names, dimensions and dtypes are the
    reference's.  Each of the six label volumes is read ONCE by tf_label_props, with `area`, `lat`, `lon` as (y, x) planes
    and `x`, `y`, `t` as vectors -- the reference's np.repeat stacks are never built; the per-core choices among the steps
    (`core_max_area*`, `core_start_*`) are small host reductions over the step arrays.  Counts and times are exact; areas
    and locations are double sums (the reference sums in the operands' own precision) cast to float32.
    `t` need not be sorted.  A coordinate id that does not occur in its volume gets count 0, area NaN, times NaT and
    location NaN; a region whose areas sum to exactly 0 raises ZeroDivisionError as np.average does."""
    area, lat, lon, x, y, t = _props_inputs(dataset)
    t_sorted, t_rank = np.unique(t, return_inverse=True)
    nat = np.datetime64("NaT", "ns")
    tt = _lib.torch()
    # the operands go to the device once, not once per volume
    area, lat, lon, x, y = (_lib.to_dev(np.ascontiguousarray(a, np.float64), tt.float64, share=True) for a in (area, lat, lon, x, y))
    t_rank = _lib.to_dev(np.ascontiguousarray(t_rank.reshape(-1), np.int32), tt.int32)

    def props(volume, ids, locations):
        ids = np.asarray(ids)
        n = int(ids.max()) if ids.size else 0
        loc = dict(x=x, y=y, lat=lat, lon=lon) if locations else {}
        return _label.label_props(dataset[volume], n, area=area, t_rank=t_rank, **loc)[ids]

    def times(rec, which):
        present = rec["count"] > 0
        out = np.full(rec.size, nat)
        out[present] = t_sorted[rec[which][present]]
        return out

    def areas(rec):
        return np.where(rec["count"] > 0, rec["area_nansum"], np.nan).astype(np.float32)

    def location(rec, key):
        present = rec["count"] > 0
        if np.any(present & (rec["w"] == 0)):
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        out = np.full(rec.size, np.nan)
        out[present] = rec[key][present] / rec["w"][present]
        return out.astype(np.float32)

    step, parent = {}, {}
    for kind, dim in _KINDS:
        parent[kind] = props(kind + "_label", dataset.coords[dim], False)
        step[kind] = props(kind + "_step_label", dataset.coords[kind + "_step"], True)

    def add_steps(kind, what):
        rec, d = step[kind], (kind + "_step",)
        if what == "area":
            dataset.add(kind + "_step_pixel_count", rec["count"], d, np.int32)
            dataset.add(kind + "_step_area", areas(rec), d, np.float32)
        elif what == "t":
            dataset.add(kind + "_step_t", times(rec, "tmin"), d, "datetime64[ns]")
        else:
            for c in ("x", "y", "lat", "lon"):
                dataset.add(f"{kind}_step_{c}", location(rec, "w" + c), d, np.float32)

    def add_times(kind, dim):
        rec = parent[kind]
        start, end = times(rec, "tmin"), times(rec, "tmax")
        dataset.add(kind + "_start_t", start, (dim,), "datetime64[ns]")
        dataset.add(kind + "_end_t", end, (dim,), "datetime64[ns]")
        dataset.add(kind + "_lifetime", end - start, (dim,), "timedelta64[ns]")

    # the reference's order of creation: core, thick anvil, thin anvil (areas, then times), then the locations
    core = np.asarray(dataset.coords["core"])
    dataset.add("core_pixel_count", parent["core"]["count"], ("core",), np.int32)
    dataset.add("core_total_area", areas(parent["core"]), ("core",), np.float32)
    add_steps("core", "area")
    widest = _first_max_step(dataset.coords["core_step"], _host(dataset["core_step_core_index"]), dataset["core_step_area"], core)
    dataset.add("core_max_area", dataset["core_step_area"][widest], ("core",), np.float32)
    add_times("core", "core")
    add_steps("core", "t")
    dataset.add("core_max_area_t", dataset["core_step_t"][widest], ("core",), "datetime64[ns]")
    for kind in ("thick_anvil", "thin_anvil"):
        if kind == "thick_anvil":
            dataset.add("thick_anvil_total_area", areas(parent[kind]), ("anvil",), np.float32)
        add_steps(kind, "area")
        add_times(kind, "anvil")
        add_steps(kind, "t")
    add_steps("core", "loc")
    first = _first_step(dataset.coords["core_step"], _host(dataset["core_step_core_index"]), core)
    for c in ("x", "y", "lat", "lon"):
        dataset.add(f"core_start_{c}", dataset[f"core_step_{c}"][first], ("core",), np.float32)
    add_steps("thick_anvil", "loc")
    add_steps("thin_anvil", "loc")


_FIELD_STATS = ("mean", "std", "median", "max", "min")


def _host_field_stats(a, over):
    """the five statistics as the reference computes them on the host: get_bulk_stats' own NumPy calls (dataset.py:19-60);
    xarray's float defaults skipna=True, ddof=0 -- NumPy's nan-functions over the named axes -- for the other two"""
    if over == "all":
        return np.nanmean(a), np.nanstd(a), np.median(a), np.nanmax(a), np.nanmin(a)
    if a.ndim != 3:
        raise ValueError(f"the field must be a (t, y, x) volume, not {a.shape}")
    axis = (1, 2) if over == "frame" else 0
    return tuple(f(a, axis) for f in (np.nanmean, np.nanstd, np.nanmedian, np.nanmax, np.nanmin))


def _field_stats(da, ds, name, over, infix, dims):
    from tobac_flow_amd import ndimage_dev
    if isinstance(da, str):
        name = da if name is None else name
        da = ds[da]
    if ds is not None and name is None:
        raise ValueError("an array passed with ds needs name= (there is no DataArray.name here)")
    if _lib.is_tensor(getattr(da, "data", None)):                 # a detection.DeviceField
        da = da.data
    if _lib.is_tensor(da):
        got = ndimage_dev.field_stats(da, over)
        out = tuple(got[k].to(da.dtype) for k in _FIELD_STATS)
    else:
        a = np.asarray(da)
        out = tuple(np.asarray(v).astype(a.dtype) for v in _host_field_stats(a, over))
    if ds is not None:
        for k, v in zip(_FIELD_STATS, out):
            ds.add(f"{name}_{infix}{k}", v, dims)
    return out


def get_bulk_stats(da, ds=None, name=None):
    """(mean, std, median, max, min) of a field over everything, each of shape () and of the field's dtype: np.nanmean,
    np.nanstd, np.median (NaN if any value is NaN), np.nanmax, np.nanmin (reference: dataset.py:19-60).  `da`: a NumPy
    array, a device tensor, a detection.DeviceField, or the name of a variable of `ds`; with `ds` (a LabelDataset) the five
    are also added as `{name}_mean`, `_std`, `_median`, `_max`, `_min` (an array then needs name=).  NumPy in, NumPy out
    through the reference's own calls; a float32 / float64 tensor of any shape stays on the GPU
    (ndimage_dev.field_stats: count, median, max and min exact, mean and std float64 sums rounded to the field's dtype)."""
    return _field_stats(da, ds, name, "all", "", ())


def get_spatial_stats(da, ds=None, name=None):
    """The same five per frame of a (t, y, x) field, NaN values ignored (nanmedian), each of shape (t,):
    `{name}_spatial_mean`, ... on ("t",) (reference: dataset.py:63-104).  A frame without a value gives NaN."""
    return _field_stats(da, ds, name, "frame", "spatial_", ("t",))


def get_temporal_stats(da, ds=None, name=None):
    """The same five per pixel along t of a (t, y, x) field, NaN values ignored, each of shape (y, x):
    `{name}_temporal_mean`, ... on ("y", "x") (reference: dataset.py:107-148).  A pixel without a value gives NaN."""
    return _field_stats(da, ds, name, "time", "temporal_", ("y", "x"))


__all__ = ("LabelDataset", "get_bulk_stats", "get_spatial_stats", "get_temporal_stats", "add_step_labels", "add_label_coords", "find_max_overlap", "link_cores_and_anvils",
           "link_step_labels", "find_edge_labels", "flag_edge_labels", "flag_nan_adjacent_labels",
           "calculate_label_properties")
