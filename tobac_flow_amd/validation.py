"""Validation of detected cores and anvils against gridded GLM lightning flashes: distances between flashes and markers,
probability of detection (POD) and false-alarm ratio (FAR).  Mirrors tobac_flow/validation.py -- get_min_dist_for_objects,
get_marker_distance, get_marker_distance_cylinder, validate_markers, get_edge_filter, with the reference's arguments and
defaults -- as scripts/dcc_validation.py:145-250 calls them.

The reference runs scipy.ndimage.distance_transform_edt on the CPU for every frame of every volume, six times per file.
Here the per-frame transform is exact integer arithmetic on the GPU (tf_edt2d_frames), the minimum over the time margin
and the one square root follow in tf_edt_cylinder, and the two np.nanmin-per-label calls are tf_label_nanmin.  Distances,
flags, POD, FAR and counts therefore EQUAL the reference's, bit for bit.  The closest marker is not unique where several
markers are equally near: the reference reports whichever SciPy's sweep meets, this module the one the scan order of
ndimage_dev.edt_squared_frames yields (smallest column distance, then the left one, then the upper one; the earliest
frame of the time margin, as np.nanargmin) -- always a marker at exactly the minimal distance, the same in every run.

NumPy in gives NumPy out with the reference's dtypes (float64 distances, int64 closest markers, bool flags); device
tensors in give device tensors out.  Divergences: per-label results are always one-dimensional (the reference squeezes a
single id to a scalar), an id < 1 in `coord` / `index` is a ValueError (the reference evaluates the background as a
region), and a negative `time_margin` is a ValueError (the reference fails inside np.nanargmin).

The stage itself is validate_detection -- scripts/dcc_validation.py:93-250 without its files -- over the reference's five
validate_* wrappers, which store what validate_markers returns in a dataset.LabelDataset (there is no xarray here).  What a
marker set needs per flash is evaluated at the flashes only: flash_list() turns the grid into the list of flash voxels once
for all five sets (tf_flash_count, tf_flash_list), tf_edt_cylinder_at reads the per-frame transform at those voxels, and no
distance volume is written.  get_edge_filter_dev is get_edge_filter on the device (tf_edge_filter), the missing-data
dilation included.  get_marker_distance_ellipse keeps refusing; the anisotropic 3-D transform it stands for is
get_marker_distance_ellipse_dev: exact in the plane, SciPy's own float64 expression along t, equal to the reference
wherever the nearest marker is unique."""
import numpy as np

from tobac_flow_amd.postprocess import _check_index, _is_tensor, _lib, _shape


def _volume_shape(x, what):
    shape = _shape(x)
    if len(shape) != 3 or 0 in shape:
        raise ValueError(f"{what} must be a non-empty (T, H, W) volume, got shape {shape}")
    return shape


def _same_shape(shape, **others):
    for name, x in others.items():
        if _shape(x) != shape:
            raise ValueError(f"{name} {_shape(x)} does not have the same shape as the labels {shape}")


def _time_margin(time_margin):
    tm = int(time_margin)
    if tm != time_margin or tm < 0:
        raise ValueError("time_margin must be a non-negative integer")
    return tm


def _out(x, like):
    """a device result in the container of the input `like`: a tensor stays, a numpy input gets a numpy array"""
    if _is_tensor(like):
        return x
    return _lib().to_host(x) if x.numel() else x.cpu().numpy()


def _cylinder(markers, tm, get_closest):
    """(float64 distances, int64 closest markers or None) as device tensors"""
    from tobac_flow_amd import ndimage_dev
    lib = _lib()
    t = lib.torch()
    dev = lib.to_dev(markers, share=True)
    d2, nearest = ndimage_dev.edt_squared_frames(dev, return_nearest=get_closest)
    dist, src = ndimage_dev.edt_cylinder(d2, nearest, tm)
    if not get_closest:
        return dist, None
    values = dev.reshape(-1)[src.reshape(-1).clamp(min=0)].to(t.int64).reshape(src.shape)
    return dist, t.where(src < 0, t.zeros_like(values), values)


def get_marker_distance_cylinder(markers, time_margin, get_closest=False):
    """For every voxel of the (T, H, W) volume `markers`: the distance within its own frame plane to the nearest marker
    (voxel != 0) of the frames t - time_margin .. t + time_margin, inf where none of them holds a marker; with
    `get_closest` also the value of that marker, 0 where there is none -- `distances` or `(distances, closest_markers)`,
    float64 and int64 (reference: validation.py:52-104).  Of equal distances in several frames the earliest frame is
    taken; see the module docstring for equally near markers within a frame."""
    _volume_shape(markers, "markers")
    tm = _time_margin(time_margin)
    dist, closest = _cylinder(markers, tm, bool(get_closest))
    return (_out(dist, markers), _out(closest, markers)) if get_closest else _out(dist, markers)


def get_marker_distance(labels, time_range=1):
    """The per-frame distance to the nearest label (inf in a frame without one), then for i = 1 .. time_range the
    reference's two statements `d[i:] = fmin(d[:-i], d[i:])`, `d[:-i] = fmin(d[:-i], d[i:])` in their order -- which is
    not a plain +- time_range window (reference: validation.py:24-36).  float64."""
    _volume_shape(labels, "labels")
    t = _lib().torch()
    d = _cylinder(labels, 0, False)[0]
    for i in range(1, int(time_range) + 1):
        d[i:] = t.fmin(d[:-i], d[i:])
        d[:-i] = t.fmin(d[:-i], d[i:])
    return _out(d, labels)


def get_marker_distance_ellipse(markers, time_margin, margin):
    """Not taken from the reference (validation.py:39-49): scripts/dcc_validation.py never calls it, and its anisotropic
    three-dimensional squared distance (sampling = margin / time_margin along t) is no integer, so the exactness contract
    of this module does not extend to it."""
    raise NotImplementedError("get_marker_distance_ellipse: the anisotropic 3-D transform is not integer-exact and the "
                              "validation script never calls it; use get_marker_distance_cylinder")


def get_marker_distance_ellipse_dev(markers, time_margin, margin):
    """The reference's get_marker_distance_ellipse (validation.py:39-49) on the GPU: for every voxel of the (T, H, W) volume
    `markers` the distance to the nearest marker (voxel != 0) where one frame counts as `margin / time_margin` pixels --
    scipy.ndimage.distance_transform_edt(markers == 0, sampling=(margin / time_margin, 1, 1)) -- and the value of that
    marker: `(distances, closest_marker)`, float64 and the dtype of `markers`.  The per-frame integer transform
    (tf_edt2d_frames) is followed by its lower envelope along t (tf_edt_time_envelope); the distance is SciPy's own
    expression for the reported marker, so it equals the reference's bit for bit wherever the nearest marker is unique
    (DESIGN.md).  Of equally near markers the one in the nearer frame is taken, then the earlier frame, and within a frame
    the one ndimage_dev.edt_squared_frames reports.  A volume without any marker gives inf and 0 (the reference's result
    for it is meaningless).  `margin / time_margin` is evaluated as written; a result that is not finite and > 0 is a
    ValueError."""
    sampling = margin / time_margin
    if not (np.isfinite(sampling) and sampling > 0):
        raise ValueError(f"margin / time_margin must be finite and > 0, got {sampling!r}")
    _volume_shape(markers, "markers")
    from tobac_flow_amd import ndimage_dev
    lib = _lib()
    t = lib.torch()
    dev = lib.to_dev(markers, share=True)
    d2, nearest = ndimage_dev.edt_squared_frames(dev, return_nearest=True)
    dist, src = ndimage_dev.edt_time_envelope(d2, nearest, float(sampling))
    values = dev.reshape(-1)[src.reshape(-1).clamp(min=0)].reshape(src.shape)
    closest = t.where(src < 0, t.zeros_like(values), values)
    return _out(dist, markers), _out(closest, markers)


def _label_ids(labels, index):
    if index is None:
        top = int(labels.max()) if 0 not in _shape(labels) else 0
        return np.arange(1, max(top, 0) + 1, dtype=np.int64)
    return _check_index(index)


def _label_nanmin(labels, field, ids):
    """(float64 minima, missing) over the device: NaN where all of a label's values are NaN; missing = no voxel at all"""
    from tobac_flow_amd import ndimage_dev
    lib = _lib()
    lab = lib.to_dev(labels, lib.torch().int32, share=True)
    mins, counts = ndimage_dev.label_nanmin(lab, lib.to_dev(field, share=True), ids)
    return mins, counts < 0


def get_min_dist_for_objects(distance_array, labels, index=None):
    """np.nanmin of `distance_array` over every label id in `index` (default 1 .. labels.max()), NaN for an id without
    voxels (reference: validation.py:13-21).  float64."""
    shape = _shape(labels)
    _same_shape(shape, distance_array=distance_array)
    ids = _label_ids(labels, index)
    if not ids.size or 0 in shape:
        nothing = np.full(ids.size, np.nan)
        return _lib().to_dev(nothing) if _is_tensor(labels) else nothing
    mins, _ = _label_nanmin(labels, distance_array, ids)        # an id without voxels is NaN already: the default
    return _out(mins, labels)


def _refuse_bad_counts(glm_grid):
    """np.repeat's own refusal of a negative count, up front, for a NumPy grid (NaN casts to a negative one); a device grid
    is checked by tf_flash_count"""
    g = np.asarray(glm_grid)
    if np.any(g < 0) or (g.dtype.kind == "f" and np.isnan(g).any()):
        raise ValueError("repeats may not contain negative values (glm_grid holds a negative or NaN flash count)")


class FlashList:
    """The flashes of a grid as a list: `voxel` (int64 device tensor), the raveled voxel of every flash in the order of
    np.repeat(np.arange(n), glm_grid.astype(int).ravel()); `shape`, the grid's; len() = the number of flashes.  Built once
    by flash_list() and shared by every marker set validated against the same grid."""

    def __init__(self, voxel, shape):
        self.voxel, self.shape, self.n = voxel, tuple(shape), int(voxel.shape[0])

    def __len__(self):
        return self.n


def _list_flashes(glm_grid):
    from tobac_flow_amd import ndimage_dev
    return FlashList(ndimage_dev.flash_list(_lib().to_dev(glm_grid, share=True)), _shape(glm_grid))


def flash_list(glm_grid):
    """The FlashList of a flash-count grid (NumPy array or device tensor; a count is truncated toward zero, a negative or
    NaN one raises ValueError as np.repeat does, and so does one of 2^31 or more).  One pass over the grid and one over the
    tiles that hold a flash (tf_flash_count, tf_flash_list); the total crosses to the host once."""
    if not _is_tensor(glm_grid):
        _refuse_bad_counts(glm_grid)                             # the refusal needs no device
    return _list_flashes(glm_grid)


def _check_operands(labels, glm_grid, glm_distance, edge_filter, time_margin):
    """(shape, time margin) of one marker set's operands; the ValueErrors of validate_markers, in its order"""
    shape = _volume_shape(labels, "labels")
    _same_shape(shape, glm_grid=glm_grid, glm_distance=glm_distance, edge_filter=edge_filter)
    return shape, _time_margin(time_margin)


def _cylinder_at(markers, tm, get_closest, flashes, margin):
    """(float64 distances, int64 closest markers or None, int64 device scalar: flashes within margin) at the flashes"""
    from tobac_flow_amd import ndimage_dev
    lib = _lib()
    t = lib.torch()
    dev = lib.to_dev(markers, share=True)
    d2, nearest = ndimage_dev.edt_squared_frames(dev, return_nearest=get_closest)
    values = None
    if get_closest:                                               # the value at the feature, as .astype(int) truncates it
        values = dev if dev.dtype == t.int32 else (dev.to(t.int64) if dev.is_floating_point() else dev).to(t.int32)
    return ndimage_dev.edt_cylinder_at(d2, nearest, values, tm, flashes.voxel, margin, get_closest)


def validate_markers(labels, glm_grid, glm_distance, edge_filter, n_glm_in_margin, coord=None, margin=10, time_margin=3,
                     get_closest=False, flashes=None):
    """Validation results for one set of markers (reference: validation.py:107-170).  Returns the reference's tuple

        flash_distance_to_marker   float64, one entry per flash: the cylinder distance of `labels` at the flash's voxel
        flash_closest_marker       int64, the closest label per flash, or None without `get_closest`
        marker_distance_to_flash   float64 per id of `coord`: the smallest `glm_distance` under the label, NaN if absent
        pod                        flashes within `margin` of a label / n_glm_in_margin (NaN where that is not > 0)
        far                        labels inside the edge margin whose distance to a flash is > margin / their number
        n_marker_in_margin         number of labels inside the edge margin
        margin_flag                bool per id: the label lies inside `edge_filter` throughout (False if absent)

    `glm_grid` holds the flash count per voxel; a negative or NaN count raises ValueError, as np.repeat does.  `coord`
    defaults to 1 .. labels.max().  The per-flash results are evaluated at the flashes only (tf_edt_cylinder_at over the
    list of flash_list()): no distance volume is built.  `flashes`: the flash_list() of `glm_grid`, to share one list over
    several marker sets; without it the list is built here."""
    shape, tm = _check_operands(labels, glm_grid, glm_distance, edge_filter, time_margin)
    if flashes is not None:
        if flashes.shape != shape:
            raise ValueError(f"flashes {flashes.shape} were not listed from a grid of the labels' shape {shape}")
    elif _is_tensor(glm_grid):
        flashes = _list_flashes(glm_grid)                        # a device grid's counts are judged on the device, as ever
    else:
        _refuse_bad_counts(glm_grid)
    ids = _label_ids(labels, coord)                              # the last check: nothing of a NumPy call has touched the device yet
    if flashes is None:
        flashes = _list_flashes(glm_grid)
    lib = _lib()
    t = lib.torch()
    flash_distance, flash_closest, n_within = _cylinder_at(labels, tm, bool(get_closest), flashes, margin)
    pod = float(int(n_within)) / n_glm_in_margin if n_glm_in_margin > 0 else np.nan
    if ids.size:
        inside, missing = _label_nanmin(labels, edge_filter, ids)
        margin_flag = (inside != 0) & ~missing                  # NaN != 0, as NaN.astype(bool); an absent id: default False
        marker_distance = _label_nanmin(labels, glm_distance, ids)[0]
    else:
        margin_flag = t.zeros(0, dtype=t.bool, device=flash_distance.device)
        marker_distance = t.zeros(0, dtype=t.float64, device=flash_distance.device)
    n_marker_in_margin = int(margin_flag.sum())
    far = float((marker_distance[margin_flag] > margin).sum()) / n_marker_in_margin if n_marker_in_margin > 0 else np.nan
    if not _is_tensor(labels):
        pod, far, n_marker_in_margin = np.float64(pod), np.float64(far), np.int64(n_marker_in_margin)
    return (_out(flash_distance, labels), _out(flash_closest, labels) if get_closest else None, _out(marker_distance, labels),
            pod, far, n_marker_in_margin, _out(margin_flag, labels))


def _member(ds, name):
    return ds[name] if isinstance(ds, dict) or not hasattr(ds, name) else getattr(ds, name)


def get_edge_filter(gridded_flash_ds, margin, time_margin):
    """Boolean (T, H, W) array, False within `time_margin` frames of the ends and of a time gap > 900 s, within `margin`
    pixels of the borders, and around missing GLM data (glm_flashes == -1) -- host NumPy, statement for statement the
    reference's (validation.py:173-219), including SciPy's binary_dilation with the reference's disc of radius `margin`
    around its hard-coded centre 10 in the rare missing-data branch.  `gridded_flash_ds` is any object or mapping with
    `glm_flashes` (T, H, W) and `t` (datetime64[ns] or nanoseconds)."""
    import scipy.ndimage as ndi
    lib = _lib()
    glm_flashes = _member(gridded_flash_ds, "glm_flashes")
    glm_flashes = lib.to_host(glm_flashes) if _is_tensor(glm_flashes) else np.asarray(glm_flashes)
    times = np.asarray(_member(gridded_flash_ds, "t"))
    edge_filter_array = np.full(glm_flashes.shape, 1).astype("bool")

    edge_filter_array[:time_margin] = False
    edge_filter_array[-time_margin:] = False
    edge_filter_array[:, :margin] = False
    edge_filter_array[:, -margin:] = False
    edge_filter_array[:, :, :margin] = False
    edge_filter_array[:, :, -margin:] = False

    time_gap = np.where((np.diff(times) / 1e9).astype(int) > 900)[0]
    for i in time_gap:
        i_slice = slice(np.maximum(i - time_margin + 1, 0), np.minimum(i + time_margin + 2, times.size))
        edge_filter_array[i_slice] = False

    if np.any(glm_flashes == -1):
        margin_structure = np.stack(
            [np.sum([(arr - 10) ** 2 for arr in np.meshgrid(np.arange(margin * 2 + 1), np.arange(margin * 2 + 1))], 0) ** 0.5
             < margin] * (time_margin * 2 + 1), 0)
        edge_filter_array[ndi.binary_dilation(glm_flashes == -1, structure=margin_structure)] = False
    return edge_filter_array


def get_edge_filter_dev(gridded_flash_ds, margin, time_margin):
    """get_edge_filter on the GPU: a device bool tensor equal to its array, for `glm_flashes` as a device tensor (a NumPy
    array is uploaded).  The frames around a time gap are T numbers and are marked on the host from `t`, by get_edge_filter's
    own statements; everything per voxel is tf_edge_filter, the missing-data dilation included -- for every margin, not
    only the reference's 10 -- and skipped after one read of the grid where it holds no -1."""
    from tobac_flow_amd import ndimage_dev
    margin, time_margin = int(margin), int(time_margin)
    if margin < 0 or time_margin < 0:
        raise ValueError("margin and time_margin must not be negative")
    glm_flashes = _member(gridded_flash_ds, "glm_flashes")
    _volume_shape(glm_flashes, "glm_flashes")
    times = np.asarray(_member(gridded_flash_ds, "t"))
    frame_off = np.zeros(times.size, bool)
    time_gap = np.where((np.diff(times) / 1e9).astype(int) > 900)[0]
    for i in time_gap:
        frame_off[slice(np.maximum(i - time_margin + 1, 0), np.minimum(i + time_margin + 2, times.size))] = True
    return ndimage_dev.edge_filter(_lib().to_dev(glm_flashes, share=True), margin, time_margin, frame_off)


# ---- the five wrappers of the reference and the script that calls them ---------------------------------------------------
def _host_array(x):
    return _lib().to_host(x) if _is_tensor(x) else np.asarray(x)


def _coords_of(ds):
    """the coordinates of a LabelDataset (`.coords`) or of a mapping that keeps them under "coords"; None if neither"""
    coords = getattr(ds, "coords", None)
    return ds["coords"] if coords is None and "coords" in ds else coords


def _has_coord(ds, name):
    coords = _coords_of(ds)
    return (coords is not None and name in coords) or name in ds


def _coord(ds, name):
    """the coordinate `name` as a host array; a mapping may also keep it beside its variables"""
    coords = _coords_of(ds)
    return _host_array(coords[name] if coords is not None and name in coords else ds[name])


def _keep_labels(labels, keep, top):
    """remapper[labels] with remapper = zeros(top + 1), remapper[keep] = keep (validation.py:342-344), on the device; a
    label above `top` is a ValueError (the reference's remapper raises IndexError)"""
    from tobac_flow_amd.dataset import _apply_lut
    lib = _lib()
    dev = lib.to_dev(labels, lib.torch().int32, share=True)
    if int(dev.max()) > top:
        raise ValueError(f"the label volume holds the label {int(dev.max())}, above the largest id {top} of its coordinate")
    lut = np.zeros(top + 1, np.int32)
    lut[keep] = keep
    out = _apply_lut(dev, lut)
    return out if _is_tensor(labels) else lib.to_host(out)


def _store(validation_ds, name, result):
    """the seven variables one marker set writes (validation.py:262-324 and its four siblings); `name` is also the dim"""
    flash_distance, flash_closest, marker_distance, pod, far, n_in_margin, margin_flag = result
    t = _lib().torch()

    def cast(x, np_dtype, t_dtype):
        return x.to(t_dtype) if _is_tensor(x) else np.asarray(x).astype(np_dtype)

    validation_ds.add(f"flash_{name}_distance", cast(flash_distance, np.float32, t.float32), ("flash",))
    if flash_closest is not None:
        validation_ds.add(f"flash_{name}_index", cast(flash_closest, np.int32, t.int32), ("flash",))
    validation_ds.add(f"{name}_glm_distance", cast(marker_distance, np.float32, t.float32), (name,))
    validation_ds.add(f"{name}_pod", np.asarray(pod, np.float64).astype(np.float32), ())
    validation_ds.add(f"{name}_far", np.asarray(far, np.float64).astype(np.float32), ())
    validation_ds.add(f"{name}_count_in_margin", np.asarray(n_in_margin).astype(np.int32), ())
    validation_ds.add(f"{name}_margin_flag", cast(margin_flag, bool, t.bool), (name,))


def validate_cores(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin, time_margin,
                   get_closest=False, flashes=None):
    """`core_label` over the ids of `core` -> flash_core_distance, flash_core_index (with get_closest), core_glm_distance,
    core_pod, core_far, core_count_in_margin, core_margin_flag (reference: validation.py:222-324).

    For this function and its four siblings: `detection_ds` is a dataset.LabelDataset, or any mapping with the reference's
    variable names and `coords`; `validation_ds` is a LabelDataset, which receives the reference's variables under its
    names, dims and dtypes: float32 distances, POD and FAR, int32 indices and counts, bool flags.  The per-flash and
    per-marker arrays are device tensors where the label volume is one and NumPy arrays otherwise; POD, FAR and the count
    are 0-d NumPy arrays either way.  `flashes`: the flash_list() of `glm_grid`, which validate_detection shares between
    the sets.  Divergences from the reference: where POD or FAR is the plain Python nan the reference's `.astype` raises
    AttributeError, here a float32 NaN is stored; the progress prints are dropped."""
    result = validate_markers(detection_ds["core_label"], glm_grid, glm_distance, edge_filter_array, n_glm_in_margin,
                              coord=_coord(detection_ds, "core"), margin=margin, time_margin=time_margin,
                              get_closest=get_closest, flashes=flashes)
    _store(validation_ds, "core", result)


def validate_cores_with_anvils(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin,
                               time_margin, get_closest=False, flashes=None):
    """The cores with `core_anvil_index != 0`, every other core removed from `core_label` on the device (tf_apply_lut) ->
    the seven `core_with_anvil` variables on the dim `core_with_anvil` (reference: validation.py:327-442; containers and
    divergences as validate_cores).  Further divergences: a label above the largest id of `core` raises ValueError where
    the reference's remapper raises IndexError, and the ids of the subset are also recorded as
    `validation_ds.coords["core_with_anvil"]` (the reference leaves the dim without a coordinate)."""
    _check_operands(detection_ds["core_label"], glm_grid, glm_distance, edge_filter_array, time_margin)    # before the remap's device work
    core = _coord(detection_ds, "core")
    keep = core[_host_array(detection_ds["core_anvil_index"]) != 0]
    labels = _keep_labels(detection_ds["core_label"], keep, int(np.max(core)))
    result = validate_markers(labels, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, coord=keep, margin=margin,
                              time_margin=time_margin, get_closest=get_closest, flashes=flashes)
    _store(validation_ds, "core_with_anvil", result)
    validation_ds.coords["core_with_anvil"] = keep


def validate_anvils(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin, time_margin,
                    get_closest=False, flashes=None):
    """`thick_anvil_label` over the ids of `anvil` -> the seven `anvil` variables (reference: validation.py:445-555;
    containers and divergences as validate_cores)."""
    result = validate_markers(detection_ds["thick_anvil_label"], glm_grid, glm_distance, edge_filter_array, n_glm_in_margin,
                              coord=_coord(detection_ds, "anvil"), margin=margin, time_margin=time_margin,
                              get_closest=get_closest, flashes=flashes)
    _store(validation_ds, "anvil", result)


def validate_anvils_with_cores(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin,
                               time_margin, get_closest=False, flashes=None):
    """The anvils some core points at through `core_anvil_index`, every other anvil removed from `thick_anvil_label` on the
    device (tf_apply_lut) -> the seven `anvil_with_core` variables on the dim `anvil_with_core` (reference:
    validation.py:558-672; containers and divergences as validate_cores).  Further divergences: a label above the largest id
    of `anvil` raises ValueError where the reference's remapper raises IndexError, and the ids of the subset are also
    recorded as `validation_ds.coords["anvil_with_core"]`."""
    _check_operands(detection_ds["thick_anvil_label"], glm_grid, glm_distance, edge_filter_array, time_margin)    # before the remap's device work
    anvil = _coord(detection_ds, "anvil")
    keep = anvil[np.isin(anvil, np.unique(_host_array(detection_ds["core_anvil_index"])))]
    labels = _keep_labels(detection_ds["thick_anvil_label"], keep, int(np.max(anvil)))
    result = validate_markers(labels, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, coord=keep, margin=margin,
                              time_margin=time_margin, get_closest=get_closest, flashes=flashes)
    _store(validation_ds, "anvil_with_core", result)
    validation_ds.coords["anvil_with_core"] = keep


def validate_anvil_markers(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin,
                           time_margin, get_closest=False, flashes=None):
    """`anvil_marker_label` over the ids of `anvil_marker` -> the seven `anvil_marker` variables (reference:
    validation.py:675-785; containers and divergences as validate_cores)."""
    result = validate_markers(detection_ds["anvil_marker_label"], glm_grid, glm_distance, edge_filter_array, n_glm_in_margin,
                              coord=_coord(detection_ds, "anvil_marker"), margin=margin, time_margin=time_margin,
                              get_closest=get_closest, flashes=flashes)
    _store(validation_ds, "anvil_marker", result)


def _present(coord, *volumes):
    """the ids of `coord` that occur in one of the label volumes (np.isin(coord, np.unique(volume))): one read of each
    volume (tf_label_filter without a criterion)"""
    from tobac_flow_amd import ndimage_dev
    lib = _lib()
    mask = np.zeros(coord.size, bool)
    for volume in volumes:
        present = ndimage_dev.label_filter(lib.to_dev(volume, lib.torch().int32, share=True))[2]
        mask |= np.isin(coord, np.flatnonzero(present) + 1)
    return mask


def _cut_to_present(detection_ds):
    """scripts/dcc_validation.py:96-116: `core`, `anvil` and `anvil_marker` cut to the ids present in their volumes, with
    the variables on those dims -- as a shallow copy: the input keeps its coordinates and variables"""
    from tobac_flow_amd.dataset import LabelDataset
    out = LabelDataset({k: v for k, v in detection_ds.items() if k != "coords"})
    out.dims = dict(getattr(detection_ds, "dims", {}))
    out.dims.setdefault("core_anvil_index", ("core",))
    volumes = {"core": ("core_label",), "anvil": ("thick_anvil_label", "thin_anvil_label"), "anvil_marker": ("anvil_marker_label",)}
    for dim, names in volumes.items():
        if not _has_coord(detection_ds, dim):
            continue
        coord = _coord(detection_ds, dim)
        mask = _present(coord, *(out[name] for name in names))
        out.coords[dim] = coord[mask]
        for var, dims in out.dims.items():
            if dim in dims and var in out and not mask.all():
                out[var] = np.compress(mask, _host_array(out[var]), axis=dims.index(dim))
    return out


def validate_detection(detection_ds, gridded_flash_ds, margin=10, time_margin=3, get_closest=False, filename=None):
    """The fourth stage: scripts/dcc_validation.py:93-250 without its file I/O.  `detection_ds`: the detection product (a
    dataset.LabelDataset, or a mapping with the label volumes, `core_anvil_index` and `coords`); `gridded_flash_ds`: an
    object or mapping with `glm_flashes` (T, H, W) on the product's grid and `t`.  With `filename` the padding frames of
    the product are trimmed first (trim_file_start / trim_file_end; a LabelDataset is required then); the flash grid is NOT
    trimmed with it -- the script grids the flashes onto the trimmed product -- so `glm_flashes` and `t` of
    `gridded_flash_ds` must already be on the trimmed frames, and a grid of another shape is a ValueError.  `core`, `anvil` and
    `anvil_marker` are cut to the ids present in their volumes; then flash_count_total, the flash distance
    (get_marker_distance_cylinder), the edge filter (get_edge_filter_dev where the grid is a device tensor,
    get_edge_filter otherwise), flash_count_in_margin, ONE flash list, and the five marker sets -- the anvil markers only
    where that coordinate exists.  Returns the validation LabelDataset with the reference's variables.  The grid is zeroed
    outside the edge filter on a copy: the script mutates the array it was handed, this function does not."""
    from tobac_flow_amd.dataset import LabelDataset
    glm_grid = _member(gridded_flash_ds, "glm_flashes")
    _volume_shape(glm_grid, "glm_flashes")
    tm = _time_margin(time_margin)
    if filename is not None:
        from tobac_flow_amd.utils.datetime_utils import trim_file_end, trim_file_start
        detection_ds = trim_file_start(trim_file_end(detection_ds, filename), filename)
    _same_shape(_volume_shape(detection_ds["core_label"], "core_label"), glm_flashes=glm_grid)
    detection_ds = _cut_to_present(detection_ds)
    validation_ds = LabelDataset()
    glm_distance = get_marker_distance_cylinder(glm_grid, tm)
    if _is_tensor(glm_grid):
        t = _lib().torch()
        total = t.nansum if glm_grid.is_floating_point() else t.sum
        n_glm_total = float(total(glm_grid.clamp(min=0)))        # clamp keeps a NaN, which nansum then skips
        edge_filter_array = get_edge_filter_dev(gridded_flash_ds, margin, tm)
        glm_grid = glm_grid * edge_filter_array if not glm_grid.is_floating_point() else t.where(edge_filter_array, glm_grid, 0.0)
        n_glm_in_margin = float(total(glm_grid))
    else:
        glm_grid = np.asarray(glm_grid)
        n_glm_total = np.nansum(glm_grid[glm_grid > 0])
        edge_filter_array = get_edge_filter(gridded_flash_ds, margin, tm)
        glm_grid = np.where(edge_filter_array, glm_grid, np.zeros((), glm_grid.dtype))
        n_glm_in_margin = np.nansum(glm_grid)
    validation_ds.add("flash_count_total", np.asarray(n_glm_total).astype(np.int32), ())
    validation_ds.add("flash_count_in_margin", np.asarray(n_glm_in_margin).astype(np.int32), ())
    flashes = flash_list(glm_grid)
    sets = [validate_cores, validate_cores_with_anvils, validate_anvils, validate_anvils_with_cores]
    if "anvil_marker" in detection_ds.coords:
        sets.append(validate_anvil_markers)
    for validate in sets:
        validate(detection_ds, validation_ds, glm_grid, glm_distance, edge_filter_array, n_glm_in_margin, margin, tm,
                 get_closest=get_closest, flashes=flashes)
    return validation_ds


__all__ = ("get_min_dist_for_objects", "get_marker_distance", "get_marker_distance_ellipse", "get_marker_distance_cylinder",
           "validate_markers", "get_edge_filter", "get_marker_distance_ellipse_dev", "FlashList", "flash_list",
           "get_edge_filter_dev", "validate_cores", "validate_cores_with_anvils", "validate_anvils",
           "validate_anvils_with_cores", "validate_anvil_markers", "validate_detection")
