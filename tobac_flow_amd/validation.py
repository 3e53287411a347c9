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
region), and a negative `time_margin` is a ValueError (the reference fails inside np.nanargmin).  The validate_*
wrappers of the reference only store what validate_markers returns in an xarray Dataset and are not taken
(there is no xarray here).  get_marker_distance_ellipse keeps refusing; the anisotropic 3-D transform it stands for is
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


def _flash_counts(glm_grid):
    """glm_grid.astype(int) with np.repeat's own refusal of a negative count up front (NaN casts to a negative one)"""
    if _is_tensor(glm_grid):
        t = _lib().torch()
        bad = bool(((glm_grid < 0) | (glm_grid != glm_grid)).any()) if glm_grid.is_floating_point() else bool((glm_grid < 0).any())
        counts = glm_grid.to(t.int64)
    else:
        g = np.asarray(glm_grid)
        bad = bool(np.any(g < 0) or (g.dtype.kind == "f" and np.isnan(g).any()))
        counts = g.astype(np.int64) if not bad else None
    if bad:
        raise ValueError("repeats may not contain negative values (glm_grid holds a negative or NaN flash count)")
    return counts


def validate_markers(labels, glm_grid, glm_distance, edge_filter, n_glm_in_margin, coord=None, margin=10, time_margin=3,
                     get_closest=False):
    """Validation results for one set of markers (reference: validation.py:107-170).  Returns the reference's tuple

        flash_distance_to_marker   float64, one entry per flash: the cylinder distance of `labels` at the flash's voxel
        flash_closest_marker       int64, the closest label per flash, or None without `get_closest`
        marker_distance_to_flash   float64 per id of `coord`: the smallest `glm_distance` under the label, NaN if absent
        pod                        flashes within `margin` of a label / n_glm_in_margin (NaN where that is not > 0)
        far                        labels inside the edge margin whose distance to a flash is > margin / their number
        n_marker_in_margin         number of labels inside the edge margin
        margin_flag                bool per id: the label lies inside `edge_filter` throughout (False if absent)

    `glm_grid` holds the flash count per voxel; a negative or NaN count raises ValueError, as np.repeat does.  `coord`
    defaults to 1 .. labels.max()."""
    shape = _volume_shape(labels, "labels")
    _same_shape(shape, glm_grid=glm_grid, glm_distance=glm_distance, edge_filter=edge_filter)
    tm = _time_margin(time_margin)
    counts = _flash_counts(glm_grid)
    ids = _label_ids(labels, coord)
    lib = _lib()
    t = lib.torch()
    dist, closest = _cylinder(labels, tm, bool(get_closest))
    repeats = lib.to_dev(counts, t.int64).reshape(-1)
    flash_distance = t.repeat_interleave(dist.reshape(-1), repeats)
    flash_closest = t.repeat_interleave(closest.reshape(-1), repeats) if get_closest else None
    pod = float((flash_distance <= margin).sum()) / n_glm_in_margin if n_glm_in_margin > 0 else np.nan
    if ids.size:
        inside, missing = _label_nanmin(labels, edge_filter, ids)
        margin_flag = (inside != 0) & ~missing                  # NaN != 0, as NaN.astype(bool); an absent id: default False
        marker_distance = _label_nanmin(labels, glm_distance, ids)[0]
    else:
        margin_flag = t.zeros(0, dtype=t.bool, device=dist.device)
        marker_distance = t.zeros(0, dtype=t.float64, device=dist.device)
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


__all__ = ("get_min_dist_for_objects", "get_marker_distance", "get_marker_distance_ellipse", "get_marker_distance_cylinder",
           "validate_markers", "get_edge_filter", "get_marker_distance_ellipse_dev")
