"""The second stage of the production chain: window-local products -> one consistent product (mirrors the "new linking
functions" of /root/reference/tobac_flow/linking.py:30-396, the ones scripts/linking_parallel.py, relabel_linked_files.py,
relabel_postprocess_goes.py, relabel_postprocess_seviri_cci.py and linked_statistics_goes.py call).

The reference works on xr.Datasets that it opens by file name.  Here a window product is a dataset.LabelDataset with
`coords["t"]` (datetime64, sorted, unique), `coords["core"]` / `coords["anvil"]` (sorted int32), the (t, y, x) int32 volumes
`core_label`, `thick_anvil_label`, `thin_anvil_label` and optionally `bt`; a file name is a key into a `store` -- a mapping
name -> LabelDataset, or a callable that returns one.  The extra `store` argument is the only change of signature; reading
and writing files stays with the caller.  A product taken from the store is never written to: every function that changes
a product works on a copy of the container with arrays of its own.

Containers: NumPy volumes take host NumPy code that restates the reference; device tensors take the device path and come
back as device tensors; the small per-label arrays (pairs, tables, maps, flags) are always host NumPy.  On the device
find_overlap_between_cores / _anvils are an index_select of the compared frames and parallel.overlap_pairs
(tf_window_overlap_pairs), and relabel_and_merge_file is ONE launch of tf_relabel_merge per volume: the window's ids, and
under its zeros the ids of the frames the previous and the next window share with it, each through its own table, without
the three relabelled copies the composition builds.  tf_relabel_merge checks the ids it consults: an id beyond its map or
a negative one raises ValueError, as the host path does for any such id in the relabelled frames; a neighbour's voxel is
consulted only where the result so far is zero, so a bad id under a voxel that is never consulted goes unnoticed there.

combine_labels: the reference assigns through `ds.core_label.sel(t=...).data = ...`, which in xarray most likely writes
into a temporary and leaves `ds` as it was (xarray is not in this image; nobody has checked).  This module builds the
documented intent -- the zeros of `ds` are filled, as File_Linker.combine_labels does through `.loc` --; the other reading
is `merge=False`, which gives the relabelling alone.

process_file composes dataset.add_label_coords, flag_edge_labels, flag_nan_adjacent_labels, link_cores_and_anvils,
add_step_labels and link_step_labels, which compute on the device whatever the container."""
from functools import partial

import numpy as np

from tobac_flow_amd import _lib
from tobac_flow_amd import dataset as _dataset
from tobac_flow_amd import parallel
from tobac_flow_amd.dataset import LabelDataset
from tobac_flow_amd.parallel import LINK_ATOL, LINK_RTOL
from tobac_flow_amd.utils.datetime_utils import get_dates_from_filename, trim_file_start_and_end
from tobac_flow_amd.utils.label_utils import remap_labels

_VOLUMES = (("core_label", "core"), ("thick_anvil_label", "anvil"), ("thin_anvil_label", "anvil"))
_REQUIRED_VARS = ("goes_imager_projection", "lat", "lon", "area", "bt", "BT", "wvd", "swd", "core_label", "thick_anvil_label",
                  "thin_anvil_label")
_LABEL_COORDS = ("core", "anvil", "core_step", "thick_anvil_step", "thin_anvil_step")


def _open(store, name):
    return store(name) if callable(store) else store[name]


def _coord_max(coord):
    coord = np.asarray(coord)
    return int(coord.max()) if coord.size else 0


def find_overlaps(x, atol, rtol, max_label, label_counts):
    """The labels under one region that the linking rule joins to it: count >= atol (> 0 if atol is 0) and
    max(count / size of the region, count / size of the label) >= rtol; never 0 (reference: linking.py:33-46)."""
    overlap_counts = np.bincount(x, minlength=max_label + 1)
    wh_overlap = overlap_counts >= atol if atol > 0 else overlap_counts > 0
    if rtol > 0:
        wh_overlap = np.logical_and(wh_overlap, np.maximum(overlap_counts / x.size, overlap_counts / label_counts) >= rtol)
    wh_overlap[0] = False
    return np.where(wh_overlap)[0]


def _common_frames(t_a, t_b):
    """(common times, their positions in t_a, their positions in t_b)"""
    t_a, t_b = np.asarray(t_a), np.asarray(t_b)
    common, at_a, at_b = np.intersect1d(t_a, t_b, return_indices=True)
    return common, at_a, at_b


def _take_frames(volume, at):
    if _lib.is_tensor(volume):
        t = _lib.torch()
        return volume.index_select(0, t.as_tensor(np.asarray(at, np.int64), device=volume.device))
    return np.asarray(volume)[np.asarray(at, np.int64)]


def _find_overlap_between(current_ds, next_ds, coord, volume):
    index = np.asarray(current_ds.coords[coord])
    min_id, max_id = _coord_max(index), _coord_max(next_ds.coords[coord])
    current, following = current_ds[volume], next_ds[volume]
    on_device = _lib.is_tensor(current) or _lib.is_tensor(following)
    y_dtype = np.dtype(np.int32) if on_device else np.asarray(following).dtype
    common, at_current, at_next = _common_frames(current_ds.coords["t"], next_ds.coords["t"])
    if common.size <= 2 or index.size == 0:
        return min_id, max_id, np.array([], dtype=index.dtype), np.array([], dtype=np.asarray(next_ds.coords[coord]).dtype)
    at_current, at_next = at_current[1:-1], at_next[1:-1]
    if on_device:
        t = _lib.torch()
        left = _take_frames(_lib.to_dev(current, t.int32), at_current)
        right = _take_frames(_lib.to_dev(following, t.int32), at_next)
        pairs = parallel.overlap_pairs(left, right, LINK_ATOL, LINK_RTOL)          # sorted by (left id, right id)
        pairs = pairs[np.isin(pairs[:, 0], index)]
        return min_id, max_id, pairs[:, 0].astype(index.dtype), pairs[:, 1].astype(y_dtype)
    from scipy.ndimage import labeled_comprehension
    left, right = _take_frames(current, at_current), _take_frames(following, at_next)
    label_counts = np.maximum(np.bincount(right.flatten(), minlength=max_id + 1), 1)
    comp_func = partial(find_overlaps, atol=LINK_ATOL, rtol=LINK_RTOL, max_label=max_id, label_counts=label_counts)
    overlap_labels = labeled_comprehension(right.flatten(), left.flatten(), index, comp_func, list, [[]])
    x = np.repeat(index, [len(n) for n in overlap_labels])
    y = np.concatenate(overlap_labels, dtype=y_dtype, casting="unsafe")
    return min_id, max_id, x, y


def find_overlap_between_cores(current_ds, next_ds):
    """(largest core id of current_ds, largest of next_ds, x, y): the pairs (x[k] in current_ds, y[k] in next_ds) of cores
    that the rule (atol 5, rtol 0.5) joins on the frames both products hold, the first and the last of them left out; more
    than two common frames are needed, else x and y are empty.  Only ids of current_ds' coordinate are asked; x follows the
    coordinate's order, y ascends under each x (reference: linking.py:49-92).  An empty coordinate counts as largest id 0."""
    return _find_overlap_between(current_ds, next_ds, "core", "core_label")


def find_overlap_between_anvils(current_ds, next_ds):
    """The same for the anvils, compared on the THICK anvil volumes (reference: linking.py:95-140)."""
    return _find_overlap_between(current_ds, next_ds, "anvil", "thick_anvil_label")


def find_overlap_between_files(filename_1, filename_2, store):
    """(reference: linking.py:143-152)"""
    ds_1, ds_2 = _open(store, filename_1), _open(store, filename_2)
    anvil_result = find_overlap_between_anvils(ds_1, ds_2)
    core_result = find_overlap_between_cores(ds_1, ds_2)
    return dict(filename_1=filename_1, filename_2=filename_2, anvil=anvil_result, core=core_result)


def find_new_labels(x, y, size):
    """The component of every node 0 .. size - 1 of the graph with edges (x[k], y[k]); components are numbered by their
    smallest member, so node 0 (no label) stays component 0 (reference: linking.py:155-161)."""
    import scipy.sparse
    import scipy.sparse.csgraph
    overlap_graph = scipy.sparse.coo_array((np.ones(np.size(x)), (x, y)), shape=(size, size))
    return scipy.sparse.csgraph.connected_components(overlap_graph, directed=False)[1]


def process_linking_output(overlap_results):
    """The per-file tables of a chain of find_overlap_between_files results: coordinate `filename`; `previous_filename`,
    `next_filename`, `core_start`, `anvil_start` over it; `core_labels` (core,) and `anvil_labels` (anvil,), the new id of
    every local id, laid end to end from each file's start (reference: linking.py:164-221)."""
    filenames = [str(o["filename_1"]) for o in overlap_results] + [str(overlap_results[-1]["filename_2"])]
    save_ds = LabelDataset(coords=dict(filename=np.array(filenames)))
    save_ds.add("previous_filename", np.array([""] + filenames[:-1]), ("filename",))
    save_ds.add("next_filename", np.array([str(o["filename_2"]) for o in overlap_results] + [""]), ("filename",))
    for kind in ("core", "anvil"):
        start = np.cumsum([0] + [o[kind][0] for o in overlap_results]).astype(np.int32)
        save_ds.add(kind + "_start", start, ("filename",))
        max_label = int(np.sum([overlap_results[0][kind][0]] + [o[kind][1] for o in overlap_results]))
        x = np.concatenate([o[kind][2] + s for o, s in zip(overlap_results, start)])
        y = np.concatenate([o[kind][3] + s for o, s in zip(overlap_results, start[1:])])
        save_ds.add(kind + "_labels", find_new_labels(x, y, max_label + 1).astype(np.int32), (kind,))
    return save_ds


def _sel_filename(links_ds, name, file):
    at = np.nonzero(np.asarray(links_ds.coords["filename"]) == str(file))[0]
    if at.size != 1:
        raise KeyError(str(file))
    return np.asarray(links_ds[name])[at[0]].item()


def _label_map_for_file(file, links_ds, kind):
    start = _sel_filename(links_ds, kind + "_start", file) + 1
    next_file = _sel_filename(links_ds, "next_filename", file)
    stop = _sel_filename(links_ds, kind + "_start", next_file) + 1 if next_file else None
    return np.asarray(links_ds[kind + "_labels"])[start:stop].copy()


def get_core_label_map_for_file(file, links_ds):
    """new id of the local core ids 1, 2, ... of `file` (reference: linking.py:224-231)"""
    return _label_map_for_file(file, links_ds, "core")


def get_anvil_label_map_for_file(file, links_ds):
    """(reference: linking.py:234-243)"""
    return _label_map_for_file(file, links_ds, "anvil")


# ---- tf_relabel_merge ----------------------------------------------------------------------------------------------------
def _table(label_map):
    """the kernel's table: indexed by local id, entry 0 is 0"""
    return np.concatenate([np.zeros(1, np.int32), np.asarray(label_map, np.int32)])


def _relabel_merge_dev(own, own_map, prev=None, next=None):
    """tf_relabel_merge on one device volume.  prev / next: None or (device volume, map, frame table) with the frame table
    an int32 array of own.shape[0] entries (the neighbour's frame under every frame of `own`, or -1)."""
    t = _lib.torch()
    own = _lib.to_dev(own, t.int32)
    T = int(own.shape[0])
    hw = int(own.numel() // T) if T else 0
    if own.numel() == 0:
        return own.clone()
    dev = own.device
    keep = []

    def side(s):
        if s is None:
            return [None, 0, None, None, 0]
        vol, label_map, frames = s
        vol = _lib.to_dev(vol, t.int32)
        frames = np.ascontiguousarray(frames, np.int32)
        if vol.numel() == 0 or not np.any(frames >= 0):
            return [None, 0, None, None, 0]
        if tuple(vol.shape[1:]) != tuple(own.shape[1:]) or frames.shape != (T,) or frames.max() >= vol.shape[0]:
            raise ValueError("tf_relabel_merge: the neighbour's frames do not fit the window")
        lut, frames_d = t.from_numpy(_table(label_map)).to(dev), t.from_numpy(frames).to(dev)
        keep.extend([vol, lut, frames_d])
        return [_lib.ptr(vol), int(vol.shape[0]), _lib.ptr(frames_d), _lib.ptr(lut), int(lut.numel())]

    lut = t.from_numpy(_table(own_map)).to(dev)
    out = t.empty_like(own)
    status = t.empty(2, dtype=t.int64, device=dev)
    _lib.check(_lib.lib().tf_relabel_merge(_lib.ptr(own), T, hw, _lib.ptr(lut), int(lut.numel()), *side(prev), *side(next),
                                           _lib.ptr(out), _lib.ptr(status), _lib.stream_ptr()), "tf_relabel_merge")
    bad_ids, bad_frames = (int(v) for v in status.cpu())
    if bad_ids or bad_frames:
        raise ValueError(f"relabelling met {bad_ids} voxels whose label is negative or larger than its label map"
                         + (f" and {bad_frames} voxels under a frame the neighbour does not hold" if bad_frames else ""))
    return out


def _remap_host(values, label_map):
    values = np.asarray(values)
    if values.size and values.min() < 0:
        raise ValueError("relabelling met a negative label")
    return remap_labels(values, new_labels=label_map)


def relabel_cores_and_anvils(ds, file, links_ds):
    """The three label volumes of `ds` through the maps of `file`: remap_labels(values, new_labels=map), the thick and the
    thin anvils with the anvil map.  `ds` gets new arrays (the old ones are not written to) and is returned.  A label larger
    than the map raises ValueError as the reference's `remapper[1:] = new_labels` does; so does a negative one, where the
    reference indexes from the end (reference: linking.py:246-258)."""
    maps = {"core": get_core_label_map_for_file(file, links_ds), "anvil": get_anvil_label_map_for_file(file, links_ds)}
    for name, kind in _VOLUMES:
        values = ds[name]
        ds[name] = _relabel_merge_dev(values, maps[kind]) if _lib.is_tensor(values) else _remap_host(values, maps[kind])
    return ds


def _positions(t, wanted):
    t, wanted = np.asarray(t), np.asarray(wanted)
    at = np.searchsorted(t, wanted)
    if np.any(at >= t.size) or np.any(t[np.minimum(at, max(t.size - 1, 0))] != wanted):
        raise KeyError("not all values found in index 't'")
    return at


def combine_labels(ds, merge_ds):
    """On the frames of merge_ds.t every zero voxel of the three label volumes of `ds` takes merge_ds' value; `ds`' volumes
    are written in place (reference: linking.py:261-277; the module docstring says which reading of it this is)."""
    at = _positions(ds.coords["t"], merge_ds.coords["t"])
    for name, _ in _VOLUMES:
        values, other = ds[name], merge_ds[name]
        if _lib.is_tensor(values):
            t = _lib.torch()
            index = t.as_tensor(at, device=values.device)
            sel = values.index_select(0, index)
            values.index_copy_(0, index, t.where(sel == 0, _lib.to_dev(other, values.dtype), sel))
        else:
            sel = values[at]
            values[at] = np.where(sel == 0, _dataset._host(other), sel)
    return ds


def _select_frames(ds, times):
    """ds.sel(t=times) of the three label volumes"""
    at = _positions(ds.coords["t"], times)
    out = LabelDataset(coords=dict(t=np.asarray(times)))
    for name, _ in _VOLUMES:
        out.add(name, _take_frames(ds[name], at), ("t", "y", "x"))
    return out


def _shared_times(ds, file, links_ds, store, which):
    """(neighbour's name, its product, the times it contributes) or None: the previous product gives all common frames but
    the last, the next one all but the first; more than one common frame is needed"""
    other_file = _sel_filename(links_ds, which + "_filename", file)
    if not other_file:
        return None
    other_ds = _open(store, other_file)
    t_overlap = np.intersect1d(np.asarray(ds.coords["t"]), np.asarray(other_ds.coords["t"]))
    if t_overlap.size <= 1:
        return None
    return other_file, other_ds, (t_overlap[:-1] if which == "previous" else t_overlap[1:])


def _merge_file(ds, file, links_ds, store, which):
    shared = _shared_times(ds, file, links_ds, store, which)
    if shared is not None:
        other_file, other_ds, times = shared
        ds = combine_labels(ds, relabel_cores_and_anvils(_select_frames(other_ds, times), other_file, links_ds))
    return ds


def merge_previous_file(ds, file, links_ds, store):
    """Fill the zeros of `ds` (already relabelled) from the previous product of `file`, relabelled with its own maps, on
    all common frames but the last (reference: linking.py:305-314)."""
    return _merge_file(ds, file, links_ds, store, "previous")


def merge_next_file(ds, file, links_ds, store):
    """... from the next product, on all common frames but the first (reference: linking.py:317-326)."""
    return _merge_file(ds, file, links_ds, store, "next")


def _load_required_vars(store, file):
    """a copy of the container with the variables the reference loads (linking.py:280-302); label coordinates are left
    behind as xarray leaves them behind with the variables they index"""
    src = _open(store, file)
    ds = LabelDataset(coords={k: v for k, v in src.coords.items() if k not in _LABEL_COORDS})
    for name in _REQUIRED_VARS:
        if name in src:
            ds[name] = src[name]
            if name in src.dims:
                ds.dims[name] = src.dims[name]
    for name, _ in _VOLUMES:
        ds.dims.setdefault(name, ("t", "y", "x"))
    return ds


def relabel_and_merge_file(file, links_ds, store, merge=True):
    """The product `file` of the store under the linked ids, its zeros filled from the previous and the next product where
    they share frames with it (merge=False: the relabelling alone).  Device volumes: one tf_relabel_merge launch per volume
    (reference: linking.py:329-334)."""
    ds = _load_required_vars(store, file)
    if not all(_lib.is_tensor(ds[name]) for name, _ in _VOLUMES):
        ds = relabel_cores_and_anvils(ds, file, links_ds)
        if merge:
            ds = merge_next_file(merge_previous_file(ds, file, links_ds, store), file, links_ds, store)
        return ds
    maps = {"core": get_core_label_map_for_file(file, links_ds), "anvil": get_anvil_label_map_for_file(file, links_ds)}
    sides = {}
    for which in ("previous", "next") if merge else ():
        shared = _shared_times(ds, file, links_ds, store, which)
        if shared is not None:
            other_file, other_ds, times = shared
            frames = np.full(np.asarray(ds.coords["t"]).size, -1, np.int32)
            frames[_positions(ds.coords["t"], times)] = _positions(other_ds.coords["t"], times)
            sides[which] = (other_ds, frames, {"core": get_core_label_map_for_file(other_file, links_ds),
                                               "anvil": get_anvil_label_map_for_file(other_file, links_ds)})
    for name, kind in _VOLUMES:
        side = {w: (o[name], m[kind], f) for w, (o, f, m) in sides.items()}
        ds[name] = _relabel_merge_dev(ds[name], maps[kind], side.get("previous"), side.get("next"))
    return ds


def process_file(file, links_ds, store, merge=True):
    """A window product ready to be written: relabelled and merged, with the label coordinates, the edge / start / end
    flags by the dates of the file name, the NaN flags if `bt` is there, trimmed to those dates, cut down to the cores and
    anvils that remain, cores linked to anvils, step labels, their coordinates and their links
    (reference: linking.py:337-380, without its prints)."""
    ds = relabel_and_merge_file(file, links_ds, store, merge=merge)
    ds = _dataset.add_label_coords(ds)
    _dataset.flag_edge_labels(ds, *get_dates_from_filename(file))
    if "BT" in ds:
        ds["bt"] = ds.pop("BT")
        if "BT" in ds.dims:
            ds.dims["bt"] = ds.dims.pop("BT")
    if "bt" in ds:
        _dataset.flag_nan_adjacent_labels(ds, ds["bt"])
    ds = trim_file_start_and_end(ds, file)
    ds = _dataset.add_label_coords(ds)        # ds.sel(core=..., anvil=...): the ids still present in the trimmed volumes
    _dataset.link_cores_and_anvils(ds)
    _dataset.add_step_labels(ds)
    ds = _dataset.add_label_coords(ds)
    _dataset.link_step_labels(ds)
    return ds


def increment_step_coords(new_ds, past_ds):
    """The non-zero entries of `core_step`, `thick_anvil_step`, `thin_anvil_step` of new_ds shifted by past_ds' largest, in
    place (reference: linking.py:383-396)."""
    for name in ("core_step", "thick_anvil_step", "thin_anvil_step"):
        steps, past = _step_values(new_ds, name), _step_values(past_ds, name)
        steps[steps != 0] += past.max().item()
    return new_ds


def _step_values(ds, name):
    return ds.coords[name] if name in ds.coords else ds[name]


__all__ = ("find_overlaps", "find_overlap_between_cores", "find_overlap_between_anvils", "find_overlap_between_files",
           "find_new_labels", "process_linking_output", "get_core_label_map_for_file", "get_anvil_label_map_for_file",
           "relabel_cores_and_anvils", "combine_labels", "merge_previous_file", "merge_next_file", "relabel_and_merge_file",
           "process_file", "increment_step_coords")
