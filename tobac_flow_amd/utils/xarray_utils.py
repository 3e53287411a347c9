"""Coordinate helpers of the gridding recipes (reference: utils/xarray_utils.py:25-31; no xarray needed)."""
import numpy as np


def get_coord_bin_edges(coord):
    """The size + 1 bin edges around the points of a one-dimensional coordinate: the midpoints of neighbouring points
    inside, the first and the last point themselves at the ends.  `coord` is an array or anything with `.data`; the sum
    and the halving are taken in float64 whatever the coordinate's dtype, as the reference does."""
    data = np.asarray(getattr(coord, "data", coord))
    bins = np.zeros(data.size + 1)
    bins[:-1] += data
    bins[1:] += data
    bins[1:-1] /= 2
    return bins


# ---- selections on a dataset.LabelDataset table (reference: utils/xarray_utils.py:106-134) -------------------------------
# Cutting a dimension cuts its coordinate and every variable that has the dimension, together.  Variables may be NumPy
# arrays or device tensors; a device tensor is cut on the device and stays there.  Where the records to keep follow from a
# device column (the *_step_*_index variables), the coordinate is cut on the device as well and only the cut coordinate
# comes back to the host.
def _is_tensor(x):
    from tobac_flow_amd import _lib
    return _lib.is_tensor(x)


def cut_dim(ds, dim, keep):
    """a new LabelDataset with dimension `dim` reduced to the positions `keep` (a NumPy integer array, or a device tensor
    of positions), in that order"""
    from tobac_flow_amd import _lib
    from tobac_flow_amd.dataset import LabelDataset
    keep_host = None if _is_tensor(keep) else np.asarray(keep, np.int64)
    keep_dev = keep if _is_tensor(keep) else None
    out = LabelDataset(coords=dict(ds.coords))
    out.dims = dict(ds.dims)
    if dim in ds.coords:
        if keep_host is not None:
            out.coords[dim] = np.asarray(ds.coords[dim])[keep_host]
        else:
            t = _lib.torch()
            coord = np.asarray(ds.coords[dim])
            ticks = coord.view(np.int64) if coord.dtype.kind in "mM" else coord
            cut = t.from_numpy(np.ascontiguousarray(ticks)).to(keep.device)[keep].cpu().numpy()
            out.coords[dim] = cut.view(coord.dtype) if coord.dtype.kind in "mM" else cut
    for name, value in ds.items():
        dims = ds.dims.get(name, ())
        if dim not in dims:
            out[name] = value
            continue
        axis = dims.index(dim)
        if _is_tensor(value):
            if keep_dev is None:
                keep_dev = _lib.torch().from_numpy(keep_host).to(value.device)
            out[name] = value.index_select(axis, keep_dev.to(value.device))
        else:
            if keep_host is None:
                keep_host = keep_dev.cpu().numpy()
            out[name] = np.take(np.asarray(value), keep_host, axis=axis)
    return out


def positions_of(coord, ids):
    """positions of `ids` in the sorted coordinate `coord`; KeyError for an id that is not there (as xarray's .sel)"""
    coord, ids = np.asarray(coord), np.atleast_1d(np.asarray(ids))
    at = np.searchsorted(coord, ids)
    found = at < coord.size
    found[found] = coord[at[found]] == ids[found]
    if not found.all():
        raise KeyError(f"not all values found in the coordinate: {ids[~found][:5]}")
    return at.astype(np.int64)


def isin_coord(column, coord):
    """np.isin(column, coord) for a NumPy column; for a device column, the same mask on the device"""
    if _is_tensor(column):
        from tobac_flow_amd import _lib
        t = _lib.torch()
        return t.isin(column, t.from_numpy(np.ascontiguousarray(coord)).to(column.device))
    return np.isin(np.asarray(column), coord)


def mask_positions(mask):
    """positions where a NumPy or device mask holds"""
    return mask.nonzero().reshape(-1) if _is_tensor(mask) else np.flatnonzero(mask)


def cut_steps(ds, step_dim, index_name, parent_dim):
    """keep the step records whose parent id (variable `index_name`) is in the coordinate `parent_dim`"""
    return cut_dim(ds, step_dim, mask_positions(isin_coord(ds[index_name], ds.coords[parent_dim])))


def sel_anvil(ds, anvil):
    """the anvils with the ids `anvil` and the thick and thin anvil steps that belong to them"""
    return isel_anvil(ds, positions_of(ds.coords["anvil"], anvil))


def isel_anvil(ds, anvil):
    """the anvils at the positions `anvil` and the thick and thin anvil steps that belong to them"""
    ds = cut_dim(ds, "anvil", np.atleast_1d(np.arange(ds.coords["anvil"].size)[anvil]))
    ds = cut_steps(ds, "thick_anvil_step", "thick_anvil_step_anvil_index", "anvil")
    return cut_steps(ds, "thin_anvil_step", "thin_anvil_step_anvil_index", "anvil")


def sel_core(ds, core):
    """the cores with the ids `core` and the core steps that belong to them"""
    return isel_core(ds, positions_of(ds.coords["core"], core))


def isel_core(ds, core):
    """the cores at the positions `core` and the core steps that belong to them"""
    ds = cut_dim(ds, "core", np.atleast_1d(np.arange(ds.coords["core"].size)[core]))
    return cut_steps(ds, "core_step", "core_step_core_index", "core")


__all__ = ("get_coord_bin_edges", "sel_anvil", "isel_anvil", "sel_core", "isel_core")
