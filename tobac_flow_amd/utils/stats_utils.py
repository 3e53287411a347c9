"""The statistics helpers the drop-in scripts reach (reference: utils/stats_utils.py:23-30 and :366-367)."""
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


__all__ = ("mse", "n_unique_along_axis")
