"""Label filters used by the detection recipes (mirrors the first three groups of
tobac_flow/analysis.py:15-201 of the reference: NumPy arrays take the reference's own host code, a label tensor on the GPU
takes one read of the volume by tf_label_filter and one tf_apply_lut gather) and the per-label statistics of analysis.py:204-245 / 293-376 as
segmented reductions on the GPU (tf_label_stats), and the coverage / unique-count maps of analysis.py:245-290
(get_label_stats: tf_unique_along_t, tf_unique_per_frame).  The xarray packaging (long_name, units attributes) is out of
scope: xarray is not in this image."""
import numpy as np
from scipy import ndimage as ndi


def _is_dev(x):
    """a torch tensor on the GPU (decided without importing torch for a NumPy caller)"""
    return type(x).__module__.startswith("torch") and bool(getattr(x, "is_cuda", False))


def _dev_mask(labels, mask):
    """the mask as a device tensor of the labels' shape: a tensor as it is, a host array uploaded"""
    from tobac_flow_amd import _lib
    if tuple(labels.shape) != tuple(mask.shape):
        raise AssertionError("Labels and mask parameters must have the same shape")
    return mask.to(labels.device) if _lib.is_tensor(mask) else _lib.to_dev(np.asarray(mask))


def _dev_measure(labels, masks=()):
    """(lengths, hits, present) of ndimage_dev.label_filter for a label tensor and a list of masks"""
    from tobac_flow_amd import ndimage_dev as nd
    if labels.dim() != 3:
        raise ValueError("a label tensor must be a (t, y, x) volume")
    return nd.label_filter(labels, [_dev_mask(labels, m) for m in masks])


def _dev_lengths(lengths, present):
    if not present.all():
        # the reference subscripts find_objects' None for an id that does not occur (analysis.py:31-33)
        raise TypeError(f"'NoneType' object is not subscriptable (label {int(np.flatnonzero(~present)[0]) + 1} does not occur)")
    return lengths


def _dev_empty_comprehension(fn, *args):
    """An all-zero volume hands SciPy's labeled_comprehension an empty label range (analysis.py:78-86), which this SciPy
    rejects with a ValueError.  Run that very call on a one-voxel stand-in so that the behaviour is the reference's,
    whatever it is."""
    fn(np.zeros((1, 1, 1), np.int32), *args)


def _dev_filter(labels, masks, min_length, *, empty, legacy=False, every_id=False):
    """the filters' device form: one tf_label_filter, one tf_apply_lut.  `empty`: what an all-zero volume does in the host
    form (a zero-argument callable that raises, or None: the volume comes back unchanged).  `every_id`: an id that does not
    occur is a ValueError (filter_labels_by_mask: the reference casts labeled_comprehension's None for it to an integer)."""
    from tobac_flow_amd import ndimage_dev as nd
    lengths, hits, present = _dev_measure(labels, masks)
    if lengths.size == 0:
        if empty is not None:
            empty()
        return labels if legacy else labels.clone()
    if every_id and not present.all():
        raise ValueError(f"label {int(np.flatnonzero(~present)[0]) + 1} does not occur in the volume")
    keep = np.ones(lengths.size, bool)
    if min_length is not None:
        keep &= _dev_lengths(lengths, present) >= min_length
    keep &= hits.all(axis=1)
    out = nd.remap_labels(labels, keep).to(labels.dtype)
    if legacy:                                                     # the reference renumbers its argument in place
        labels.copy_(out)
        return labels
    return out


_ONE = np.zeros((1, 1, 1), bool)


def find_object_lengths(labels, axis: int = 0):
    """Extent of every label along `axis` (reference: analysis.py:15-35).  A label tensor on the GPU is measured there
    (axis 0; another axis downloads it) and gives a NumPy array all the same: every caller indexes host arrays with it."""
    if _is_dev(labels):
        if axis != 0 or labels.dim() != 3:
            labels = labels.cpu().numpy()
        else:
            lengths, _, present = _dev_measure(labels)
            return _dev_lengths(lengths, present) if lengths.size else np.array([])
    return np.array([o[axis].stop - o[axis].start for o in ndi.find_objects(labels)])


def mask_labels(labels, mask):
    """Boolean per label (1..max): does it overlap `mask`? (reference: analysis.py:38-63).  NumPy array also for a label
    tensor on the GPU."""
    assert labels.shape == mask.shape, "Labels and mask parameters must have the same shape"
    if _is_dev(labels):
        return _dev_measure(labels, [mask])[1][:, 0]
    hit = np.unique(labels[mask])
    out = np.zeros(labels.max() + 1, dtype=bool)
    out[hit] = True
    return out[1:]


def _keep(labels, wh):
    lut = np.zeros([np.nanmax(labels) + 1], labels.dtype)
    lut[1:] = np.cumsum(wh) * wh
    return lut[labels]


def _lengths_ok(labels, min_length):
    return np.array([o[0].stop - o[0].start for o in ndi.find_objects(labels)]) >= min_length


def _any_in(labels, mask, dtype=None, default=None):
    return ndi.labeled_comprehension(mask, labels, range(1, np.nanmax(labels) + 1), np.any, dtype, default)


def filter_labels_by_length(labels, min_length):
    if _is_dev(labels):
        return _dev_filter(labels, [], min_length, empty=None)
    return _keep(labels, _lengths_ok(labels, min_length))


def filter_labels_by_mask(labels, mask):
    if _is_dev(labels):
        return _dev_filter(labels, [mask], None, every_id=True,
                           empty=lambda: _dev_empty_comprehension(filter_labels_by_mask, _ONE))
    return _keep(labels, _any_in(labels, mask))


def filter_labels_by_length_and_mask(labels, mask, min_length):
    if _is_dev(labels):
        return _dev_filter(labels, [mask], min_length,
                           empty=lambda: _dev_empty_comprehension(filter_labels_by_length_and_mask, _ONE, min_length))
    return _keep(labels, np.logical_and(_lengths_ok(labels, min_length), _any_in(labels, mask)))


def filter_labels_by_multimask(labels, masks):
    if type(masks) is not list:
        raise ValueError("masks input must be a list of masks to process")
    if _is_dev(labels):
        return _dev_filter(labels, masks, None,
                           empty=lambda: _dev_empty_comprehension(filter_labels_by_multimask, [_ONE] * len(masks)))
    return _keep(labels, np.logical_and.reduce([_any_in(labels, m, np.bool_, 0) for m in masks]))


def filter_labels_by_length_and_multimask(labels, masks, min_length):
    if type(masks) is not list:
        raise ValueError("masks input must be a list of masks to process")
    if _is_dev(labels):
        return _dev_filter(labels, masks, min_length,
                           empty=lambda: _dev_empty_comprehension(filter_labels_by_length_and_multimask, [_ONE] * len(masks), min_length))
    return _keep(labels, np.logical_and(_lengths_ok(labels, min_length),
                                        np.logical_and.reduce([_any_in(labels, m, np.bool_, 0) for m in masks])))


def _legacy_filter(labels, keep_fn):
    """in-place renumbering in ascending label order (analysis.py:142-201)"""
    flat = labels.ravel()
    edges = np.cumsum(np.bincount(flat))
    order = np.argsort(flat)
    lengths = np.array([o[0].stop - o[0].start for o in ndi.find_objects(labels)])
    nxt = 1
    for i in range(edges.size - 1):
        if edges[i + 1] > edges[i]:
            where = order[edges[i]:edges[i + 1]]
            if keep_fn(lengths[i], where):
                flat[where] = nxt
                nxt += 1
            else:
                flat[where] = 0
    return labels


def filter_labels_by_length_legacy(labels, min_length):
    if _is_dev(labels):
        return _dev_filter(labels, [], min_length, empty=None, legacy=True)
    return _legacy_filter(labels, lambda n, where: n >= min_length)


def filter_labels_by_length_and_mask_legacy(labels, mask, min_length):
    if _is_dev(labels):
        return _dev_filter(labels, [mask], min_length, empty=None, legacy=True)
    return _legacy_filter(labels, lambda n, where: n >= min_length and np.any(mask.ravel()[where]))


def filter_labels_by_length_and_multimask_legacy(labels, masks, min_length):
    if type(masks) is not list:
        raise ValueError("masks input must be a list of masks to process")
    if _is_dev(labels):
        return _dev_filter(labels, masks, min_length, empty=None, legacy=True)
    return _legacy_filter(labels, lambda n, where: n >= min_length and np.all([np.any(m.ravel()[where]) for m in masks]))


def _label_stats(labels, field, weights, dtype):
    """(mean, std, max, min) per label 1 .. labels.max() through tf_label_stats; NaN where a label carries no weight."""
    import ctypes
    from tobac_flow_amd import _lib
    t = _lib.torch()
    L = _lib.lib()
    if tuple(np.shape(labels)) != tuple(np.shape(field)) or (weights is not None and tuple(np.shape(weights)) != tuple(np.shape(field))):
        raise ValueError("Input labels and field do not have the same shape")          # legacy_utils.py:44-45
    lab = _lib.to_dev(labels, t.int32).contiguous()
    n_labels = int(lab.max()) if lab.numel() else 0
    if dtype is None:
        dtype = np.float32 if _lib.is_tensor(field) else np.asarray(field).dtype
    if n_labels <= 0:
        return tuple(np.zeros(0, dtype) for _ in range(4))
    x = _lib.to_dev(field, t.float32).contiguous()
    w = None if weights is None else _lib.to_dev(weights, t.float32).contiguous()
    out = _lib.empty((n_labels, 6), t.float64)
    ws = _lib.workspace(L.tf_label_stats_workspace_bytes(n_labels), "label_stats")
    _lib.check(L.tf_label_stats(_lib.ptr(lab), _lib.ptr(x), _lib.ptr(w) if w is not None else ctypes.c_void_p(0), lab.numel(),
                                n_labels, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_stats")
    o = out.cpu().numpy()
    carries_weight = o[:, 0] > 0                                  # `if np.nansum(w) > 0 else [nan] * 4`
    return tuple(np.where(carries_weight, o[:, k], np.nan).astype(dtype) for k in (2, 3, 4, 5))


def get_stats_for_labels(labels, da, dim=None, dtype=None):
    """np.nanmean / nanstd / nanmax / nanmin of `da` over every label 1 .. max: four arrays of length labels.max()
    (reference: analysis.py:204-245, which wraps them as DataArrays named f"{dim}_{da.name}_mean" etc.).  Accumulated in
    double on the GPU; the reference sums in the data's own precision."""
    return _label_stats(labels, da, None, dtype)


def weighted_statistics_on_labels(labels, da, weights, name=None, dim=None, dtype=None):
    """Weighted mean, weighted standard deviation, and the max / min over the positively weighted values of `da` for every
    label 1 .. max, NaN values ignored, NaN for labels without weight (reference: analysis.py:293-376)."""
    return _label_stats(labels, da, weights, dtype)


def get_label_stats(da, ds, name=None):
    """Coverage and unique-count maps of a (t, y, x) label volume, added to `ds` (reference: analysis.py:245-290):
    `{name}_fraction` (y, x) float32 = count_nonzero(da, 0) / T, `{name}_unique_count` (y, x) int32 = distinct non-zero
    labels along t, `{name}_temporal_fraction` (t,) float32 = count_nonzero(da, (1, 2)) / (Y * X) and
    `{name}_temporal_unique_count` (t,) int32 = distinct non-zero labels per frame.  `da` is the name of a variable of
    `ds`, or an array / device tensor together with `name=` (there is no DataArray.name here).  Four reads of the volume
    on the GPU: its smallest and largest value (the per-frame kernel is sized by the largest id), then one counting pass
    per direction; both counts are exact."""
    from tobac_flow_amd import _lib
    from tobac_flow_amd import label as _label
    from tobac_flow_amd.utils.stats_utils import _sorted_form, _stamps_fit
    if isinstance(da, str):
        name = da if name is None else name
        da = ds[da]
    if name is None:
        raise ValueError("get_label_stats: an array needs name= (there is no DataArray.name here)")
    if len(da.shape) != 3:
        raise ValueError("get_label_stats: the labels must be a (t, y, x) volume")
    T, Y, X = (int(n) for n in da.shape)
    tensor = _lib.is_tensor(da)
    integer = (not da.dtype.is_floating_point and not da.dtype.is_complex) if tensor else np.asarray(da).dtype.kind in "iu"
    lo, hi = (int(da.min()), int(da.max())) if integer and T * Y * X else (0, 0)
    if integer and T * Y * X and T < 65536 and _stamps_fit(lo, hi, T * Y * X):
        unique, count, _ = _label.unique_along_t(da)
        t_unique, t_count = _label.unique_per_frame(da, hi)
    else:                                                          # not a label volume: counted on the host
        host = _lib.to_host(da) if tensor else np.asarray(da)
        unique, count = _sorted_form(host, 0), np.count_nonzero(host, 0)
        t_unique, t_count = _sorted_form(host.reshape([T, -1]), 1), np.count_nonzero(host, (1, 2))
    ds.add(f"{name}_fraction", count / T, ("y", "x"), np.float32)
    ds.add(f"{name}_unique_count", unique, ("y", "x"), np.int32)
    ds.add(f"{name}_temporal_fraction", t_count / (X * Y), ("t",), np.float32)
    ds.add(f"{name}_temporal_unique_count", t_unique, ("t",), np.int32)
