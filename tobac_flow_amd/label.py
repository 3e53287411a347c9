"""Flow-aware labelling (mirrors /root/reference/tobac_flow/label.py:84-321).

The whole of it runs behind two C-ABI entry points of the HIP library (include/tobac_flow_hip.h):
tf_flow_label (label.py:84-175: per-step connected components, then the linking) and tf_flow_link_overlap
(label.py:249-321).  What the reference does per label in a Python loop -- a bincount / unique over the label's
pixels in the two nearest-neighbour-warped label volumes (label.py:139-170, utils/label_utils.py:352-376) -- is one
run-length / sort / reduce-by-key pass over the volume on the GPU; the small label graph is then walked in the
reference's own order inside the library (labels ascending, each unvisited label opens a group and absorbs, breadth
first, every not-yet-visited label it overlaps, forward neighbours before backward ones; the relation is DIRECTED, so
first come, first served).

`subsegment_labels` (label.py:13-80; subsegment_shrink != 0) splits every per-step region by a distance-transform
watershed.  The reference composes it from SciPy and scikit-image; here it is a chain of device operators:
flat_label (tf_label), the exact integer distance transform of every frame (tf_edt2d_frames), the pixel counts
(tf_label_sizes), tf_subseg_prepare (dist_mask in float64, bit for bit numpy's, and the shrunk markers),
ndimage_dev.peak_local_max_2d per frame (candidates on the device, the shared host `select_peaks` for the selection),
flat_label of the markers, tf_subseg_rank and one tf_watershed per frame.  Two facts fix that shape.  scikit-image pushes
every marker of a frame with age 0, so the pop order of equal-valued markers depends on the whole content of THAT frame's
heap: the flood runs frame by frame, in the reference's order (on_ambiguous="reference").  And the flood's key has to keep
the order of the float64 -dist_mask: rounded to float32, values of different regions meet and the heap's arrangement
changes with them; the flood only compares keys, so the per-frame rank of -dist_mask, stored as float32, is exact.  The
reference's -1 background markers never enter scikit-image's flood (its _validate_inputs multiplies the markers by the
mask); they are 0 here.
Contract: where no peak-selection tie exists the labels equal the reference's bit for bit.  A peak-selection tie is two
equal-valued peak candidates closer than peak_min_distance (Chebyshev) that do not both lie inside one shrunk marker:
scikit-image orders candidates with numpy's non-stable argsort, so which of the two becomes a peak changes with the numpy
version; the result is then a valid greedy selection (tests/test_host_logic.py documents the same tie for select_peaks).
Deviations: a frame without any background voxel raises ValueError (the reference's answer there rests on the float64
rounding of 1e18 + d^2 under its time sampling of 1e9), and so does a frame with more than 2^24 distinct distances.
"""
import ctypes
import warnings

import numpy as np
from scipy import ndimage as ndi

from tobac_flow_amd import _lib
from tobac_flow_amd.utils.label_utils import find_overlapping_labels


def _structure_bytes(structure):
    s = np.asarray(structure)
    if s.shape != (3, 3, 3):
        raise ValueError("structure must be a (3, 3, 3) array")
    s = np.ascontiguousarray(s != 0, np.uint8)
    if int(s[0].sum()) != 1 or int(s[2].sum()) != 1:
        # label.py:129-131 unpacks Flow.convolve's stack into exactly two arrays
        raise ValueError("structure must have exactly one element in each of its first and last planes "
                         f"(got {int(s[0].sum())} and {int(s[2].sum())}): the reference unpacks two warped label stacks")
    return s


def _call_with_run_retry(fn, size_fn, shape, tag):
    """The library sizes its pair-count scratch for a number of label runs; on TF_ENOMEM it reports the number it
    needs (in the object-count slot) and the call is repeated once with that."""
    T, H, W = shape
    n_obj = ctypes.c_int(0)
    guess = max(T * H * W // 16, 65536)
    for attempt in range(2):
        ws = _lib.workspace(size_fn(T, H, W, guess), tag)
        rc = fn(ws, n_obj)
        if rc == -2 and attempt == 0 and n_obj.value > guess:
            guess = int(n_obj.value) + 1024
            continue
        break
    _lib.check(rc, tag)
    return n_obj.value


def link_overlap_dev(flow, flat_dev, structure, overlap, absolute_overlap):
    """tf_flow_link_overlap on a device int32 tensor of per-step labels; returns the device int32 object labels."""
    t = _lib.torch()
    L = _lib.lib()
    st = _structure_bytes(structure)
    fw, bw = flow._dev_flows()
    T, H, W = flat_dev.shape
    out = _lib.empty((T, H, W), t.int32)
    _call_with_run_retry(
        lambda ws, n_obj: L.tf_flow_link_overlap(_lib.ptr(flat_dev), _lib.ptr(fw), _lib.ptr(bw), T, H, W,
                                                 st.ctypes.data_as(_lib._P), float(overlap), int(absolute_overlap),
                                                 _lib.ptr(out), ctypes.byref(n_obj), _lib.ptr(ws), ws.numel(),
                                                 _lib.stream_ptr()),
        L.tf_flow_link_workspace_bytes, (T, H, W), "tf_flow_link_overlap")
    return out


def flow_label_dev(flow, mask_dev, structure, overlap, absolute_overlap):
    """tf_flow_label on a device uint8 mask; returns the device int32 object labels."""
    t = _lib.torch()
    L = _lib.lib()
    st = _structure_bytes(structure)
    fw, bw = flow._dev_flows()
    T, H, W = mask_dev.shape
    out = _lib.empty((T, H, W), t.int32)
    _call_with_run_retry(
        lambda ws, n_obj: L.tf_flow_label(_lib.ptr(mask_dev), _lib.ptr(fw), _lib.ptr(bw), T, H, W,
                                          st.ctypes.data_as(_lib._P), float(overlap), int(absolute_overlap),
                                          _lib.ptr(out), ctypes.byref(n_obj), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr()),
        L.tf_flow_label_workspace_bytes, (T, H, W), "tf_flow_label")
    return out


def _finish(new_dev, present_dev, dtype, on_device):
    if not bool(((new_dev != 0) == present_dev).all()):
        warnings.warn("Not all regions present in labeled array", RuntimeWarning)      # label.py:172-174
    return new_dev if on_device else _lib.to_host(new_dev).astype(dtype, copy=False)


def flow_label(flow, mask, structure=ndi.generate_binary_structure(3, 1), dtype=np.int32, overlap: float = 0.0,
               absolute_overlap: int = 0, subsegment_shrink: float = 0.0, peak_min_distance: int = 10):
    """Label 3-D connected objects in a semi-Lagrangian frame (reference: label.py:84-175)."""
    t = _lib.torch()
    on_device = isinstance(mask, t.Tensor)
    m = (_lib.to_dev(mask) != 0)
    if tuple(m.shape) != tuple(flow.shape):
        raise AssertionError("Data input must have the same shape as the Flow object")
    if subsegment_shrink != 0:                               # label.py:126-131; a region without a marker stays 0 (_finish warns)
        flat_dev = subsegment_labels_dev(m, subsegment_shrink, peak_min_distance)
        new_dev = link_overlap_dev(flow, flat_dev, structure, overlap, absolute_overlap)
    else:
        new_dev = flow_label_dev(flow, m.to(t.uint8).contiguous(), structure, overlap, absolute_overlap)
    return _finish(new_dev, m, dtype, on_device)


_INT32_MAX = 2 ** 31 - 1


def subsegment_labels_dev(mask_dev, shrink_factor=0.1, peak_min_distance=5, stats=None):
    """subsegment_labels on a (T, H, W) device tensor whose non-zero voxels are the regions; returns the device int32
    subsegment labels (the recipe and its contract: the module docstring).  stats: a list that receives, per flooded frame,
    (frame, the `stats` dictionary of its watershed_dev call)."""
    from tobac_flow_amd import ndimage_dev as nd
    from tobac_flow_amd.watershed import neighbour_offsets, watershed_dev
    t = _lib.torch()
    L = _lib.lib()
    if mask_dev.dim() != 3 or 0 in mask_dev.shape:
        raise ValueError(f"subsegment_labels: a non-empty (t, y, x) volume is required, got shape {tuple(mask_dev.shape)}")
    T, H, W = (int(n) for n in mask_dev.shape)
    labels = nd.flat_label(mask_dev != 0)                                        # label.py:49
    inside = labels != 0
    d2, _ = nd.edt_squared_frames(labels == 0)                                   # label.py:52, frame by frame and in integers
    full = t.nonzero(d2[:, 0, 0] == _INT32_MAX).flatten()
    if full.numel():
        raise ValueError(f"subsegment_labels: frame {int(full[0])} has no background voxel: the distance to the edge of its "
                         "region is not defined")
    n_labels = int(labels.max())
    counts = _label_sizes_dev(labels, n_labels)                                  # label.py:53
    dist = _lib.empty((T, H, W), t.float64)
    shrunk = _lib.empty((T, H, W), t.uint8)
    _lib.check(L.tf_subseg_prepare(_lib.ptr(labels), _lib.ptr(d2), _lib.ptr(counts), n_labels, labels.numel(),
                                   float(shrink_factor), _lib.ptr(dist), _lib.ptr(shrunk), _lib.stream_ptr()),
               "tf_subseg_prepare")                                              # label.py:54-56
    del d2
    seeds = shrunk.view(t.bool)
    for i in range(T):                                                           # label.py:59-64
        peaks = nd.peak_local_max_2d(dist[i], min_distance=peak_min_distance, threshold_abs=1e-8)
        if len(peaks):
            p = t.from_numpy(np.ascontiguousarray(peaks, np.int64)).to(dist.device)
            seeds[i][p[:, 0], p[:, 1]] = True
    markers = nd.flat_label(seeds)                                               # label.py:66
    markers.mul_(inside)                                                         # label.py:67, with 0 for the reference's -1
    del seeds, shrunk

    plane = ndi.generate_binary_structure(3, 1)
    plane[0] = 0
    plane[-1] = 0
    nbr = neighbour_offsets(plane)                                               # (-y, -x, +x, +y): scikit-image's 2-D order
    still = t.zeros((1, H, W, 2), dtype=t.float32, device=dist.device)
    inside8 = inside.to(t.int8)
    flood = (markers != 0).view(T, -1).any(1).cpu().numpy()                      # a frame without a marker stays 0
    out = t.zeros((T, H, W), dtype=t.int32, device=dist.device)
    for i in np.flatnonzero(flood):                                              # label.py:75-78
        i = int(i)
        keys = t.unique(dist[i])                                                 # the frame's distinct values, ascending
        rank = _lib.empty((1, H, W), t.float32)
        _lib.check(L.tf_subseg_rank(_lib.ptr(dist[i]), H * W, _lib.ptr(keys), keys.numel(), _lib.ptr(rank), _lib.stream_ptr()),
                   "tf_subseg_rank")
        flood_stats = {} if stats is not None else None
        out[i] = watershed_dev(still, still, rank, markers[i:i + 1], inside8[i:i + 1], nbr, stats=flood_stats)[0]
        if stats is not None:
            stats.append((i, flood_stats))
    return out


def subsegment_labels(input_mask, shrink_factor: float = 0.1, peak_min_distance: int = 5):
    """Split the regions of a (t, y, x) mask, time step by time step, by a watershed of their distance transform
    (reference: label.py:13-80).  A numpy array gives a numpy int32 array, a device tensor a device int32 tensor."""
    on_device = isinstance(input_mask, _lib.torch().Tensor)
    out = subsegment_labels_dev(_lib.to_dev(input_mask), shrink_factor, peak_min_distance)
    return out if on_device else _lib.to_host(out)


def find_neighbour_labels(label, label_stack, bins, args, processed_labels, forward_labels, back_labels,
                          overlap: float = 0, absolute_overlap: int = 1):
    """Append the not-yet-visited labels that overlap `label` at t+1 / t-1 (reference: label.py:178-245;
    kept for API parity -- flow_label / flow_link_overlap use the vectorised form above)."""
    if bins[label] > bins[label - 1]:
        locs = args[bins[label - 1]:bins[label]]
        for warped in (forward_labels, back_labels):
            for new_label in find_overlapping_labels(warped, locs, bins, overlap=overlap,
                                                     absolute_overlap=absolute_overlap):
                if not processed_labels[new_label]:
                    label_stack.append(new_label)
                    processed_labels[new_label] = True


def flow_link_overlap(flow, flat_labels, structure=ndi.generate_binary_structure(3, 1), dtype=np.int32,
                      overlap: float = 0.0, absolute_overlap: int = 0):
    """Link existing per-step labels into contiguous objects (reference: label.py:249-321)."""
    t = _lib.torch()
    on_device = isinstance(flat_labels, t.Tensor)
    flat_dev = _lib.to_dev(flat_labels, t.int32)
    if tuple(flat_dev.shape) != tuple(flow.shape):
        raise AssertionError("Data input must have the same shape as the Flow object")
    new_dev = link_overlap_dev(flow, flat_dev, structure, overlap, absolute_overlap)
    return _finish(new_dev, flat_dev != 0, dtype, on_device)


def pair_counts(a, b, include_b_zero=False, _keep_on_device=False):
    """Every distinct pair (a[i], b[i]) with a[i] > 0 and b[i] > 0 (b[i] >= 0 with include_b_zero) of two int32 label
    volumes and how often it occurs, sorted by (a, b): host int64 arrays (ids_a, ids_b, counts).  tf_pair_counts --
    the per-label np.bincount / np.unique of the reference (label_utils.py:352-376, linking.py:33-47, dataset.py:292-297)
    as one run-length / sort / reduce-by-key pass on the GPU."""
    t = _lib.torch()
    L = _lib.lib()
    a_dev, b_dev = _lib.to_dev(a, t.int32).contiguous(), _lib.to_dev(b, t.int32).contiguous()
    if a_dev.shape != b_dev.shape:
        raise ValueError("label volumes must have the same shape")
    n = a_dev.numel()
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    runs = cap = max(n // 16, 65536)
    n_out = ctypes.c_int64(0)
    for _ in range(3):
        ws = _lib.workspace(L.tf_pair_counts_workspace_bytes(n, runs), "pair_counts")
        oa, ob, oc = _lib.empty((cap,), t.int32), _lib.empty((cap,), t.int32), _lib.empty((cap,), t.int64)
        rc = L.tf_pair_counts(_lib.ptr(a_dev), _lib.ptr(b_dev), n, 1 if include_b_zero else 0, _lib.ptr(oa), _lib.ptr(ob),
                              _lib.ptr(oc), cap, ctypes.byref(n_out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        if rc == -2 and n_out.value > 0:                      # needs room for that many runs / pairs
            runs = cap = int(n_out.value) + 1024
            continue
        break
    _lib.check(rc, "tf_pair_counts")
    k = int(n_out.value)
    if _keep_on_device:
        return oa[:k], ob[:k], oc[:k]
    return (oa[:k].cpu().numpy().astype(np.int64), ob[:k].cpu().numpy().astype(np.int64), oc[:k].cpu().numpy())


def make_step_labels_dev(labels):
    """utils.label_utils.make_step_labels (reference: label_utils.py:183-200) on a device int32 volume: the pieces of the
    non-zero mask connected within a time step (flat_label = tf_label, t planes of the structure zeroed), every piece split
    into the original labels it contains, ids contiguous from 1 ordered by piece, then by label = the rank of the voxel's
    (piece, label) pair among the distinct pairs (tf_pair_counts returns them sorted; tf_pair_rank looks the rank up).
    Labels must be >= 0 (label volumes of the detection recipes are)."""
    from tobac_flow_amd import ndimage_dev as nd
    t = _lib.torch()
    lab = _lib.to_dev(labels, t.int32).contiguous()
    out = t.zeros_like(lab)
    if lab.numel() == 0:
        return out
    if int(lab.min().item()) < 0:
        raise ValueError("make_step_labels_dev: negative labels (the device form ranks (piece, label) pairs of positive labels)")
    plane = ndi.generate_binary_structure(3, 1)
    plane[0] = 0
    plane[2] = 0
    pieces, n_pieces = nd.label(lab != 0, plane)
    if n_pieces == 0:
        return out
    pa, pb, _ = pair_counts(pieces, lab, _keep_on_device=True)
    _lib.check(_lib.lib().tf_pair_rank(_lib.ptr(pieces), _lib.ptr(lab), lab.numel(), _lib.ptr(pa), _lib.ptr(pb), pa.numel(),
                                       _lib.ptr(out), _lib.stream_ptr()), "tf_pair_rank")
    return out


def label_sizes(labels, n_labels=None):
    """np.bincount(labels.ravel(), minlength=n_labels + 1) of a non-negative int32 volume (tf_label_sizes); ids above
    n_labels are not counted."""
    t = _lib.torch()
    lab = _lib.to_dev(labels, t.int32).contiguous()
    if n_labels is None:
        n_labels = int(lab.max()) if lab.numel() else 0
    if lab.numel() == 0:
        return np.zeros(int(n_labels) + 1, np.int64)
    return _lib.to_host(_label_sizes_dev(lab, n_labels))


def _label_sizes_dev(lab, n_labels):
    """label_sizes of a non-empty contiguous int32 device volume, left on the device (int64[n_labels + 1])"""
    out = _lib.empty((int(n_labels) + 1,), _lib.torch().int64)
    _lib.check(_lib.lib().tf_label_sizes(_lib.ptr(lab), lab.numel(), int(n_labels), _lib.ptr(out), _lib.stream_ptr()), "tf_label_sizes")
    return out


def slice_labels_dev(labels):
    """utils.label_utils.slice_labels on the GPU (tf_slice_labels): (device int32 step labels, number of step labels)."""
    t = _lib.torch()
    L = _lib.lib()
    lab = _lib.to_dev(labels, t.int32).contiguous()
    T = lab.shape[0]
    hw = lab.numel() // max(T, 1)
    out = _lib.empty(tuple(lab.shape), t.int32)
    if lab.numel() == 0:
        return out, 0
    n_ids = ctypes.c_int64(0)
    cap = 1 << 22
    for _ in range(2):
        ws = _lib.workspace(L.tf_slice_labels_workspace_bytes(T, cap), "slice_labels")
        rc = L.tf_slice_labels(_lib.ptr(lab), T, hw, _lib.ptr(out), ctypes.byref(n_ids), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        if rc == -2 and n_ids.value > cap:
            cap = int(n_ids.value)
            continue
        break
    _lib.check(rc, "tf_slice_labels")
    return out, int(n_ids.value)


_PROPS_RECORD = np.dtype([("count", np.int64), ("area_nansum", np.float64), ("w", np.float64), ("wx", np.float64),
                          ("wy", np.float64), ("wlat", np.float64), ("wlon", np.float64), ("tmin", np.int32), ("tmax", np.int32)])


def label_props(labels, n_labels, area=None, x=None, y=None, lat=None, lon=None, t_rank=None):
    """tf_label_props on an int32 (T, H, W) label volume (numpy or device tensor): a host record array of n_labels + 1
    entries with the fields count, area_nansum, w, wx, wy, wlat, wlon, tmin, tmax (entry 0, the background, stays empty).
    area, lat, lon: (H, W); x: (W,); y: (H,); t_rank: (T,) ints >= 0 -- host arrays or device tensors, passed as they are;
    None switches the sums that need it off."""
    t = _lib.torch()
    lab = _lib.to_dev(labels, t.int32, share=True).contiguous()
    if lab.dim() != 3:
        raise ValueError("label_props: labels must be a (t, y, x) volume")
    T, H, W = (int(n) for n in lab.shape)
    n_labels = int(n_labels)
    if lab.numel() == 0 or n_labels < 0:
        raise ValueError("label_props: empty volume or negative n_labels")
    keep = []                                                     # the operands stay alive until the result is on the host

    def operand(a, shape, dtype, name):
        if a is None:
            return ctypes.c_void_p(0)
        if not _lib.is_tensor(a):
            a = np.ascontiguousarray(a, dtype)
        if tuple(a.shape) != shape:
            raise ValueError(f"label_props: {name} has shape {tuple(a.shape)}, expected {shape}")
        keep.append(_lib.to_dev(a, getattr(t, np.dtype(dtype).name), share=True))
        return _lib.ptr(keep[-1])

    args = [operand(area, (H, W), np.float64, "area"), operand(x, (W,), np.float64, "x"), operand(y, (H,), np.float64, "y"),
            operand(lat, (H, W), np.float64, "lat"), operand(lon, (H, W), np.float64, "lon"),
            operand(t_rank, (T,), np.int32, "t_rank")]
    acc = _lib.empty((n_labels + 1, 8), t.float64)
    _lib.check(_lib.lib().tf_label_props(_lib.ptr(lab), T, H, W, n_labels, *args, _lib.ptr(acc), _lib.stream_ptr()),
               "tf_label_props")
    return acc.cpu().numpy().view(_PROPS_RECORD).reshape(n_labels + 1)


def unique_along_t(volume):
    """Per pixel of an int32 (T, H, W) volume the number of distinct non-zero values along t and the number of non-zero
    ones (tf_unique_along_t): host int32 (H, W) arrays, and the pixels per workgroup of the LDS form that ran (0: the
    per-pixel sets lived in HBM scratch, T > 640)."""
    t = _lib.torch()
    L = _lib.lib()
    vol = _lib.to_dev(volume, t.int32, share=True).contiguous()
    T, H, W = (int(n) for n in vol.shape)
    if vol.numel() == 0:
        raise ValueError("unique_along_t: empty volume")
    uniq, nz = _lib.empty((H, W), t.int32), _lib.empty((H, W), t.int32)
    need = L.tf_unique_along_t_workspace_bytes(T, H, W)
    ws = _lib.workspace(need, "unique_along_t") if need else None
    lanes = ctypes.c_int(-1)
    _lib.check(L.tf_unique_along_t(_lib.ptr(vol), T, H, W, _lib.ptr(uniq), _lib.ptr(nz), ctypes.byref(lanes),
                                   _lib.ptr(ws) if ws is not None else ctypes.c_void_p(0), ws.numel() if ws is not None else 0,
                                   _lib.stream_ptr()), "tf_unique_along_t")
    return uniq.cpu().numpy(), nz.cpu().numpy(), int(lanes.value)


def unique_per_frame(volume, n_labels=None):
    """Per frame of an int32 (T, ...) volume the number of distinct ids in [1, n_labels] (default: the largest value) and
    the number of non-zero voxels (tf_unique_per_frame): host arrays int32 (T,) and int64 (T,)."""
    t = _lib.torch()
    L = _lib.lib()
    vol = _lib.to_dev(volume, t.int32, share=True).contiguous()
    T = int(vol.shape[0])
    if vol.numel() == 0:
        raise ValueError("unique_per_frame: empty volume")
    if n_labels is None:
        n_labels = max(int(vol.max()), 0)
    uniq, nz = _lib.empty((T,), t.int32), _lib.empty((T,), t.int64)
    ws = _lib.workspace(L.tf_unique_per_frame_workspace_bytes(int(n_labels)), "unique_per_frame")
    _lib.check(L.tf_unique_per_frame(_lib.ptr(vol), T, vol.numel() // T, int(n_labels), _lib.ptr(uniq), _lib.ptr(nz),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_unique_per_frame")
    return uniq.cpu().numpy(), nz.cpu().numpy()


__all__ = ("subsegment_labels", "subsegment_labels_dev", "flow_label", "find_neighbour_labels", "flow_link_overlap", "flow_label_dev", "link_overlap_dev",
           "pair_counts", "label_sizes", "slice_labels_dev", "make_step_labels_dev", "label_props", "unique_along_t",
           "unique_per_frame")
