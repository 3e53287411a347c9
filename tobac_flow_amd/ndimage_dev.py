"""Device-resident versions of the scipy.ndimage / numpy glue the detection recipes use (SURVEY.md
section 8f-2).  Every function takes and returns torch tensors on the GPU and is bit-exact with the SciPy /
numpy call it replaces (tests/test_gpu_detection.py); the numpy paths of detection.py keep using SciPy."""
import numpy as np

from tobac_flow_amd import _lib


def _structure27(structure):
    s = np.asarray(structure) != 0
    if s.shape != (3, 3, 3):
        raise ValueError("structure must be a (3, 3, 3) array")
    return np.ascontiguousarray(s, np.uint8)


def _as_u8_mask(x):
    """non-zero -> 1 as a contiguous uint8 tensor; a bool tensor is reinterpreted in place (its bytes are 0 / 1 already)"""
    t = _lib.torch()
    if x.dtype == t.bool:
        return x.contiguous().view(t.uint8)
    return (x != 0).contiguous().view(t.uint8)


def _binary(t_in, structure, op, iterations, border_value):
    t = _lib.torch()
    L = _lib.lib()
    x = _as_u8_mask(t_in)
    T, H, W = x.shape
    out = t.empty_like(x)
    tmp = t.empty_like(x) if iterations > 1 else None
    st = _structure27(structure)
    _lib.check(L.tf_binary_morph(_lib.ptr(x), T, H, W, st.ctypes.data_as(_lib._P), op, int(iterations), int(bool(border_value)),
                                 _lib.ptr(out), _lib.ptr(tmp), _lib.stream_ptr()), "tf_binary_morph")
    return out.view(t.bool)                       # the kernels write 0 / 1


def binary_erosion(x, structure, iterations=1, border_value=0):
    """scipy.ndimage.binary_erosion(x, structure=structure, iterations=iterations, border_value=border_value)"""
    return _binary(x, structure, 0, iterations, border_value)


def binary_dilation(x, structure, iterations=1, border_value=0):
    return _binary(x, structure, 1, iterations, border_value)


def binary_opening(x, structure, iterations=1):
    """scipy.ndimage.binary_opening: erosion then dilation, border_value 0"""
    return binary_dilation(binary_erosion(x, structure, iterations), structure, iterations)


def linearise_field(field, lower_threshold, upper_threshold):
    """utils.normalisation_utils.linearise_field on a float32 device tensor"""
    t = _lib.torch()
    if lower_threshold == upper_threshold:
        raise ValueError("lower and upper thresholds must have different values")
    f = field.to(t.float32).contiguous()
    out = t.empty_like(f)
    _lib.check(_lib.lib().tf_linearise(_lib.ptr(f), f.numel(), float(lower_threshold), float(upper_threshold),
                                       _lib.ptr(out), _lib.stream_ptr()), "tf_linearise")
    return out


def field_masks(field):
    """(field >= 1, (field <= 0) | isnan(field), isnan(field)) as bool tensors from ONE read of a float32 field
    (tf_field_masks: the thresholds of detect_anvils' seeds, detection.py:551-552, 607-609)"""
    t = _lib.torch()
    f = field.to(t.float32).contiguous()
    ge1, le0, isn = (t.empty(f.shape, dtype=t.uint8, device=f.device) for _ in range(3))
    _lib.check(_lib.lib().tf_field_masks(_lib.ptr(f), f.numel(), _lib.ptr(ge1), _lib.ptr(le0), _lib.ptr(isn), _lib.stream_ptr()),
               "tf_field_masks")
    return ge1.view(t.bool), le0.view(t.bool), isn.view(t.bool)


def merge_seeds(comp, bg, isnan):
    """seeds = -1 where (bg | isnan) else comp (tf_merge_seeds; detection.py:558, 616)"""
    t = _lib.torch()
    c = comp.to(t.int32).contiguous()
    out = t.empty_like(c)
    _lib.check(_lib.lib().tf_merge_seeds(_lib.ptr(c), _lib.ptr(_as_u8_mask(bg)), _lib.ptr(_as_u8_mask(isnan)), c.numel(), _lib.ptr(out),
                                         _lib.stream_ptr()), "tf_merge_seeds")
    return out


def label_filter(labels, criteria=()):
    """(lengths int64[n], hits bool[n, K], present bool[n]) for the labels 1..n of a (t, y, x) label tensor, n its largest
    label, in one read of the volume (tf_label_filter): the extent along the leading axis (0 for an id that does not occur),
    whether some voxel of the label satisfies each of the K <= 8 criteria, and whether the id occurs at all.  A criterion is
    a bool / uint8 tensor of the labels' shape (satisfied where non-zero) or a tuple (field_tensor, op, threshold) with op
    one of ">=", ">", "<=", "<": float32 and float64 fields are compared in their own dtype, as NumPy compares an array
    with a Python float; any other dtype is converted to float64.  n = 0 returns empty arrays without a launch."""
    t = _lib.torch()
    lab = labels.to(t.int32).contiguous()
    if lab.dim() != 3:
        raise ValueError("label_filter: the labels must be a (t, y, x) volume")
    T, H, W = lab.shape
    criteria = list(criteria)
    K = len(criteria)
    if K > 8:
        raise ValueError("label_filter: at most 8 criteria")
    crit = (_lib.LabelCriterion * max(K, 1))()
    keep = []                                                       # the operands stay alive until the kernel is enqueued
    for k, c in enumerate(criteria):
        if isinstance(c, tuple):
            field, op, threshold = c
            if op not in _lib.CMP_OPS:
                raise ValueError(f"label_filter: unknown comparison {op!r}")
            field = field if field.dtype in (t.float32, t.float64) else field.to(t.float64)
            field = field.to(lab.device).contiguous()
            crit[k] = _lib.LabelCriterion(field.data_ptr(), _float_type(field), _lib.CMP_OPS[op], float(threshold))
        else:
            field = c.to(lab.device)
            field = (field.view(t.uint8) if field.dtype == t.bool else field if field.dtype == t.uint8 else (field != 0).view(t.uint8)).contiguous()
            crit[k] = _lib.LabelCriterion(field.data_ptr(), _lib.TF_U8, 0, 0.0)
        if tuple(field.shape) != tuple(lab.shape):
            raise ValueError("label_filter: a criterion must have the shape of the labels")
        keep.append(field)
    n = max(int(lab.max().item()), 0) if lab.numel() else 0
    if n == 0:
        return np.zeros(0, np.int64), np.zeros((0, K), bool), np.zeros(0, bool)
    rec = t.empty((n + 1, 4), dtype=t.int32, device=lab.device)
    _lib.check(_lib.lib().tf_label_filter(_lib.ptr(lab), T, H, W, n, crit, K, _lib.ptr(rec), _lib.stream_ptr()), "tf_label_filter")
    r = rec[1:].cpu().numpy().astype(np.int64)
    del keep
    present = r[:, 1] >= 0
    lengths = np.where(present, r[:, 1] - r[:, 0] + 1, 0)
    hits = ((r[:, 2:3] >> np.arange(K)[None, :]) & 1).astype(bool)
    return lengths, hits, present


def remap_labels(labels, locations):
    """utils.label_utils.remap_labels(labels, locations) for a boolean `locations` of length max label"""
    t = _lib.torch()
    lab = labels.to(t.int32).contiguous()
    locations = np.asarray(locations, bool)
    lut = np.zeros(locations.size + 1, np.int32)
    lut[1:][locations] = np.arange(1, int(locations.sum()) + 1)
    lut_t = t.from_numpy(lut).to(lab.device)
    out = t.empty_like(lab)
    _lib.check(_lib.lib().tf_apply_lut(_lib.ptr(lab), lab.numel(), _lib.ptr(lut_t), lut.size, _lib.ptr(out), _lib.stream_ptr()),
               "tf_apply_lut")
    return out


def label(x, structure=None):
    """scipy.ndimage.label(x, structure) -> (int32 labels tensor, n_labels).  `structure`: (3, 3, 3), symmetric;
    default = ndi.generate_binary_structure(3, 1)."""
    import ctypes
    import scipy.ndimage as ndi
    t = _lib.torch()
    L = _lib.lib()
    xb = _as_u8_mask(x)
    T, H, W = xb.shape
    st = _structure27(ndi.generate_binary_structure(3, 1) if structure is None else structure)
    out = t.empty((T, H, W), dtype=t.int32, device=xb.device)
    ws = _lib.workspace(L.tf_label_workspace_bytes(T, H, W), "label")
    n = ctypes.c_int(0)
    _lib.check(L.tf_label(_lib.ptr(xb), T, H, W, st.ctypes.data_as(_lib._P), _lib.ptr(out), ctypes.byref(n),
                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label")
    return out, n.value


def flat_label(mask, structure=None):
    """utils.label_utils.flat_label: components that never connect across the leading (time) axis"""
    import scipy.ndimage as ndi
    s = np.array(ndi.generate_binary_structure(3, 1) if structure is None else structure, bool).copy()
    s[0] = 0
    s[-1] = 0
    return label(mask, s)[0]


def _float_type(x):
    t = _lib.torch()
    if x.dtype == t.float32:
        return _lib.TF_F32
    if x.dtype == t.float64:
        return _lib.TF_F64
    raise TypeError(f"float32 or float64 tensor required, got {x.dtype}")


def gaussian_kernel1d(sigma, truncate=4.0):
    """(weights, radius) of scipy.ndimage.gaussian_filter1d(order=0): radius = int(truncate * sigma + 0.5),
    exp(-0.5 / sigma^2 * x^2) normalised to sum 1, float64"""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return np.ascontiguousarray(phi / phi.sum(), np.float64), radius


def gaussian_filter(x, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(x, sigma, mode='reflect', truncate=truncate) for a (T, H, W) float32 / float64
    device tensor: one symmetric correlate1d pass per axis with sigma > 1e-15, in axis order, each pass rounding to
    x's dtype (SciPy filters the later axes in place on the output of the earlier ones)."""
    t = _lib.torch()
    L = _lib.lib()
    ty = _float_type(x)
    sig = [float(v) for v in (sigma if np.ndim(sigma) else [sigma] * 3)]
    if x.dim() != 3 or len(sig) != 3:
        raise ValueError("gaussian_filter: a (T, H, W) tensor and a scalar or 3 sigmas are required")
    if any(v < 0 for v in sig):
        raise ValueError("gaussian_filter: sigma must be non-negative")
    cur = x.contiguous()
    T, H, W = cur.shape
    bufs = [None, None]
    k = 0
    for axis, sd in enumerate(sig):
        if sd <= 1e-15:
            continue
        w, r = gaussian_kernel1d(sd, truncate)
        if bufs[k] is None:
            bufs[k] = t.empty_like(cur)
        out = bufs[k]
        _lib.check(L.tf_correlate1d_sym(_lib.ptr(cur), ty, T, H, W, axis, w.ctypes.data_as(_lib._P), r, _lib.ptr(out),
                                        _lib.stream_ptr()), "tf_correlate1d_sym")
        cur, k = out, k ^ 1
    return cur.clone() if cur is x else cur


def _grey(x, footprint, op):
    t = _lib.torch()
    ty = _float_type(x)
    fp = np.asarray(footprint) != 0
    while fp.ndim < 3:
        fp = fp[np.newaxis]
    if fp.ndim != 3 or any(n not in (1, 3) for n in fp.shape):
        raise ValueError("footprint axes must have length 1 or 3")
    full = np.zeros((3, 3, 3), np.uint8)                     # centre the footprint in a 3x3x3 box
    full[tuple(slice(1, 2) if n == 1 else slice(0, 3) for n in fp.shape)] = fp
    if not np.array_equal(full, full[::-1, ::-1, ::-1]):
        raise ValueError("footprint must be point-symmetric (SciPy mirrors it for dilations)")
    if fp.all() and fp.size > 1:
        raise NotImplementedError("an all-true footprint takes SciPy's separable min/max path, whose NaN handling "
                                  "differs from the footprint path implemented here")
    xc = x.contiguous()
    T, H, W = xc.shape
    out = t.empty_like(xc)
    _lib.check(_lib.lib().tf_grey_morph(_lib.ptr(xc), ty, T, H, W, np.ascontiguousarray(full).ctypes.data_as(_lib._P), op,
                                        _lib.ptr(out), _lib.stream_ptr()), "tf_grey_morph")
    return out


def grey_erosion(x, footprint):
    """scipy.ndimage.grey_erosion(x, footprint=footprint) (flat footprint, mode 'reflect')"""
    return _grey(x, footprint, 0)


def grey_dilation(x, footprint):
    """scipy.ndimage.grey_dilation(x, footprint=footprint) (flat footprint, mode 'reflect')"""
    return _grey(x, footprint, 1)


def grey_opening(x, footprint):
    """scipy.ndimage.grey_opening(x, footprint=footprint): erosion then dilation"""
    return grey_dilation(grey_erosion(x, footprint), footprint)


def binary_fill_holes(x, structure):
    """scipy.ndimage.binary_fill_holes(x, structure): SciPy floods the background from outside the array
    (binary_dilation of the empty set, border_value 1, mask = ~x, to convergence) and returns what the flood does
    not reach.  Here: the background components (tf_label, same structure) that contain a pixel whose structure
    neighbourhood leaves the volume are 'outside'; every other background pixel is a hole."""
    t = _lib.torch()
    xb = x != 0
    bg = ~xb
    edge = binary_dilation(t.zeros_like(xb), structure, 1, border_value=1)      # one SciPy dilation step from outside
    lab, n = label(bg, structure)
    if n == 0:
        return xb.clone()
    # which components occur under `edge`: measured on the labels of those voxels alone, because the background is mostly ONE
    # component, and on a volume-filling label every lane of tf_label_filter queues at the same record (16 x 1500 x 2500:
    # 18 ms with the whole labelling and `edge & bg` as a criterion; profiles/label_extent_retired.txt)
    outside = np.zeros(n, bool)
    present = label_filter(lab * edge)[2]
    outside[:present.size] = present
    return ~(remap_labels(lab, outside) != 0)


def peak_local_max_2d(image, min_distance=1, threshold_abs=None):
    """skimage.feature.peak_local_max(image2d, min_distance=d, threshold_abs=threshold_abs) (scikit-image 0.18, every other
    argument at its default) for a 2-D float device tensor; returns the (n, 2) int64 numpy array
    utils.peak_utils.peak_local_max returns.
    The candidate mask (separable maximum filter, threshold = threshold_abs or the image minimum, border exclusion) is built
    on the GPU; the few candidates go to the host, where the SAME selection code as the host function orders and thins them."""
    import torch.nn.functional as F
    from tobac_flow_amd.utils.peak_utils import select_peaks
    t = _lib.torch()
    _float_type(image)
    if image.dim() != 2:
        raise ValueError("peak_local_max_2d: a 2-D tensor is required")
    d = int(min_distance)
    H, W = image.shape
    # NaN anywhere -> NaN threshold -> no peak, as in numpy
    threshold = image.min() if threshold_abs is None else float(threshold_abs)
    size = 2 * d + 1
    if size == 1 or image.numel() == 1:
        mask = image > threshold
    else:
        # maximum_filter(footprint = ones, mode = 'constant', cval = 0): zero padding, then max over the window
        padded = F.pad(image[None, None], (d, d, d, d), mode="constant", value=0.0)
        mx = F.max_pool2d(F.max_pool2d(padded, kernel_size=(1, size), stride=1), kernel_size=(size, 1), stride=1)[0, 0]
        mask = image == mx
        if bool(mask.all().item()):
            mask = t.zeros_like(mask)
        mask = mask & (image > threshold)
    if d:
        mask = mask.clone()
        mask[:d] = False
        mask[-d:] = False
        mask[:, :d] = False
        mask[:, -d:] = False
    coords = t.nonzero(mask)                                  # row-major, like np.nonzero
    vals = image[coords[:, 0], coords[:, 1]] if coords.shape[0] else image.new_zeros(0)
    return select_peaks(coords.cpu().numpy(), vals.cpu().numpy(), d)


_DISC_CACHE = {}


def within_distance(points, shape, radius, device):
    """scipy.ndimage.distance_transform_edt(~peaks) < radius for a 2-D frame whose only non-zero pixels are `points`
    ((n, 2) int array): squared distances are integers, so this is the union of the discs dy^2 + dx^2 < radius^2.
    A frame WITHOUT any point has no background for the transform; SciPy (1.7 and 1.15 alike) then returns
    sqrt((y + 1)^2 + x^2), i.e. the test marks a small corner at the origin -- reproduced as is."""
    t = _lib.torch()
    H, W = shape
    r2 = float(radius) ** 2
    out = t.zeros((H, W), dtype=t.bool, device=device)
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    if len(pts) == 0:
        yy = t.arange(H, device=device)[:, None] + 1
        xx = t.arange(W, device=device)[None, :]
        return (yy * yy + xx * xx).to(t.float64) < r2
    key = float(radius)
    if key not in _DISC_CACHE:
        k = int(np.ceil(radius))
        dy, dx = np.mgrid[-k:k + 1, -k:k + 1]
        keep = (dy * dy + dx * dx) < r2
        _DISC_CACHE[key] = np.stack([dy[keep], dx[keep]], 1).astype(np.int64)
    offs = _DISC_CACHE[key]
    cells = (pts[:, None, :] + offs[None, :, :]).reshape(-1, 2)
    ok = (cells[:, 0] >= 0) & (cells[:, 0] < H) & (cells[:, 1] >= 0) & (cells[:, 1] < W)
    cells = t.from_numpy(cells[ok]).to(device)
    out[cells[:, 0], cells[:, 1]] = True
    return out


def _edt_dtype(x):
    t = _lib.torch()
    return {t.uint8: _lib.TF_U8, t.bool: _lib.TF_U8, t.int32: _lib.TF_I32, t.float32: _lib.TF_F32, t.float64: _lib.TF_F64}.get(x.dtype)


def edt_squared_frames(features, return_nearest=False):
    """tf_edt2d_frames of a (T, H, W) device tensor whose non-zero voxels (NaN included) are the features: (d2, nearest),
    the int32 squared distance of every voxel to the nearest feature of its frame and (with return_nearest, else None) the
    int32 raveled index y' * W + x' of such a feature; INT32_MAX and -1 throughout a frame without features.  Of several
    equally near features the one with the smallest |x' - x| is reported, then the left one, then the upper one."""
    t = _lib.torch()
    L = _lib.lib()
    if features.dim() != 3 or 0 in features.shape:
        raise ValueError("a non-empty (T, H, W) volume is required")
    x = features if _edt_dtype(features) is not None else (features != 0)      # other integer widths: only != 0 matters
    x = x.contiguous()
    if x.dtype == t.bool:
        x = x.view(t.uint8)
    T, H, W = x.shape
    d2 = t.empty((T, H, W), dtype=t.int32, device=x.device)
    nearest = t.empty((T, H, W), dtype=t.int32, device=x.device) if return_nearest else None
    nbytes = L.tf_edt2d_frames_workspace_bytes(T, H, W)
    ws = _lib.workspace(nbytes, "edt") if nbytes else None                      # 0: a shape the entry point rejects with its reason
    _lib.check(L.tf_edt2d_frames(_lib.ptr(x), _edt_dtype(x), T, H, W, _lib.ptr(d2), _lib.ptr(nearest), _lib.ptr(ws),
                                 ws.numel() if ws is not None else 0, _lib.stream_ptr()), "tf_edt2d_frames")
    return d2, nearest


def edt_cylinder(d2, nearest, time_margin):
    """tf_edt_cylinder: (float64 distances, int64 source voxels or None) -- per voxel the square root of the smallest d2
    over the frames t - time_margin .. t + time_margin (inf where none has a feature) and, when `nearest` is given, the
    raveled index into the volume of the nearest feature of the earliest frame that holds the minimum (-1 where none)."""
    t = _lib.torch()
    T, H, W = d2.shape
    dist = t.empty((T, H, W), dtype=t.float64, device=d2.device)
    src = t.empty((T, H, W), dtype=t.int64, device=d2.device) if nearest is not None else None
    _lib.check(_lib.lib().tf_edt_cylinder(_lib.ptr(d2), _lib.ptr(nearest), T, H * W, int(time_margin), _lib.ptr(dist),
                                          _lib.ptr(src), _lib.stream_ptr()), "tf_edt_cylinder")
    return dist, src


def _count_grid(grid):
    """a flash grid as the validation kernels take it: float32, float64 or int32 and contiguous (bool and the narrower
    integers widen to int32, everything else to float64)"""
    t = _lib.torch()
    if grid.dtype in (t.bool, t.uint8, t.int8, t.int16):
        grid = grid.to(t.int32)
    elif grid.dtype not in (t.float32, t.float64, t.int32):
        grid = grid.to(t.float64)
    return grid.contiguous(), {t.float32: _lib.TF_F32, t.float64: _lib.TF_F64, t.int32: _lib.TF_I32}[grid.dtype]


def flash_tile():
    """the number of voxels one workgroup of tf_flash_count / tf_flash_list handles"""
    return int(_lib.lib().tf_flash_tile())


def flash_list(grid):
    """tf_flash_count + tf_flash_list: the int64 device tensor np.repeat(np.arange(n), grid.astype(int).ravel()) -- the
    raveled voxel of every flash of the flash-count device tensor `grid`, in order, a count truncated toward zero.
    ValueError, in np.repeat's words, for a negative or NaN count (tested before truncation), and a ValueError of its own
    for a count >= 2^31.  The total crosses to the host once, to size the list."""
    import ctypes
    t = _lib.torch()
    L = _lib.lib()
    g, dtype = _count_grid(grid)
    n = g.numel()
    if n == 0:
        return t.zeros(0, dtype=t.int64, device=g.device)
    ws = _lib.workspace(L.tf_flash_workspace_bytes(n), "flash_list")
    total, bad = ctypes.c_int64(0), ctypes.c_int(0)
    _lib.check(L.tf_flash_count(_lib.ptr(g), dtype, n, _lib.ptr(ws), ws.numel(), ctypes.byref(total), ctypes.byref(bad),
                                _lib.stream_ptr()), "tf_flash_count")
    if bad.value & 1:
        raise ValueError("repeats may not contain negative values (glm_grid holds a negative or NaN flash count)")
    if bad.value:
        raise ValueError("glm_grid holds a flash count of 2^31 or more: the list of its flashes cannot be held")
    voxel = t.empty(total.value, dtype=t.int64, device=g.device)
    _lib.check(L.tf_flash_list(_lib.ptr(g), dtype, n, _lib.ptr(ws), ws.numel(), _lib.ptr(voxel), total.value,
                               _lib.stream_ptr()), "tf_flash_list")
    return voxel


def edt_cylinder_at(d2, nearest, markers, time_margin, voxel, margin, get_closest=False):
    """tf_edt_cylinder_at: (float64 distances, int64 closest markers or None, int64 device scalar) -- edt_cylinder's
    distance gathered at the raveled voxels `voxel` (int64 device tensor), with get_closest the value of `markers` (the
    int32 volume d2 and nearest were made from) at the nearest feature of the earliest frame that holds the minimum (0 where
    there is none), and the number of entries whose distance is <= margin.  No volume is written."""
    t = _lib.torch()
    if d2.dim() != 3 or 0 in d2.shape or d2.dtype != t.int32:
        raise ValueError("d2 must be a non-empty (T, H, W) int32 tensor")
    if get_closest and (nearest is None or markers is None or markers.dtype != t.int32 or markers.shape != d2.shape or
                        nearest.shape != d2.shape or nearest.dtype != t.int32):
        raise ValueError("get_closest needs nearest and the int32 marker volume, both of d2's shape")
    if voxel.dtype != t.int64 or voxel.dim() != 1:
        raise ValueError("voxel must be a one-dimensional int64 tensor")
    T, H, W = d2.shape
    d2, voxel = d2.contiguous(), voxel.contiguous()
    n = voxel.numel()
    dist = t.empty(n, dtype=t.float64, device=d2.device)
    closest = t.empty(n, dtype=t.int64, device=d2.device) if get_closest else None
    within = t.empty((), dtype=t.int64, device=d2.device)
    _lib.check(_lib.lib().tf_edt_cylinder_at(_lib.ptr(d2), _lib.ptr(nearest.contiguous()) if get_closest else None,
                                             _lib.ptr(markers.contiguous()) if get_closest else None, T, H * W, int(time_margin),
                                             _lib.ptr(voxel), n, float(margin), _lib.ptr(dist), _lib.ptr(closest),
                                             _lib.ptr(within), _lib.stream_ptr()), "tf_edt_cylinder_at")
    return dist, closest, within


def edge_filter(grid, margin, time_margin, frame_off=None):
    """tf_grid_has_missing + tf_edge_filter: the bool (T, H, W) device tensor of validation.get_edge_filter for the flash
    grid `grid` (device tensor): False within time_margin frames of the ends and margin pixels of the borders, in the frames
    `frame_off` marks (T booleans, host or device), and where binary_dilation of grid == -1 with the reference's structure
    reaches.  Whether the grid holds a -1 crosses to the host once; without one the dilation is not run."""
    t = _lib.torch()
    L = _lib.lib()
    if grid.dim() != 3 or 0 in grid.shape:
        raise ValueError("a non-empty (T, H, W) grid is required")
    g, dtype = _count_grid(grid)
    T, H, W = g.shape
    off = None
    if frame_off is not None:
        off = _lib.to_dev(np.ascontiguousarray(_lib.to_host(frame_off) if _lib.is_tensor(frame_off) else frame_off, np.uint8))
        if off.numel() != T:
            raise ValueError(f"frame_off must hold one entry per frame ({T}), got {off.numel()}")
    flag = t.empty((), dtype=t.int32, device=g.device)
    _lib.check(L.tf_grid_has_missing(_lib.ptr(g), dtype, g.numel(), _lib.ptr(flag), _lib.stream_ptr()), "tf_grid_has_missing")
    missing = int(flag)
    nbytes = L.tf_edge_filter_workspace_bytes(T, H, W, missing)
    ws = _lib.workspace(nbytes, "edge_filter") if nbytes else None
    out = t.empty((T, H, W), dtype=t.uint8, device=g.device)
    _lib.check(L.tf_edge_filter(_lib.ptr(g), dtype, T, H, W, int(margin), int(time_margin), _lib.ptr(off), missing,
                                _lib.ptr(out), _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_ptr()),
               "tf_edge_filter")
    return out.view(t.bool)


def distance_transform_edt_frames(x, return_distances=True, return_indices=False):
    """scipy.ndimage.distance_transform_edt(x[t], return_distances=..., return_indices=...) for every frame t of a
    (T, H, W) device tensor: the float64 distance of every voxel to the nearest voxel of its frame where x == 0, and the
    (2, T, H, W) int32 row and column indices of that voxel.  Distances equal SciPy's bit for bit (an integer squared
    distance and one correctly rounded square root).  Where several zero voxels are equally near, the one with the
    smallest column distance is returned, then the left one, then the upper one; SciPy's choice among them follows its
    own sweep and may differ.  A frame with NO zero voxel returns inf and -1 (SciPy's result for such a frame is
    meaningless, and the reference guards against it with np.any).  Returns what SciPy returns: the distances, the
    indices, or the tuple of both."""
    if not (return_distances or return_indices):
        raise RuntimeError("at least one of return_distances/return_indices must be True")
    t = _lib.torch()
    d2, nearest = edt_squared_frames(x == 0, return_nearest=return_indices)
    out = []
    if return_distances:
        out.append(edt_cylinder(d2, None, 0)[0])
    if return_indices:
        W = x.shape[2]
        rows = t.div(nearest, W, rounding_mode="floor")
        out.append(t.stack([rows, t.where(nearest < 0, nearest, nearest - rows * W)]))
    return out[0] if len(out) == 1 else tuple(out)


def _sampling_t(sampling_t):
    s = float(sampling_t)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"the sampling along t must be finite and > 0, got {sampling_t!r}")
    return s


def edt_time_envelope(d2, nearest, sampling_t):
    """tf_edt_time_envelope: (float64 distances, int64 source voxels or None) of the 3-D transform with sampling
    (sampling_t, 1, 1) from the (T, H, W) outputs of edt_squared_frames -- per voxel the frame k with the smallest
    fl(fl((k - t) sampling_t)^2 + d2[k]) (of equal ones the nearer frame, then the earlier), the distance to that frame's
    nearest feature in SciPy's summation order, inf where no frame has a feature, and the raveled index of the feature in
    the volume (-1 where none).  With nearest=None the distance is the square root of that smallest sum itself, which is
    not SciPy's order of summation, and there are no source voxels."""
    t = _lib.torch()
    s = _sampling_t(sampling_t)
    if d2.dim() != 3 or 0 in d2.shape or d2.dtype != t.int32:
        raise ValueError("d2 must be a non-empty (T, H, W) int32 tensor")
    if nearest is not None and (nearest.shape != d2.shape or nearest.dtype != t.int32):
        raise ValueError("nearest must be an int32 tensor of d2's shape")
    d2 = d2.contiguous()
    nearest = nearest.contiguous() if nearest is not None else None
    T, H, W = d2.shape
    dist = t.empty((T, H, W), dtype=t.float64, device=d2.device)
    src = t.empty((T, H, W), dtype=t.int64, device=d2.device) if nearest is not None else None
    _lib.check(_lib.lib().tf_edt_time_envelope(_lib.ptr(d2), _lib.ptr(nearest), T, H, W, s, _lib.ptr(dist), _lib.ptr(src),
                                               _lib.stream_ptr()), "tf_edt_time_envelope")
    return dist, src


def _edt_sampling(sampling, ndim):
    """the sampling along t of distance_transform_edt; every in-plane sampling must be 1"""
    if sampling is None:
        return 1.0
    s = np.asarray(sampling, np.float64)
    if s.ndim == 0:
        s = np.full(ndim, float(s))
    if s.shape != (ndim,):
        raise ValueError(f"sampling must be a scalar or one value per axis ({ndim}), got {sampling!r}")
    if not np.all(s[-2:] == 1):
        raise ValueError("distance_transform_edt: only the leading (time) axis of a (T, H, W) input may have a sampling "
                         f"other than 1 -- the in-plane transform is the integer one -- got {sampling!r}")
    return _sampling_t(s[0]) if ndim == 3 else 1.0


def distance_transform_edt(x, sampling=None, return_distances=True, return_indices=False):
    """scipy.ndimage.distance_transform_edt(x, sampling=sampling, return_distances=..., return_indices=...) for a (H, W)
    or (T, H, W) device tensor: the float64 distance of every voxel to the nearest voxel where x == 0 and the (ndim, ...)
    int32 indices of that voxel.  `sampling` is None, 1, or for a volume (s_t, 1, 1) with s_t finite and > 0: the in-plane
    transform is the exact integer one (edt_squared_frames), the time axis is its lower envelope (edt_time_envelope), and
    the distance is SciPy's expression for the reported voxel.  It equals SciPy's bit for bit wherever the nearest zero
    voxel is unique, and everywhere for an integer s_t; of several equally near ones this function reports the nearer
    frame, then the earlier one, and within a frame the one edt_squared_frames reports, SciPy the one its sweep meets.
    An input without any zero voxel gives inf and -1 (SciPy's result for it is meaningless).  Returns what SciPy returns:
    the distances, the indices, or the tuple of both."""
    if not (return_distances or return_indices):
        raise RuntimeError("at least one of return_distances/return_indices must be True")
    ndim = len(x.shape)
    if ndim not in (2, 3) or 0 in x.shape:
        raise ValueError(f"a non-empty (H, W) or (T, H, W) tensor is required, got shape {tuple(x.shape)}")
    s = _edt_sampling(sampling, ndim)
    if ndim == 2:
        out = distance_transform_edt_frames(x[None], return_distances, return_indices)
        if return_distances and return_indices:
            return out[0][0], out[1][:, 0]
        return out[:, 0] if return_indices else out[0]
    t = _lib.torch()
    d2, nearest = edt_squared_frames(x == 0, return_nearest=True)       # the distance is evaluated at the feature: SciPy's order
    dist, src = edt_time_envelope(d2, nearest, s)
    if not return_indices:
        return dist
    H, W = x.shape[1:]
    frame = t.div(src, H * W, rounding_mode="floor")
    rest = src - frame * (H * W)
    row = t.div(rest, W, rounding_mode="floor")
    indices = t.stack([frame, row, rest - row * W]).to(t.int32)
    indices[:, src < 0] = -1
    return (dist, indices) if return_distances else indices


def label_nanmin(labels, field, ids):
    """tf_label_nanmin: (float64 minima, int64 counts) for the label ids `ids` (a 1-D int64 numpy array, every id >= 1):
    np.nanmin of `field` (bool, uint8, float32 or float64 device tensor; other types are widened to float64) over the
    voxels of each label of the int32 device tensor `labels`; NaN where the label has no non-NaN voxel; the count of
    non-NaN voxels, -1 where the label has no voxel at all."""
    t = _lib.torch()
    L = _lib.lib()
    if tuple(labels.shape) != tuple(field.shape):
        raise ValueError(f"labels {tuple(labels.shape)} and field {tuple(field.shape)} do not have the same shape")
    ids = np.ascontiguousarray(ids, np.int64)
    n_ids = ids.size
    mins = t.full((n_ids,), float("nan"), dtype=t.float64, device=labels.device)
    counts = t.full((n_ids,), -1, dtype=t.int64, device=labels.device)
    if n_ids == 0 or labels.numel() == 0:
        return mins, counts
    lab = labels.to(t.int32).contiguous()
    f = field.contiguous()
    if f.dtype == t.bool:
        f = f.view(t.uint8)
    elif f.dtype not in (t.uint8, t.float32, t.float64):
        f = f.to(t.float64)
    dtype = {t.uint8: _lib.TF_U8, t.float32: _lib.TF_F32, t.float64: _lib.TF_F64}[f.dtype]
    top = int(ids.max())
    n_labels = top if top <= lab.numel() else min(top, int(lab.max()))         # ids beyond the largest label have no voxel
    if n_labels < 1:
        return mins, counts
    ids_t = t.from_numpy(ids).to(labels.device)
    ws = _lib.workspace(L.tf_label_nanmin_workspace_bytes(n_labels), "label_nanmin")
    _lib.check(L.tf_label_nanmin(_lib.ptr(lab), _lib.ptr(f), dtype, lab.numel(), n_labels, _lib.ptr(ids_t), n_ids,
                                 _lib.ptr(mins), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "tf_label_nanmin")
    return mins, counts


# ---- generic per-label reductions (tf_label_reduce, tf_label_order) ----------------------------------------------------
LABEL_REDUCE_OPS = ("size", "count", "nonzero", "sum", "min", "max", "ssd")
_INT32_MIN, _INT32_MAX, _LABEL_REDUCE_MAX_SPAN = -2 ** 31, 2 ** 31 - 1, 2 ** 27


def _reduce_operands(labels, field):
    """(labels int32 (n,), field, TF dtype, layout, T, hw) for tf_label_reduce / tf_label_order.  The field keeps its
    dtype where the kernels take it (bool as its bytes; narrower integers and floats are widened exactly to int32 /
    float32) and its layout: a volume, one plane that every frame shares (leading axes of length 1) or one value per
    frame (trailing axes of length 1); any other broadcast is materialised."""
    t = _lib.torch()
    if field.dtype == t.bool:
        field = field.view(t.uint8) if field.is_contiguous() else field.to(t.uint8)
    elif field.dtype in (t.int8, t.int16):
        field = field.to(t.int32)
    elif field.dtype in (t.float16, t.bfloat16):
        field = field.to(t.float32)
    elif field.dtype not in (t.uint8, t.int32, t.float32, t.float64):
        raise TypeError(f"per-label reductions on the GPU take bool, (u)int8, int16, int32, float16, float32 and float64 "
                        f"fields, not {field.dtype}: pass NumPy arrays for the host path")
    shape = tuple(t.broadcast_shapes(tuple(labels.shape), tuple(field.shape)))
    if tuple(labels.shape) != shape:
        labels = labels.expand(shape)
    lab = labels.to(t.int32).contiguous().reshape(-1)
    n = lab.numel()
    fs = (1,) * (len(shape) - field.dim()) + tuple(field.shape)
    code = {t.uint8: _lib.TF_U8, t.int32: _lib.TF_I32, t.float32: _lib.TF_F32, t.float64: _lib.TF_F64}[field.dtype]
    if fs != shape and n:
        for k in range(1, len(shape)):
            hw = int(np.prod(shape[k:]))
            if all(s == 1 for s in fs[:k]) and fs[k:] == shape[k:]:
                return lab, field.contiguous().reshape(-1), code, 1, n // hw, hw
            if fs[:k] == shape[:k] and all(s == 1 for s in fs[k:]):
                return lab, field.contiguous().reshape(-1), code, 2, n // hw, hw
        field = field.expand(shape)
    return lab, field.contiguous().reshape(-1), code, 0, 1, n


def _id_span(ids):
    """(ids as int64, lo, hi) of the ids a label volume can hold; (ids, None, None) when there is none"""
    ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
    if (ids == _INT32_MIN).any():
        raise ValueError("per-label reductions on the GPU take label ids above INT32_MIN")
    held = ids[(ids > _INT32_MIN) & (ids <= _INT32_MAX)]
    return (ids, int(held.min()), int(held.max())) if held.size else (ids, None, None)


def label_records(labels, field, lo, hi, var=False, order=False):
    """tf_label_reduce over the id span [lo, hi]: the (hi - lo + 1, 8) int64 device tensor of 64-byte records of
    include/tobac_flow_hip.h (slot 3 of a float field and slot 6 hold the bits of doubles: .view(torch.float64)); with
    `var` slot 6 is filled (a second read of the volume).  With `order` also tf_label_order's (hi - lo + 1, 2) float64
    tensor of the two middle values.  A span of 2^27 ids or more is refused by the library before anything is allocated
    or launched (ValueError)."""
    t = _lib.torch()
    L = _lib.lib()
    lab, f, code, layout, T, hw = _reduce_operands(labels, field)
    if lab.numel() == 0:
        raise ValueError("per-label reductions need at least one voxel")
    want = 1 if var else 0
    args = (_lib.ptr(lab), _lib.ptr(f), code, layout, T, hw, lo, hi)
    if hi - lo >= _LABEL_REDUCE_MAX_SPAN or lo <= _INT32_MIN or hi > _INT32_MAX or lo > hi:
        _lib.check(L.tf_label_reduce(*args, want, None, None, 0, _lib.stream_ptr()), "tf_label_reduce")
        raise ValueError("tf_label_reduce: bad span")                  # not reached: the library refuses such a span
    rec = _lib.empty((hi - lo + 1, 8), t.int64)
    ws = _lib.workspace(L.tf_label_reduce_workspace_bytes(lo, hi), "label_reduce") if var else None
    _lib.check(L.tf_label_reduce(*args, want, _lib.ptr(rec), _lib.ptr(ws), ws.numel() if var else 0, _lib.stream_ptr()),
               "tf_label_reduce")
    if not order:
        return rec
    n_keys = int(rec[:, 1].sum())
    mid = _lib.empty((hi - lo + 1, 2), t.float64)
    ws = _lib.workspace(L.tf_label_order_workspace_bytes(lo, hi, n_keys, code), "label_order")
    _lib.check(L.tf_label_order(*args, _lib.ptr(rec), n_keys, _lib.ptr(mid), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "tf_label_order")
    return rec, mid


def _unkey(k):
    """the double behind an order key of slots 4 / 5 (int64 view of the unsigned key)"""
    t = _lib.torch()
    return t.where(k < 0, k & 0x7fffffffffffffff, ~k).view(t.float64)


def label_reduce(labels, field, ids, ops=("size", "sum")):
    """tf_label_reduce: per label id of `ids` (any int64 sequence: unsorted, with duplicates, with ids that do not occur;
    0 and negative ids are regions like any other) the quantities named in `ops`, as a dict of device tensors (len(ids),):
      "size" voxels, "count" voxels whose value is not NaN, "nonzero" voxels whose value is != 0 (NaN among them): int64
      "sum"  of the non-NaN values: float64 for a float field (last bits depend on arrival order), int64 (exact) otherwise
      "min", "max" of the non-NaN values, exact: float64, NaN where there is none
      "ssd"  sum of (x - mean)^2 over the non-NaN values about mean = sum / count, float64 (a second read of the volume)
    `labels` is an integer device tensor, `field` a device tensor that broadcasts against it (_reduce_operands).  The
    library works on the span [min(ids), max(ids)]: 64 B per id of it, below 2^27 ids (ValueError beyond)."""
    t = _lib.torch()
    ops = tuple(ops)
    unknown = [o for o in ops if o not in LABEL_REDUCE_OPS]
    if unknown:
        raise ValueError(f"unknown ops {unknown}: one of {LABEL_REDUCE_OPS}")
    ids, lo, hi = _id_span(ids)
    integer = not field.dtype.is_floating_point
    kinds = {"size": t.int64, "count": t.int64, "nonzero": t.int64, "sum": t.int64 if integer else t.float64}
    out = {o: t.zeros((ids.size,), dtype=kinds.get(o, t.float64), device=labels.device) for o in ops}
    for o in ("min", "max"):
        if o in out:
            out[o] += float("nan")
    if lo is None:
        return out
    rec = label_records(labels, field, lo, hi, var="ssd" in ops)
    held = (ids > _INT32_MIN) & (ids <= _INT32_MAX)
    at = t.from_numpy(np.where(held, ids - lo, 0)).to(rec.device)
    r = rec[at] * t.from_numpy(held.astype(np.int64)).to(rec.device)[:, None]          # ids no volume can hold: zeros
    some = r[:, 1] > 0
    nan = t.full((ids.size,), float("nan"), dtype=t.float64, device=rec.device)
    take = {"size": lambda: r[:, 0], "count": lambda: r[:, 1], "nonzero": lambda: r[:, 2],
            "sum": lambda: r[:, 3] if integer else r[:, 3].contiguous().view(t.float64),
            "min": lambda: t.where(some, _unkey(r[:, 4].contiguous()), nan),
            "max": lambda: t.where(some, _unkey(r[:, 5].contiguous()), nan),
            "ssd": lambda: r[:, 6].contiguous().view(t.float64)}
    return {o: take[o]() for o in ops}


def label_order(labels, field, ids):
    """tf_label_order: (len(ids), 2) float64 device tensor of the two middle values of each label's non-NaN values in
    ascending order (equal for an odd count, NaN for a label without such a value): np.median's operands.  Exact; a zero
    comes back as +0.0.  Operands and limits as label_reduce."""
    t = _lib.torch()
    ids, lo, hi = _id_span(ids)
    out = t.full((ids.size, 2), float("nan"), dtype=t.float64, device=labels.device)
    if lo is None:
        return out
    _, mid = label_records(labels, field, lo, hi, order=True)
    held = (ids > _INT32_MIN) & (ids <= _INT32_MAX)
    got = mid[t.from_numpy(np.where(held, ids - lo, 0)).to(mid.device)]
    return t.where(t.from_numpy(held).to(mid.device)[:, None], got, out)


# ---- field statistics (tf_field_stats) ---------------------------------------------------------------------------------
class _FramesByDtype(dict):
    """read-only {dtype name: frames}; looked up by a torch dtype, a NumPy dtype or a name"""

    def __getitem__(self, dtype):
        return dict.__getitem__(self, str(getattr(dtype, "name", dtype)).replace("torch.", ""))

    def _read_only(self, *args, **kwargs):
        raise TypeError("FIELD_STATS_LDS_FRAMES is a constant")

    __setitem__ = __delitem__ = clear = pop = popitem = setdefault = update = _read_only


# the largest T of which tf_field_stats' per-pixel form keeps a workgroup's tile in LDS and reads the volume once
# (TF_FIELD_STATS_LDS_FRAMES_F32 / _F64 of include/tobac_flow_hip.h)
FIELD_STATS_LDS_FRAMES = _FramesByDtype(float32=64, float64=32)
FIELD_STATS_OVER = {"all": 0, "frame": 1, "time": 2}


def field_stats(x, over="all"):
    """tf_field_stats: the statistics of get_bulk_stats / get_spatial_stats / get_temporal_stats (dataset.py) of a float32
    or float64 device tensor, NaN values ignored, as a dict of device tensors: `count` (int64, the non-NaN values of each
    slice) and `mean`, `std` (ddof 0), `median`, `max`, `min` (float64).  over="all": one slice, results of shape (), any
    shape of `x`, and the median is np.median's (NaN if any value is NaN); "frame": (t, y, x) -> (t,); "time": (t, y, x) ->
    (y, x).  Count, median, max and min are exact -- the median is computed in the dtype of `x` and widened --; mean and std
    are float64 sums with identical bits from run to run.  A slice without a non-NaN value gives NaN five times.  Any view
    is made contiguous first.  An empty tensor is a ValueError, another dtype a TypeError."""
    t = _lib.torch()
    if over not in FIELD_STATS_OVER:
        raise ValueError(f"over must be one of {tuple(FIELD_STATS_OVER)}, not {over!r}")
    if x.dtype not in (t.float32, t.float64):
        raise TypeError(f"field statistics on the GPU take torch.float32 and torch.float64 tensors, not {x.dtype}: "
                        "pass a NumPy array for the host path")
    if x.numel() == 0:
        raise ValueError("field statistics need at least one value")
    if over == "all":
        T, H, W, shape = 1, 1, x.numel(), ()
    else:
        if x.dim() != 3:
            raise ValueError(f"over={over!r} takes a (t, y, x) volume, not {tuple(x.shape)}")
        T, H, W = (int(n) for n in x.shape)
        shape = (T,) if over == "frame" else (H, W)
    L = _lib.lib()
    x = _lib.to_dev(x)
    code = _lib.TF_F32 if x.dtype == t.float32 else _lib.TF_F64
    S = int(np.prod(shape, dtype=np.int64))
    count, stats = _lib.empty((S,), t.int64), _lib.empty((5, S), t.float64)
    ws = _lib.workspace(L.tf_field_stats_workspace_bytes(code, T, H, W, FIELD_STATS_OVER[over]), "field_stats")
    _lib.check(L.tf_field_stats(_lib.ptr(x), code, T, H, W, FIELD_STATS_OVER[over], _lib.ptr(count), _lib.ptr(stats),
                                _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_field_stats")
    out = {"count": count.reshape(shape)}
    out.update((name, stats[k].reshape(shape)) for k, name in enumerate(("mean", "std", "median", "max", "min")))
    return out
