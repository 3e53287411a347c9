"""Semi-Lagrangian convolution on the MI355X.

Mirrors /root/reference/tobac_flow/convolve.py (same names, arguments, defaults, exceptions);
the three cv2.remap-based stages (warp_flow :8-86, convolve_same_step :89-144, convolve_step
:147-245) run as ONE fused HIP gather (tf_convolve, include/tobac_flow_hip.h) and the callables the
reference itself passes as `func` are reduced inside that kernel.  Any other Python callable
still works: the (n_struct, H, W) stack is gathered on the GPU and `func` is applied on the host
per frame, exactly like convolve.py:305-347.

The three stages are also callable by name, for a caller that runs its own time loop (a streaming
detector that holds three frames, the reference's own loop): `warp_flow`, `convolve_same_step` and
`convolve_step` take what the reference's functions take -- separate frames, an image that is a
crop of the flow's frame or larger than it, `grid_locs` in full-frame coordinates, float offsets, a
(3, m, n) structure -- and run as tf_warp_offsets / tf_gather_offsets / tf_convolve_step.  They
accept numpy arrays or device tensors and return the same kind; their deviations from the reference
(float64 images sampled in float32, integer-valued `grid_locs` and same-step offsets only) are
named in their docstrings.
"""
import functools
from typing import Callable

import numpy as np
import scipy.ndimage as ndi

from tobac_flow_amd import _lib

_METHODS = ("nearest", "linear", "cubic", "lanczos")


def tag_func(code):
    """Mark a numpy callable as having a fused GPU implementation (tf_convolve `func` code)."""
    def deco(f):
        f._tf_func = code
        return f
    return deco


def _func_code(func):
    if func is None:
        return _lib.FUNC_STACK
    code = getattr(func, "_tf_func", None)
    if code is not None:
        return code
    if isinstance(func, functools.partial) and func.func is np.any and not func.args \
            and func.keywords == {"axis": 0}:
        return _lib.FUNC_ANY       # detection.py:313-320
    return None


def _check_method(method, structure):
    if method not in _METHODS:
        raise ValueError(f"method must be one of {list(_METHODS)}")


def _np_dtype(dtype):
    return np.dtype(np.float64 if dtype is None else dtype)


def convolve_dev(data, fwd, bwd, structure, method, dtype, fill_value, func_code, t0=0, t1=None, out=None):
    """Device-resident core: `data`, `fwd`, `bwd` are torch tensors on the GPU.

    Returns a torch tensor: (n_struct, T, H, W) for FUNC_STACK else (T, H, W) (frames outside
    [t0, t1) are left untouched / unspecified).
    """
    t = _lib.torch()
    L = _lib.lib()
    T, H, W = data.shape
    if t1 is None:
        t1 = T
    nd = _np_dtype(dtype)
    if data.dtype in (t.int32, t.int64, t.int16, t.int8, t.uint8, t.bool):
        data = data.to(t.int32)            # cv2 casts int64 images to CV_32S (remap: nearest only)
        dt_code = _lib.TF_I32
        if method != "nearest":
            raise ValueError("integer data can only be warped with method='nearest'")
    else:
        data = data.to(t.float32)
        dt_code = _lib.TF_F32
    if nd == np.float32:
        out_code, tdt = _lib.TF_F32, t.float32
    elif nd == np.float64:
        out_code, tdt = _lib.TF_F64, t.float64
    elif nd == np.int32:
        out_code, tdt = _lib.TF_I32, t.int32
    else:
        raise ValueError(f"dtype {nd} is not supported on the GPU path (float32, float64, int32)")
    struct = np.ascontiguousarray(np.asarray(structure) != 0, dtype=np.uint8)
    n_struct = int(struct.sum())
    shape = (n_struct, T, H, W) if func_code == _lib.FUNC_STACK else (T, H, W)
    if out is None:
        out = _lib.empty(shape, tdt)
    fill = float(fill_value)
    rc = L.tf_convolve(_lib.ptr(data), dt_code, T, H, W, _lib.ptr(fwd), _lib.ptr(bwd),
                       struct.ctypes.data_as(_lib._P), _lib.INTERP[method], fill, func_code,
                       _lib.ptr(out), out_code, t0, t1, _lib.stream_ptr())
    _lib.check(rc, "tf_convolve")
    return out


def convolve(
    data: np.ndarray,
    forward_flow: np.ndarray,
    backward_flow: np.ndarray,
    structure: np.ndarray = ndi.generate_binary_structure(3, 1),
    method: str = "linear",
    dtype: type = np.float32,
    fill_value: float = np.nan,
    func: Callable | None = None,
    _dev_flows=None,
) -> np.ndarray:
    """Convolve a sequence of images using optical flow vectors to offset adjacent elements in
    the leading dimension (reference: convolve.py:248-348)."""
    assert structure.shape == (3, 3, 3), "Structure input must be a 3x3x3 array"
    t = _lib.torch()
    if hasattr(data, "to_numpy") and not isinstance(data, np.ndarray) and not isinstance(data, t.Tensor):
        data = data.to_numpy()                                  # xr.DataArray
    _check_method(method, structure)
    on_device = isinstance(data, t.Tensor)
    d = _lib.to_dev(data)
    if d.dtype == t.float64:
        d = d.to(t.float32)        # documented deviation: cv2 would remap a float64 image in double
    if _dev_flows is not None:
        fwd, bwd = _dev_flows
    else:
        fwd, bwd = _lib.to_dev(forward_flow, t.float32), _lib.to_dev(backward_flow, t.float32)
    nd = _np_dtype(dtype)
    code = _func_code(func)
    T, H, W = d.shape
    if code is not None:
        out = convolve_dev(d, fwd, bwd, structure, method, nd, fill_value, code)
        return out if on_device else _lib.to_host(out)
    # arbitrary Python callable: gather the stack on the GPU frame by frame, reduce on the host
    data_np = d.cpu().numpy() if on_device else np.asarray(data)
    res = np.full(data_np.shape, fill_value, dtype=nd)
    for i in range(T):
        # a 3-frame window keeps the true sequence ends: frame -1 / T are all-fill (convolve.py:307-314)
        lo, hi = max(i - 1, 0), min(i + 2, T)
        st = convolve_dev(d[lo:hi], fwd[lo:hi], bwd[lo:hi], structure, method, nd, fill_value,
                          _lib.FUNC_STACK, t0=i - lo, t1=i - lo + 1)
        res[i] = func(st[:, i - lo].cpu().numpy())
    if np.issubdtype(data_np.dtype, np.floating):
        res[np.isnan(data_np)] = fill_value
    return _lib.to_dev(res) if on_device else res


# ---- step-level functions (convolve.py:8-245) -------------------------------------------------------
_OUT_CODES = {np.dtype(np.float32): _lib.TF_F32, np.dtype(np.float64): _lib.TF_F64, np.dtype(np.int32): _lib.TF_I32}


def _np_of(x):
    """dtype of a numpy array / array-like / torch tensor as a numpy dtype"""
    if isinstance(x, _lib.torch().Tensor):
        return np.dtype(str(x.dtype).replace("torch.", ""))
    return np.asarray(x).dtype


def _is_int(dt):
    return dt.kind in "iub"


def _check_grid(grid_locs, shape):
    """grid_locs validated BEFORE any device work: (rows, cols, 2), integer-valued, within int32"""
    if grid_locs is None:
        return
    if tuple(grid_locs.shape) != tuple(shape) + (2,):
        raise ValueError(f"grid_locs must have shape {tuple(shape) + (2,)}, not {tuple(grid_locs.shape)}")
    t = _lib.torch()
    if isinstance(grid_locs, t.Tensor):                 # checked where it lives: no copy of a full-frame grid to the host
        if grid_locs.dtype == t.int32:
            return
        g, integral = grid_locs, (lambda a: bool((a == a.round()).all()))
        floating = g.dtype.is_floating_point
        integer = not floating and not g.dtype.is_complex
    else:
        g, integral = np.asarray(grid_locs), (lambda a: bool(np.all(a == np.rint(a))))
        floating, integer = g.dtype.kind == "f", _is_int(g.dtype)
    if not (integer or (floating and integral(g))):     # NaN / inf fail too
        raise ValueError("grid_locs must hold integer values")
    if g.shape[0] and g.shape[1] and (g.min() < -2 ** 31 or g.max() >= 2 ** 31):
        raise ValueError("grid_locs must fit a 32-bit integer")


def _grid_dev(grid_locs):
    if grid_locs is None:
        return None
    t = _lib.torch()
    if not isinstance(grid_locs, t.Tensor):
        grid_locs = np.ascontiguousarray(grid_locs).astype(np.int32)
    return _lib.to_dev(grid_locs, t.int32)


def _image_kind(dtypes, method):
    """TF_I32 when every image is of an integer type (cv2 remaps those as CV_32S, nearest only), else TF_F32"""
    if all(_is_int(d) for d in dtypes):
        if method != "nearest":
            raise ValueError("integer data can only be warped with method='nearest'")
        return _lib.TF_I32
    return _lib.TF_F32


def _image_dev(img, code):
    t = _lib.torch()
    return _lib.to_dev(img, t.int32 if code == _lib.TF_I32 else t.float32)   # float64 -> float32: documented deviation


def _check_fill(code, fill_value):
    if code == _lib.TF_I32 and not np.isfinite(fill_value):
        raise ValueError("cannot convert a non-finite fill_value to integer data")


def _torch_dtype(nd):
    t = _lib.torch()
    return {np.dtype(np.float32): t.float32, np.dtype(np.float64): t.float64, np.dtype(np.int32): t.int32}[nd]


def _result(shape, native, res):
    """(tensor the kernels write, its numpy dtype): `res` itself when it is a device tensor the library can write"""
    t = _lib.torch()
    if isinstance(res, t.Tensor) and res.is_cuda and res.is_contiguous() and tuple(res.shape) == tuple(shape) \
            and _np_of(res) in _OUT_CODES:
        return res, _np_of(res)
    return _lib.empty(tuple(shape), _torch_dtype(native)), native


def _deliver(out, res, on_device):
    """hand `out` back in the caller's container; with res= the values go into it (cast to its dtype)"""
    t = _lib.torch()
    if res is None:
        return out if on_device else _lib.to_host(out)
    if res is out:
        return res
    if isinstance(res, t.Tensor):
        res.view(out.shape).copy_(out)                  # .view: raises rather than writing into a copy
    else:
        view = res.reshape(tuple(out.shape))
        if not np.shares_memory(view, res):
            raise ValueError("res cannot take the result's shape without a copy")
        view[...] = _lib.to_host(out)
    return res


def _check_res(res, shape):
    if res is not None and int(np.prod(res.shape)) != int(np.prod(shape)):
        raise ValueError(f"res has shape {tuple(res.shape)}, the result has shape {tuple(shape)}")


def warp_flow(
    img: np.ndarray,
    flow: np.ndarray,
    method: str = "linear",
    fill_value: float = np.nan,
    offsets: np.ndarray = np.array([[0, 0]]),
    res: np.ndarray | None = None,
    grid_locs: np.ndarray | None = None,
) -> np.ndarray:
    """Warp an image according to a set of optical flow vectors, to every one of a list of (x, y) `offsets` at once
    (reference: convolve.py:8-86).  Returns (K, H, W) with (H, W) = flow.shape[:2]; `img` may have another shape
    (a crop, or a frame larger than the flow) and `grid_locs` (H, W, 2) gives the (x, y) position of every output
    pixel in the image's coordinates (default: the pixel index).

    numpy arrays in, numpy array out; device tensors in, device tensor out.  With `res=` the result is written into
    it (cast to its dtype) and `res` is returned.

    Deviations: a float64 image is sampled in float32 (like `convolve`); float images return float32, integer images
    (method="nearest" only, else ValueError) int32; `grid_locs` must hold integer values -- a floating array is
    accepted if it is integral, otherwise ValueError (the reference would add the fractions to the coordinates)."""
    if method not in _METHODS:
        raise ValueError(f"method must be one of {list(_METHODS)}")
    t = _lib.torch()
    on_device = isinstance(img, t.Tensor)
    if img.ndim != 2 or flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("img must have shape (h, w) and flow shape (H, W, 2)")
    H, W = int(flow.shape[0]), int(flow.shape[1])
    offs = offsets.detach().cpu().numpy() if isinstance(offsets, t.Tensor) else np.asarray(offsets)
    offs = np.ascontiguousarray(np.atleast_2d(offs).astype(np.float32))
    if offs.ndim != 2 or offs.shape[1] != 2:
        raise ValueError("offsets must have shape (K, 2)")
    K = offs.shape[0]
    _check_grid(grid_locs, (H, W))
    code = _image_kind([_np_of(img)], method)
    _check_fill(code, fill_value)
    _check_res(res, (K, H, W))
    native = np.dtype(np.int32 if code == _lib.TF_I32 else np.float32)
    if K == 0:
        return _deliver(_lib.empty((0, H, W), _torch_dtype(native)), res, on_device)
    d, f, g = _image_dev(img, code), _lib.to_dev(flow, t.float32), _grid_dev(grid_locs)
    out, odt = _result((K, H, W), native, res)
    rc = _lib.lib().tf_warp_offsets(_lib.ptr(d), code, d.shape[0], d.shape[1], _lib.ptr(f), _lib.ptr(g), H, W,
                                    offs.ctypes.data_as(_lib._P), K, _lib.INTERP[method], float(fill_value),
                                    _lib.ptr(out), _OUT_CODES[odt], _lib.stream_ptr())
    _lib.check(rc, "tf_warp_offsets")
    return _deliver(out, res, on_device)


def convolve_same_step(
    img: np.ndarray,
    offsets: np.ndarray,
    fill_value: float = np.nan,
    res: np.ndarray | None = None,
    grid_locs: np.ndarray | None = None,
) -> np.ndarray:
    """Gather an image at a list of integer (x, y) `offsets` from every pixel; taps outside the image take
    `fill_value` (reference: convolve.py:89-144).  Returns (K, h, w), or (K,) + grid_locs.shape[:2] with `grid_locs`.

    numpy arrays in, numpy array out; device tensors in, device tensor out; `res=` is written and returned.

    Deviations: `offsets` must be integer-valued, a non-integral offset raises ValueError -- the reference truncates
    the SUM of pixel index and offset without `grid_locs` but the offset alone with it, so that negative fractions
    land on different pixels in the two forms; `grid_locs` must hold integer values (ValueError otherwise); float
    images return float32, integer images int32."""
    t = _lib.torch()
    on_device = isinstance(img, t.Tensor)
    if img.ndim != 2:
        raise ValueError("img must have shape (h, w)")
    h, w = int(img.shape[0]), int(img.shape[1])
    offs = offsets.detach().cpu().numpy() if isinstance(offsets, t.Tensor) else np.asarray(offsets)
    offs = np.atleast_2d(offs)
    if offs.ndim != 2 or offs.shape[1] != 2:
        raise ValueError("offsets must have shape (K, 2)")
    if not _is_int(offs.dtype) and not (offs.dtype.kind == "f" and np.all(offs == np.rint(offs))):
        raise ValueError("offsets must be integer-valued")
    if offs.size and np.abs(offs).max() >= 2 ** 31:
        raise ValueError("offsets must fit a 32-bit integer")
    offs = np.ascontiguousarray(offs.astype(np.int32))
    K = offs.shape[0]
    rows, cols = (h, w) if grid_locs is None else (int(grid_locs.shape[0]), int(grid_locs.shape[1]))
    _check_grid(grid_locs, (rows, cols))
    code = _image_kind([_np_of(img)], "nearest")
    _check_fill(code, fill_value)
    _check_res(res, (K, rows, cols))
    native = np.dtype(np.int32 if code == _lib.TF_I32 else np.float32)
    if K == 0:
        return _deliver(_lib.empty((0, rows, cols), _torch_dtype(native)), res, on_device)
    d, g = _image_dev(img, code), _grid_dev(grid_locs)
    out, odt = _result((K, rows, cols), native, res)
    rc = _lib.lib().tf_gather_offsets(_lib.ptr(d), code, h, w, _lib.ptr(g), rows, cols, offs.ctypes.data_as(_lib._P), K,
                                      float(fill_value), _lib.ptr(out), _OUT_CODES[odt], _lib.stream_ptr())
    _lib.check(rc, "tf_gather_offsets")
    return _deliver(out, res, on_device)


def convolve_step(
    prev_step: np.ndarray,
    same_step: np.ndarray,
    next_step: np.ndarray,
    forward_flow: np.ndarray,
    backward_flow: np.ndarray,
    structure: np.ndarray = ndi.generate_binary_structure(3, 1),
    method: str = "linear",
    dtype: type = np.float32,
    fill_value: float = np.nan,
    res: np.ndarray | None = None,
    grid_locs: np.ndarray | None = None,
) -> np.ndarray:
    """Convolve one time step: the (n_struct, H, W) stack of the taps of a (3, m, n) `structure` -- plane 0 warped
    from `prev_step` through `backward_flow`, plane 1 gathered from `same_step`, plane 2 warped from `next_step`
    through `forward_flow`, each plane in np.where order (reference: convolve.py:147-245).  The three frames are
    separate arrays; nothing is copied into a volume.  The structure's centre [m // 2, n // 2] is subtracted from
    the (col, row) offsets as the reference does it, swap for m != n included.

    numpy arrays in, numpy array out; device tensors in, device tensor out; `res=` is written (cast to its dtype,
    which then takes the place of `dtype`) and returned.

    Deviations: float64 frames are sampled in float32; `dtype` is float32, float64 or int32; the frames in use and
    the flows must all have same_step's shape; `grid_locs` must hold integer values (ValueError otherwise)."""
    if len(structure.shape) != 3:
        raise ValueError("structure must have three dimensions")
    if structure.shape[0] != 3:
        raise ValueError("leading dimension of structure must have length 3")
    t = _lib.torch()
    struct = structure.detach().cpu().numpy() if isinstance(structure, t.Tensor) else np.asarray(structure)
    struct = np.ascontiguousarray(struct != 0, dtype=np.uint8)
    nb, ns, nf = (int(np.count_nonzero(struct[k])) for k in range(3))
    if (nb or nf) and method not in _METHODS:
        raise ValueError(f"method must be one of {list(_METHODS)}")
    on_device = isinstance(same_step, t.Tensor)
    if same_step.ndim != 2:
        raise ValueError("same_step must have shape (H, W)")
    H, W = int(same_step.shape[0]), int(same_step.shape[1])
    used = [(prev_step, backward_flow)] * bool(nb) + [(next_step, forward_flow)] * bool(nf)
    for frame, flow in used:
        if tuple(frame.shape) != (H, W) or tuple(flow.shape) != (H, W, 2):
            raise ValueError("prev_step, next_step and the flows must have same_step's shape (H, W) / (H, W, 2)")
    _check_grid(grid_locs, (H, W))
    frames = [prev_step] * bool(nb) + [same_step] * bool(ns) + [next_step] * bool(nf)
    code = _image_kind([_np_of(f) for f in frames], method if (nb or nf) else "nearest")
    _check_fill(code, fill_value)
    n_struct = nb + ns + nf
    _check_res(res, (n_struct, H, W))
    nd = np.dtype(dtype) if res is None else _np_of(res)
    if nd not in _OUT_CODES:
        if res is None:
            raise ValueError(f"dtype {nd} is not supported on the GPU path (float32, float64, int32)")
        nd = np.dtype(np.int32 if code == _lib.TF_I32 else np.float64)      # exact for the samples; cast into res afterwards
    if n_struct == 0:
        return _deliver(_lib.empty((0, H, W), _torch_dtype(nd)), res, on_device)
    p = _image_dev(prev_step, code) if nb else None
    s = _image_dev(same_step, code) if ns else None
    n = _image_dev(next_step, code) if nf else None
    bw = _lib.to_dev(backward_flow, t.float32) if nb else None
    fw = _lib.to_dev(forward_flow, t.float32) if nf else None
    g = _grid_dev(grid_locs)
    out, odt = _result((n_struct, H, W), nd, res)
    rc = _lib.lib().tf_convolve_step(_lib.ptr(p), _lib.ptr(s), _lib.ptr(n), code, H, W, _lib.ptr(fw), _lib.ptr(bw), _lib.ptr(g),
                                     struct.ctypes.data_as(_lib._P), struct.shape[1], struct.shape[2],
                                     _lib.INTERP[method] if (nb or nf) else 0, float(fill_value), _lib.ptr(out),
                                     _OUT_CODES[odt], _lib.stream_ptr())
    _lib.check(rc, "tf_convolve_step")
    return _deliver(out, res, on_device)


__all__ = ("convolve", "convolve_dev", "tag_func", "warp_flow", "convolve_same_step", "convolve_step")
