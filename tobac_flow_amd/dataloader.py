"""bt, wvd and swd (or twd) from raw channel stacks on the GPU: the array-level work under the reference's loaders --
load_mcmip (tobac_flow/dataloader.py:240-321), seviri_dataloader (:588-688), seviri_nat_dataloader (:833-958),
get_stripe_deviation (:234-237) and fill_time_gap_nan (:341-357).  The file decoders (netCDF4, satpy), the geodesy
(`return_new_ds`) and fill_time_gap_full_disk, which fetches further files, stay with the caller.

What a decoder hands out goes in as it is: float32 stacks, where NaN and +-inf mean missing, or the 16-bit packed integers
of the files with their scale, offset and fill (`PackedChannel`: half the bytes across PCIe); NumPy arrays are uploaded,
device tensors are used in place, strides included -- a `[..., y0:y1, x0:x1]` view of full frames needs no copy.
`prepare_fields` is the device operator (tf_prepare_fields after one tf_stripe_deviation per DQF plane); `goes_fields`,
`seviri_fields` and `seviri_nat_fields` are the three recipes of the reference.  The results are
detection.DeviceField's with the new time coordinate, which create_flow and the detection recipes take as they are.

Contract.  The fields equal the NumPy form of the reference's lines bit for bit: CF decoding with two float32
roundings, one rounding per difference, a joint mask.  The stripe deviation has np.nanmean's and np.nanstd's column values
bit for bit (exact integer counts and sums, NumPy's own second pass down the column) and one float64 row sum in a fixed
order: it is identical from run to run and differs from NumPy's by the order of that sum only."""
import ctypes
import warnings
from datetime import timedelta

import numpy as np

from tobac_flow_amd import _lib
from tobac_flow_amd.utils.datetime_utils import get_datetime_from_coord


class PackedChannel:
    """A channel as the file stores it: int16 `raw` (T, H, W) with CF `scale_factor`, `add_offset`, an optional `_FillValue`
    and netCDF's `_Unsigned` (GOES CMI): with `unsigned` the bits are read as uint16.  A uint16 NumPy array is taken as
    those bits with unsigned=True.  The fill value is normalised to the stored type (a `_FillValue` of -1 on an unsigned
    variable is 65535)."""

    def __init__(self, raw, scale_factor, add_offset, fill_value=None, unsigned=False):
        if isinstance(raw, np.ndarray) and raw.dtype == np.uint16:
            raw, unsigned = raw.view(np.int16), True
        if _np_dtype(raw) != np.dtype(np.int16):
            raise TypeError(f"a packed channel is int16 (or uint16 bits), got {_np_dtype(raw)}")
        self.raw, self.unsigned = raw, bool(unsigned)
        self.scale_factor, self.add_offset = np.float32(scale_factor), np.float32(add_offset)
        if fill_value is None:
            self.fill_value = None
        else:
            bits = int(fill_value) & 0xffff
            self.fill_value = bits if self.unsigned else bits - 0x10000 if bits >= 0x8000 else bits

    shape = property(lambda self: tuple(self.raw.shape))


def _is_tensor(x):
    return _lib.is_tensor(x)


def _np_dtype(x):
    if _is_tensor(x):
        return np.dtype(str(x.dtype).replace("torch.", ""))
    return np.asarray(x).dtype


def _plane(x, shape, kinds, what, hold):
    """one (T, H, W) operand as a filled FieldPlane: a host array uploaded, a device tensor in place with its strides"""
    if not _is_tensor(x):
        x = np.asarray(x)
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(x.shape)}, expected (T, H, W) = {tuple(shape)}")
    dtype = _np_dtype(x)
    if dtype not in kinds:
        raise TypeError(f"{what} must be {' or '.join(str(np.dtype(k)) for k in kinds)}, got {dtype}")
    if _is_tensor(x):
        if not x.is_cuda:
            x = _lib.to_dev(x)
        elif x.stride(2) != 1 and shape[2] > 1 or any(s < 0 for s in x.stride()):
            x = x.contiguous()                                    # x must be contiguous; any frame and row stride will do
    else:
        x = _lib.to_dev(x)
    hold.append(x)
    P = _lib.FieldPlane()
    P.data = x.data_ptr()
    P.row_stride = x.stride(1) if shape[1] > 1 else shape[2]
    P.frame_stride = x.stride(0) if shape[0] > 1 else P.row_stride * shape[1]
    if P.row_stride < shape[2] or P.frame_stride < P.row_stride:
        raise ValueError(f"{what}: rows must not overlap and frames must lie behind one another")
    P.dtype = {np.dtype(np.float32): _lib.TF_F32, np.dtype(np.int16): _lib.TF_I16, np.dtype(np.int8): _lib.TF_I8,
               np.dtype(np.uint8): _lib.TF_U8}[dtype]
    return P


def _dqf_plane(item, shape, what, hold):
    """a DQF plane: an int8 / uint8 array, or (array, fill_value)"""
    arr, fill = item if isinstance(item, tuple) else (item, None)
    P = _plane(arr, shape, (np.dtype(np.int8), np.dtype(np.uint8)), what, hold)
    if fill is not None:
        bits = int(fill) & 0xff
        P.has_fill, P.fill = 1, bits - 0x100 if P.dtype == _lib.TF_I8 and bits >= 0x80 else bits
    return P


def _channel_plane(ch, shape, what, hold):
    if isinstance(ch, PackedChannel):
        P = _plane(ch.raw, shape, (np.dtype(np.int16),), what, hold)
        P.scale, P.offset, P.is_unsigned = float(ch.scale_factor), float(ch.add_offset), int(ch.unsigned)
        if ch.fill_value is not None:
            P.has_fill, P.fill = 1, ch.fill_value
        return P
    return _plane(ch, shape, (np.dtype(np.float32),), what + " (float32, or a PackedChannel)", hold)


def _shape3(x, what):
    shape = tuple(x.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what} must be a non-empty (T, H, W) stack, got shape {shape}")
    return shape


def _times(t, n):
    t = np.asarray(getattr(t, "values", t))
    if t.dtype.kind != "M" or t.ndim != 1:
        raise TypeError("t must be a one-dimensional datetime64 array")
    if n is not None and t.size != n:
        raise ValueError(f"t has {t.size} entries for {n} frames")
    return t


def frame_table(t, time_gap=None, keep=None):
    """Which input frame every output frame is made from: `(src, t_out)`, src int32 with -1 for an all-NaN frame.  Pure
    host code.  In this order: `keep` (bool per frame) drops frames with the warning of goes_dataloader:78-94; more than
    one frame left is sorted by time, stably (load_mcmip:316-317); duplicate times raise the RuntimeError of :131-132;
    with `time_gap` a NaN frame goes in wherever two frames are further apart than that (fill_time_gap_nan:341-357), at
    t[i] + (t[i + 1] - t[i]) / 2 in datetime64 arithmetic (create_nan_slice:325)."""
    t = _times(t, None)
    idx = np.arange(t.size)
    if keep is not None:
        keep = np.asarray(keep)
        if keep.dtype != np.bool_ or keep.shape != t.shape:
            raise ValueError("keep must be one bool per frame")
        if not np.all(keep):
            warnings.warn("Invalid time stamps found in ABI data, removing", RuntimeWarning)
            idx = idx[keep]
    if idx.size == 0:
        raise ValueError("no frame is left")
    if idx.size > 1:
        idx = idx[np.argsort(t[idx], kind="stable")]
    ts = t[idx]
    if np.unique(ts).size < ts.size:
        raise RuntimeError("Duplicate time steps in input index values")
    src, t_out = [int(idx[0])], [ts[0]]
    if time_gap is not None and ts.size > 1:
        gap = np.diff(np.asarray(get_datetime_from_coord(ts), dtype=object)) > time_gap
    else:
        gap = np.zeros(ts.size - 1, bool)
    for i in range(ts.size - 1):
        if gap[i]:
            src.append(-1)
            t_out.append(ts[i] + (ts[i + 1] - ts[i]) / 2)
        src.append(int(idx[i + 1]))
        t_out.append(ts[i + 1])
    return np.asarray(src, np.int32), np.asarray(t_out, dtype=t.dtype)


def get_stripe_deviation(dqf, fill_value=None):
    """get_stripe_deviation (tobac_flow/dataloader.py:234-237) of a (T, H, W) int8 / uint8 DQF stack under xarray's skipna
    rule, `fill_value` being NaN: (T, H) float64, NaN for a row without a valid term -- a NumPy array for a NumPy stack, a
    device tensor for a device tensor."""
    shape = _shape3(dqf, "dqf")
    hold = []
    P = _dqf_plane((dqf, fill_value), shape, "dqf", hold)
    t = _lib.torch()
    dev = t.empty(shape[:2], dtype=t.float64, device=_lib.device())
    _stripes(P, shape, 0.0, dev, None)
    return dev if _is_tensor(dqf) else _lib.to_host(dev)


def _stripes(P, shape, threshold, dev, row_flags):
    L = _lib.lib()
    nbytes = L.tf_stripe_workspace_bytes(*shape)
    ws = _lib.workspace(nbytes, "fields")
    _lib.check(L.tf_stripe_deviation(ctypes.byref(P), *shape, float(threshold), _lib.ptr(dev), _lib.ptr(row_flags), _lib.ptr(ws),
                                     nbytes, _lib.stream_ptr()), "tf_stripe_deviation")


def _recipe(r, n_channels):
    r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
    if not 1 <= len(r) <= 3:
        raise ValueError("a recipe is (a,), (a, b) or (a, b, floor)")
    a, b, floor = (r + (None, None))[:3]
    if not 0 <= int(a) < n_channels or (b is not None and not 0 <= int(b) < n_channels):
        raise ValueError("a recipe names a channel that is not there")
    return int(a), -1 if b is None else int(b), floor


def prepare_fields(channels, recipes, t, dqf=(), time_gap=None, keep=None, stripe_threshold=2, return_masked=False):
    """tf_prepare_fields: the fields of `recipes` from the raw `channels`, one DeviceField per recipe.

    channels: up to 8 (T, H, W) stacks, all float32 arrays or all PackedChannel's, host or device.  recipes: up to 4 of
    (a,), (a, b) or (a, b, floor) -- channel a, the difference a - b, and np.maximum(., floor) of it.  dqf: up to 8 int8 /
    uint8 stacks, or (stack, fill_value) pairs.  A voxel where any field is non-finite, any DQF plane is non-zero or fill,
    or whose row is a stripe row of any DQF plane (get_stripe_deviation > stripe_threshold; None: no stripe test) is NaN
    in every field.  t, time_gap, keep: frame_table.  return_masked=True appends the int32 device tensor of the number of
    NaN voxels per output frame (a frame with nothing left has H W of them)."""
    channels, recipes, dqf = list(channels), list(recipes), list(dqf)
    if not 1 <= len(channels) <= _lib.FIELD_MAX_CHANNELS:
        raise ValueError(f"1 to {_lib.FIELD_MAX_CHANNELS} channels, got {len(channels)}")
    if not 1 <= len(recipes) <= _lib.FIELD_MAX_RECIPES:
        raise ValueError(f"1 to {_lib.FIELD_MAX_RECIPES} recipes, got {len(recipes)}")
    if len(dqf) > _lib.FIELD_MAX_DQF:
        raise ValueError(f"at most {_lib.FIELD_MAX_DQF} DQF planes, got {len(dqf)}")
    packed = [isinstance(c, PackedChannel) for c in channels]
    if any(packed) and not all(packed):
        raise TypeError("the channels must all be float32 or all be packed")
    shape = _shape3(channels[0], "channels[0]")
    recipes = [_recipe(r, len(channels)) for r in recipes]
    src, t_out = frame_table(_times(t, shape[0]), time_gap, keep)

    tt = _lib.torch()
    hold = []
    P = _lib.FieldPrep()
    (P.T, P.H, P.W), P.T_out = shape, len(src)
    P.n_channels, P.n_dqf, P.n_recipes = len(channels), len(dqf), len(recipes)
    for i, c in enumerate(channels):
        P.channel[i] = _channel_plane(c, shape, f"channels[{i}]", hold)
    for i, d in enumerate(dqf):
        P.dqf[i] = _dqf_plane(d, shape, f"dqf[{i}]", hold)
    dev = _lib.device()
    if dqf and stripe_threshold is not None:
        row_flags = tt.zeros(shape[:2], dtype=tt.uint8, device=dev)
        for i in range(len(dqf)):                                 # one after another on one stream: the flags OR without atomics
            _stripes(P.dqf[i], shape, stripe_threshold, None, row_flags)
        P.row_flags = row_flags.data_ptr()
        hold.append(row_flags)
    outs = [tt.empty((len(src),) + shape[1:], dtype=tt.float32, device=dev) for _ in recipes]
    for i, ((a, b, floor), out) in enumerate(zip(recipes, outs)):
        P.recipe[i].a, P.recipe[i].b, P.recipe[i].out = a, b, out.data_ptr()
        if floor is not None:
            P.recipe[i].has_floor, P.recipe[i].floor = 1, float(floor)
    src_dev = _lib.to_dev(src)
    n_masked = tt.empty(len(src), dtype=tt.int32, device=dev)
    P.src, P.n_masked = src_dev.data_ptr(), n_masked.data_ptr()
    _lib.check(_lib.lib().tf_prepare_fields(ctypes.byref(P), _lib.stream_ptr()), "tf_prepare_fields")
    del hold
    from tobac_flow_amd.detection import DeviceField
    fields = [DeviceField(out, t_out) for out in outs]
    return fields + [n_masked] if return_masked else fields


def fill_time_gap_nan(field, t, time_gap):
    """fill_time_gap_nan (tobac_flow/dataloader.py:341-357) of one finished float32 (T, H, W) field -- a DeviceField, a
    device tensor or a NumPy array: an all-NaN frame wherever two frames are further apart than `time_gap`, every value,
    infinities included, kept.  `t` is the field's time coordinate (None: a DeviceField's own; it must be sorted, as the
    reference's is by then).  Returns `(field, t_out)` in the container of the input; a DeviceField carries t_out."""
    from tobac_flow_amd.detection import DeviceField
    data = field.data if isinstance(field, DeviceField) else field
    if t is None and isinstance(field, DeviceField):
        t = field.t.values
    shape = _shape3(data, "field")
    t = _times(t, shape[0])
    if t.size > 1 and np.any(np.diff(t) < np.timedelta64(0)):
        raise ValueError("t must be sorted")
    src, t_out = frame_table(t, time_gap)
    tt = _lib.torch()
    hold = []
    P = _lib.FieldPrep()
    (P.T, P.H, P.W), P.T_out = shape, len(src)
    P.n_channels, P.n_recipes, P.flags = 1, 1, _lib.FIELD_COPY
    P.channel[0] = _plane(data, shape, (np.dtype(np.float32),), "field", hold)
    out = tt.empty((len(src),) + shape[1:], dtype=tt.float32, device=_lib.device())
    P.recipe[0].a, P.recipe[0].b, P.recipe[0].out = 0, -1, out.data_ptr()
    src_dev = _lib.to_dev(src)
    P.src = src_dev.data_ptr()
    _lib.check(_lib.lib().tf_prepare_fields(ctypes.byref(P), _lib.stream_ptr()), "tf_prepare_fields")
    del hold
    if isinstance(field, DeviceField):
        return DeviceField(out, t_out), t_out
    return (out if _is_tensor(field) else _lib.to_host(out)), t_out


# ---- the reference's three loaders at array level ------------------------------------------------------------------------
def _deliver(fields, on_device, *inputs):
    """DeviceField's for device input and, with on_device, for host input; NumPy arrays otherwise (their time coordinate is
    frame_table(t, time_gap, keep)[1])"""
    device_in = any(_is_tensor(c.raw if isinstance(c, PackedChannel) else c) for c in inputs)
    if device_in or on_device:
        return tuple(fields)
    return tuple(_lib.to_host(f.data) for f in fields)


def goes_fields(c08, c10, c13, c15, t, dqf=(), time_gap=timedelta(minutes=15), keep=None, on_device=True):
    """load_mcmip and the time handling of goes_dataloader at array level: `(bt, wvd, swd)` = C13, C08 - C10, C13 - C15
    from the CMI stacks (float32, or PackedChannel's as the MCMIP files store them), masked jointly where a field is
    non-finite, a plane of `dqf` (the DQF_C08 / C10 / C13 / C15 stacks) is set or fill, or a row is a stripe row
    (get_stripe_deviation > 2); `keep` is the padded-range check of goes_dataloader:78-94, the frames are sorted by time
    and NaN frames fill gaps above `time_gap`."""
    fields = prepare_fields([c08, c10, c13, c15], [(2,), (0, 1), (2, 3)], t, dqf=dqf, time_gap=time_gap, keep=keep)
    return _deliver(fields, on_device, c08, c10, c13, c15)


def seviri_fields(ch5, ch6, ch9, ch10, t, time_gap=timedelta(minutes=30), on_device=True):
    """seviri_dataloader at array level: `(bt, wvd, swd)` = ch9, ch5 - ch6, ch9 - ch10 of the brightness temperatures,
    masked jointly where one is non-finite; NaN frames fill gaps above `time_gap`"""
    fields = prepare_fields([ch5, ch6, ch9, ch10], [(2,), (0, 1), (2, 3)], t, time_gap=time_gap)
    return _deliver(fields, on_device, ch5, ch6, ch9, ch10)


def seviri_nat_fields(wv_062, wv_073, ir_087, ir_108, ir_120, t, time_gap=timedelta(minutes=30), on_device=True):
    """seviri_nat_dataloader at array level: `(bt, wvd, twd)` = IR_108, WV_062 - WV_073, max(IR_087 - IR_120, 0), masked
    jointly where one is non-finite; NaN frames fill gaps above `time_gap`"""
    fields = prepare_fields([wv_062, wv_073, ir_087, ir_108, ir_120], [(3,), (0, 1), (2, 4, 0.0)], t, time_gap=time_gap)
    return _deliver(fields, on_device, wv_062, wv_073, ir_087, ir_108, ir_120)


__all__ = ("PackedChannel", "get_stripe_deviation", "frame_table", "fill_time_gap_nan", "prepare_fields", "goes_fields",
           "seviri_fields", "seviri_nat_fields")
