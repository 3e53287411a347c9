"""Point observations onto a grid on the GPU: the array-level binning under the reference's GLM, NEXRAD and flux gridding
(tobac_flow/glm.py:77-145, tobac_flow/nexrad.py:80-231, scripts/grid_flux.py:65-112), which call np.histogram2d,
scipy.stats.binned_statistic_dd and binned_statistic_2d once per frame, site and variable.

`bin_points` is the device operator (tf_bin_points: ONE pass over the points gives the counts, the masked counts and both
sums of every frame); `histogramdd`, `histogram2d`, `binned_statistic_dd`, `binned_statistic_2d` are thin forms under the
libraries' names and `weighted_binned_mean_2d` is grid_flux.py:65-73 in one launch.  tobac_flow_amd.glm and
tobac_flow_amd.nexrad build the reference's recipes on it.

Contract.  Counts equal NumPy's / SciPy's bit for bit, in every run.  Sums are double atomics: they differ from
the libraries' sequential bincount by the SUMMATION ORDER only -- for a bin with n terms both lie within
(n - 1) 2^-53 sum|term| of the exact sum; a one-term bin is bit-equal -- and may differ in the last bits from run to run.
Means are the quotient of two such sums taken in double.

Divergences.  `bins` must be explicit edge arrays (an integer bin count is NotImplementedError: the reference never passes
one).  Only the statistics "count", "sum" and "mean" exist, `values` is one-dimensional and `binnumber` is None.  Under the
SciPy rule a non-finite coordinate or value is a ValueError (SciPy 1.15 raises it with an integer bin count only; with
explicit edges it drops such a coordinate silently and lets a NaN value poison its bin).  NumPy arrays in give NumPy arrays
out; device tensors stay on the device."""
import collections
import ctypes

import numpy as np

from tobac_flow_amd.postprocess import _is_tensor, _lib, _np_dtype, _shape

OUTPUTS = ("count", "count_v", "sum_w", "sum_wv")
RULES = {"numpy": 0, "scipy": 1}
MAX_POINTS = 2 ** 31 - 1

BinnedStatisticddResult = collections.namedtuple("BinnedStatisticddResult", ("statistic", "bin_edges", "binnumber"))
BinnedStatistic2dResult = collections.namedtuple("BinnedStatistic2dResult", ("statistic", "x_edge", "y_edge", "binnumber"))


def power_of_ten(n):
    """10^n as np.around builds it: a table up to 10^8, then repeated multiplication by 10 (exact up to 10^22)"""
    n = int(n)
    ret = float(10 ** n) if n < 9 else 1e9
    for _ in range(n - 9):
        ret *= 10.0
    return ret


def scipy_decimals(min_width):
    """`decimal` of scipy.stats._binned_statistic._bin_numbers for the smallest edge difference of an axis (in the edges'
    dtype: the logarithm of a float32 width is taken in float32, as SciPy's is)"""
    if not min_width > 0:
        raise ValueError("The smallest edge difference is numerically 0.")
    return int(-np.log10(min_width)) + 6


def check_edges(bins, n_dims):
    """the edge arrays of `bins` (numpy float64, or device tensors as they are) and their smallest widths; an integer bin
    count is NotImplementedError, anything but 1-D non-decreasing arrays of at least 2 entries a ValueError"""
    if np.isscalar(bins) or bins is None:
        raise NotImplementedError("bins must be explicit edge arrays: the reference never passes a bin count")
    if (_is_tensor(bins) or isinstance(bins, np.ndarray)) and len(_shape(bins)) == 1 and n_dims != 1:
        bins = [bins] * n_dims                                    # np.histogram2d: one edge array for both axes
    if len(bins) != n_dims:
        raise ValueError("The dimension of bins must be equal to the dimension of the sample x.")
    edges, widths = [], []
    for d, e in enumerate(bins):
        if np.isscalar(e) or e is None:
            raise NotImplementedError("bins must be explicit edge arrays: the reference never passes a bin count")
        if not _is_tensor(e):
            e = np.asarray(e, dtype=np.float64)
        if len(_shape(e)) != 1 or _shape(e)[0] < 2:
            raise ValueError(f"bins[{d}] must be a one-dimensional array of at least 2 edges")
        diff = e[1:] - e[:-1]
        if not bool((diff >= 0).all()):                           # false for a NaN edge as well
            raise ValueError(f"`bins[{d}]` must be monotonically increasing, when an array")
        edges.append(e)
        widths.append(float(diff.min()))
    return edges, widths


def scipy_edges(edges, sample_dtype):
    """the edges as SciPy uses them: cast to a float32 sample's dtype ("preserve sample floating point precision in bin
    edges"); it takes the smallest width of THOSE and rounds point and last edge in float32.  Widened again for the
    device, float32 edges compare the same."""
    if np.dtype(sample_dtype) != np.dtype(np.float32):
        return list(edges)
    return [e.to(_lib().torch().float32) if _is_tensor(e) else e.astype(np.float32) for e in edges]


def _flat(x, name, n, kinds):
    shape, dtype = _shape(x), _np_dtype(x)
    if len(shape) != 1 or (n is not None and shape[0] != n):
        raise ValueError(f"{name} must be one-dimensional with one entry per point, got shape {shape}")
    if dtype not in kinds:
        raise TypeError(f"{name} must be {' or '.join(str(np.dtype(k)) for k in kinds)}, got {dtype}")
    return dtype


_REAL = (np.dtype(np.float32), np.dtype(np.float64))
_MASK = (np.dtype(np.bool_), np.dtype(np.uint8))


def _windows(win_start, win_end):
    ws = np.asarray(win_start.cpu() if _is_tensor(win_start) else win_start)
    we = np.asarray(win_end.cpu() if _is_tensor(win_end) else win_end)
    if ws.ndim != 1 or ws.shape != we.shape or ws.size < 1 or ws.dtype.kind not in "iu" or we.dtype.kind not in "iu":
        raise ValueError("win_start and win_end must be one-dimensional integer arrays of one length >= 1")
    ws, we = ws.astype(np.int64), we.astype(np.int64)
    if (np.diff(ws) < 0).any() or (np.diff(we) < 0).any():
        raise ValueError("win_start and win_end must both be non-decreasing")
    return ws, we


def bin_points(coords, edges, *, rule="numpy", values=None, weights=None, keep=None, keep_value=None, finite_value=False,
               time=None, win_start=None, win_end=None, flip=(), outputs=("count",), out=None, raise_on_status=True):
    """tf_bin_points: bin N points onto a (T, n_0[, n_1[, n_2]]) grid in one pass.  Returns a dict of DEVICE tensors, one per
    name in `outputs` -- "count" (int32: points passing `keep`), "count_v" (int32: those also passing `keep_value` and, with
    `finite_value`, holding a finite value), "sum_w", "sum_wv" (float64: sums of weight and of weight * value over the
    count_v points) -- and "status" (int, 0 under the NumPy rule).

    coords: 1 to 3 one-dimensional arrays, all float32 or all float64; coords[0] is the slowest output axis.  edges: one
    non-decreasing edge array per axis, arbitrary spacing.  The bin is searchsorted(edges, v, side="right") - 1.
    rule="numpy": v == edges[-1] belongs to the last bin, anything else beyond the edges, +-inf and NaN are dropped.
    rule="scipy": v >= edges[-1] belongs to the last bin iff np.around(v, d) == np.around(edges[-1], d) with SciPy's
    d = int(-log10(min width)) + 6, np.around evaluated in the coordinates' dtype as SciPy does; a zero width, a non-finite
    coordinate or a non-finite value is a ValueError.  `finite_value` drops non-finite values silently instead, under
    either rule.  values, weights: float32 or float64, a missing weight is 1; the product is taken in NumPy's result type.
    time (int64) with win_start, win_end (T integers each, both non-decreasing): a point goes to every frame f with
    win_start[f] <= t < win_end[f]; without them T = 1.  flip: axes written mirrored.  out: a dict of device tensors to
    accumulate into (+=) instead of fresh zeros, e.g. the result of an earlier call.  raise_on_status=False returns the
    status word (tf_bin_points' TF_BIN_STATUS_* bits) instead of raising SciPy's ValueError for it.

    Counts are identical in every run; the sums may differ in the last bits from run to run (atomic summation order)."""
    lib = _lib()
    params, result, status, hold = prepare(coords, edges, rule=rule, values=values, weights=weights, keep=keep,
                                           keep_value=keep_value, finite_value=finite_value, time=time, win_start=win_start,
                                           win_end=win_end, flip=flip, outputs=outputs, out=out)
    lib.check(lib.lib().tf_bin_points(ctypes.byref(params), lib.stream_ptr()), "tf_bin_points")
    result["status"] = int(status.item()) if status is not None else 0
    del hold
    if not raise_on_status:
        return result
    if result["status"] & lib.BIN_STATUS_COORD:
        raise ValueError("sample contains non-finite values.")
    if result["status"] & lib.BIN_STATUS_VALUE:
        raise ValueError("values contains non-finite values.")
    return result


def prepare(coords, edges, *, rule="numpy", values=None, weights=None, keep=None, keep_value=None, finite_value=False,
            time=None, win_start=None, win_end=None, flip=(), outputs=("count",), out=None):
    """What bin_points does before the launch: the validated operands on the device and the filled TfBinPoints --
    `(params, result, status, hold)`, `hold` keeping the operands alive.  tools/binning_time.py times the entry point alone
    with it."""
    coords = list(coords)
    if not 1 <= len(coords) <= 3:
        raise ValueError("1 to 3 coordinate arrays")
    if rule not in RULES:
        raise ValueError(f"rule must be 'numpy' or 'scipy', got {rule!r}")
    n = _shape(coords[0])[0] if len(_shape(coords[0])) == 1 else None
    ctype = _flat(coords[0], "coords[0]", n, _REAL)
    for d, c in enumerate(coords[1:], 1):
        if _flat(c, f"coords[{d}]", n, _REAL) != ctype:
            raise TypeError("the coordinate arrays must all be float32 or all be float64")
    if n > MAX_POINTS:
        raise ValueError(f"{n} points: at most 2^31 - 1 per call, split the points (the outputs accumulate)")
    edges, widths = check_edges(edges, len(coords))
    if rule == "scipy":
        edges = scipy_edges(edges, ctype)
        widths = [(e[1:] - e[:-1]).min() for e in edges]
        widths = [np.dtype(ctype).type(w.item()) if _is_tensor(w) else w for w in widths]
    decimals = [scipy_decimals(w) for w in widths] if rule == "scipy" else [0] * len(coords)
    vtype = _flat(values, "values", n, _REAL) if values is not None else None
    wtype = _flat(weights, "weights", n, _REAL) if weights is not None else None
    for name, mask in (("keep", keep), ("keep_value", keep_value)):
        if mask is not None:
            _flat(mask, name, n, _MASK)
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs):
        raise ValueError(f"outputs must name some of {OUTPUTS}")
    if "sum_wv" in outputs and values is None:
        raise ValueError("sum_wv needs values")
    windows = [x is not None for x in (time, win_start, win_end)]
    if any(windows) and not all(windows):
        raise ValueError("time, win_start and win_end go together")
    ws = we = None
    if all(windows):
        _flat(time, "time", n, (np.dtype(np.int64),))
        ws, we = _windows(win_start, win_end)
    flip = tuple(int(d) for d in flip)
    if any(d < 0 or d >= len(coords) for d in flip):
        raise ValueError("flip names an axis that is not there")
    shape = (1 if ws is None else int(ws.size),) + tuple(_shape(e)[0] - 1 for e in edges)

    lib = _lib()
    t = lib.torch()
    code = {np.dtype(np.float32): lib.TF_F32, np.dtype(np.float64): lib.TF_F64}
    hold = []                                                     # keeps every operand alive until the launch is enqueued

    def dev(x, dtype=None):
        if not _is_tensor(x) and np.asarray(x).size == 0:         # nothing to stage
            x = t.zeros(0, dtype=getattr(t, str(np.asarray(x).dtype)), device=lib.device())
        y = lib.to_dev(x, dtype)
        if y.dtype == t.bool:
            y = y.view(t.uint8)
        hold.append(y)
        return y.data_ptr() or None

    P = lib.BinPoints()
    P.n_dims, P.coord_dtype, P.rule = len(coords), code[ctype], RULES[rule]
    P.value_dtype = code[vtype] if vtype is not None else 0
    P.weight_dtype = code[wtype] if wtype is not None else 0
    P.flags = lib.BIN_FINITE_VALUE if finite_value else 0
    P.flip_mask = sum(1 << d for d in set(flip))
    P.n_points, P.n_frames = n, shape[0]
    for d in range(len(coords)):
        P.decimals[d], P.round_scale[d] = decimals[d], power_of_ten(abs(decimals[d]))
        P.n_edges[d] = _shape(edges[d])[0]
        P.coord[d] = dev(coords[d])
        P.edges[d] = dev(edges[d], t.float64)
    P.keep, P.keep_value = (dev(m) if m is not None else None for m in (keep, keep_value))
    P.value, P.weight = (dev(x) if x is not None else None for x in (values, weights))
    if ws is not None:
        P.time, P.win_start, P.win_end = dev(time), dev(ws), dev(we)
    result = {}
    for name in outputs:
        dtype = t.int32 if name.startswith("count") else t.float64
        if out is not None and name in out:
            buf = out[name]
            if not _is_tensor(buf) or tuple(buf.shape) != shape or buf.dtype != dtype or not buf.is_contiguous() or not buf.is_cuda:
                raise ValueError(f"out[{name!r}] must be a contiguous device tensor of shape {shape} and dtype {dtype}")
        else:
            buf = t.zeros(shape, dtype=dtype, device=lib.device())
        result[name] = buf
        setattr(P, name, buf.data_ptr())
    status = t.zeros(1, dtype=t.int32, device=lib.device()) if rule == "scipy" else None
    P.status = status.data_ptr() if status is not None else None
    return P, result, status, hold


# ---- the libraries' names --------------------------------------------------------------------------------------------------
def _columns(sample):
    """np.histogramdd's `sample`: an (N, D) array, or a sequence of D coordinate arrays"""
    if (_is_tensor(sample) or isinstance(sample, np.ndarray)) and len(_shape(sample)) == 2:
        return [sample[:, d].contiguous() if _is_tensor(sample) else np.ascontiguousarray(sample[:, d]) for d in range(_shape(sample)[1])]
    if (_is_tensor(sample) or isinstance(sample, np.ndarray)) and len(_shape(sample)) == 1:
        return [sample]
    return [c if _is_tensor(c) else np.asarray(c) for c in sample]


def _on_device(*operands):
    return any(_is_tensor(x) for x in operands if x is not None)


def _give(x, device):
    return x if device else _lib().to_host(x)


def histogramdd(sample, bins, weights=None):
    """np.histogramdd(sample, bins=bins, weights=weights) for explicit edge arrays: `(hist, edges)`, hist float64 -- the
    counts, or the sums of the weights (summation order: module docstring).  No `range`, no `density`."""
    cols = _columns(sample)
    device = _on_device(*cols, weights)
    edges, _ = check_edges(bins, len(cols))
    if weights is None:
        hist = bin_points(cols, edges, outputs=("count",))["count"].to(_lib().torch().float64)
    else:
        hist = bin_points(cols, edges, weights=weights, outputs=("sum_w",))["sum_w"]
    return _give(hist[0], device), list(edges)


def histogram2d(x, y, bins, weights=None):
    """np.histogram2d(x, y, bins=bins, weights=weights) for explicit edges (one array for both axes, or a pair):
    `(hist, xedges, yedges)`"""
    hist, edges = histogramdd([x, y], bins, weights)
    return hist, edges[0], edges[1]


def binned_statistic_dd(sample, values, statistic="mean", bins=None):
    """scipy.stats.binned_statistic_dd(sample, values, statistic, bins) for explicit edge arrays and statistic "count",
    "sum" or "mean" (NaN over an empty bin); anything else is NotImplementedError.  The result carries `.statistic`
    (float64) and `.bin_edges`; `.binnumber` is None: the bin of every point is never materialised.  `values` is
    one-dimensional (ignored for "count").  Sums: module docstring."""
    if statistic not in ("count", "sum", "mean"):
        raise NotImplementedError(f"statistic {statistic!r}: only 'count', 'sum' and 'mean' run on the device")
    cols = _columns(sample)
    edges, _ = check_edges(bins, len(cols))
    if statistic == "count":
        device = _on_device(*cols)
        stat = bin_points(cols, edges, rule="scipy", outputs=("count",))["count"].to(_lib().torch().float64)
    else:
        device = _on_device(*cols, values)
        if not _is_tensor(values):
            values = np.asarray(values)
            if values.dtype.kind in "iub":
                values = values.astype(np.float64)
        if len(_shape(values)) != 1:
            raise NotImplementedError("values must be one-dimensional")
        got = bin_points(cols, edges, rule="scipy", values=values, outputs=("count_v", "sum_wv"))
        stat = got["sum_wv"]
        if statistic == "mean":
            t = _lib().torch()
            count = got["count_v"].to(t.float64)
            stat = t.where(count > 0, stat / count, t.full_like(stat, float("nan")))
    return BinnedStatisticddResult(_give(stat[0], device), scipy_edges(edges, _np_dtype(cols[0])), None)


def binned_statistic_2d(x, y, values, statistic="mean", bins=None):
    """scipy.stats.binned_statistic_2d(x, y, values, statistic, bins): as binned_statistic_dd, the result carries
    `.statistic`, `.x_edge`, `.y_edge`; `.binnumber` is None"""
    edges, _ = check_edges(bins, 2)
    res = binned_statistic_dd([x, y], values, statistic, edges)
    return BinnedStatistic2dResult(res.statistic, res.bin_edges[0], res.bin_edges[1], None)


def weighted_binned_mean_2d(x, y, data, weights, bins=None):
    """scripts/grid_flux.py:65-73: the mean of `data` weighted by `weights` over the bins of (x, y), points with a non-finite
    `data` left out -- sum(data * weights) / sum(weights) per bin, NaN where the bin is empty.  One launch gives both sums
    (the reference: two binned_statistic_2d calls over the masked copies); x, y, data and weights may have any one shape.
    The product is taken in the operands' NumPy result type, as `data[wh] * weights[wh]` is."""
    edges, _ = check_edges(bins, 2)
    device = _on_device(x, y, data, weights)
    flat = [a.reshape(-1) if _is_tensor(a) else np.asarray(a).reshape(-1) for a in (x, y, data, weights)]
    got = bin_points(flat[:2], edges, rule="scipy", values=flat[2], weights=flat[3], finite_value=True,
                     outputs=("sum_w", "sum_wv"))
    return _give((got["sum_wv"] / got["sum_w"])[0], device)


# ---- times ---------------------------------------------------------------------------------------------------------------
def time_ticks(x):
    """Times as int64 microseconds since 1970-01-01 (the resolution of the reference's datetimes): datetime64 of any unit,
    Python datetimes, or integers that already are such ticks (NumPy arrays or device tensors)."""
    if _is_tensor(x):
        if _np_dtype(x) != np.dtype(np.int64):
            raise TypeError("times on the device must be int64 microseconds")
        return x
    a = np.asarray(x)
    if a.dtype.kind == "O":
        a = np.asarray(a, dtype="datetime64[us]")
    if a.dtype.kind == "M":
        return a.astype("datetime64[us]").astype(np.int64)
    if a.dtype.kind in "iu":
        return a.astype(np.int64)
    raise TypeError(f"times must be datetimes or integer microseconds, got {a.dtype}")
