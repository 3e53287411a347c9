"""Grouped reductions over step records: the one grouping pass behind the third stage (utils/stats_utils.py *_groupby,
utils/filter_utils.py, postprocess.process_*_properties).

`reduce_groups(groups, coord, ops)` evaluates a list of column operations per group id of `coord`.  An operation is a tuple
`(name, f, w, aux)` with `name` one of `_lib.GROUP_OPS` and the columns it takes (None for the others):

    COUNT                                      -> int64
    SUM MEAN MIN MAX of f (NaN skipped)        -> float64 (MIN / MAX of an int64 column: int64)
    PICK_ARGMIN / ARGMAX / IDXMIN / IDXMAX     -> int64 position in the record table (IDX*: NaN skipped, -1 if all NaN)
    WEIGHTED_AVERAGE COMBINED_MEAN AVERAGE_UNCERTAINTY of (f, w);  COMBINED_STD of (f = stds, w = areas, aux = means)
    FIRST_MINUS_LAST LAST_MINUS_FIRST MAX_DIFF -> float64, int64 for an int64 column;  ANY_NAN -> int64 0 / 1
    GRADIENT_MIN / GRADIENT_PICK_IDXMIN of (f, aux = times)

Members of a group are taken in record order, groups in the order of `coord`.  Device tensors are reduced by
tf_group_reduce (csrc/group_reduce.hip) in as few calls as its 16-entry table allows and come back as device tensors; the
host sees the two status words only.  NumPy columns take the NumPy code below.  Either way a record whose id is not in
`coord`, and a `coord` id without a record, raise ValueError (the reference would silently misalign its columns)."""
import ctypes

import numpy as np

from tobac_flow_amd import _lib

_INT_OUT = {"COUNT", "PICK_ARGMIN", "PICK_ARGMAX", "PICK_IDXMIN", "PICK_IDXMAX", "ANY_NAN", "GRADIENT_PICK_IDXMIN"}
_INT_IN = {"MIN", "MAX", "PICK_ARGMIN", "PICK_ARGMAX", "PICK_IDXMIN", "PICK_IDXMAX", "FIRST_MINUS_LAST", "LAST_MINUS_FIRST", "MAX_DIFF"}
_WEIGHTED = {"WEIGHTED_AVERAGE", "COMBINED_MEAN", "COMBINED_STD", "AVERAGE_UNCERTAINTY"}
_THIRD = {"COMBINED_STD", "GRADIENT_MIN", "GRADIENT_PICK_IDXMIN"}


def _kind(x):
    """'f4' / 'f8' / 'i8' / 'i4' ... of a numpy array or a tensor"""
    if _lib.is_tensor(x):
        t = _lib.torch()
        return {t.float32: "f4", t.float64: "f8", t.int64: "i8", t.int32: "i4", t.int16: "i2", t.uint8: "u1", t.bool: "b1"}.get(x.dtype, "?")
    return x.dtype.kind + str(x.dtype.itemsize)


def as_ticks(x):
    """datetime64 / timedelta64 columns as their int64 ticks (a view); anything else unchanged"""
    if not _lib.is_tensor(x):
        x = np.asarray(x)
        if x.dtype.kind in "mM":
            return x.view(np.int64)
    return x


def _column(x, n, what, ints_ok):
    """a column as the kernels take it: 1-D, n long, float32 / float64 (or int64 where the operation takes integers)"""
    x = as_ticks(x)
    if tuple(x.shape) != (n,):
        raise ValueError(f"{what}: a column of shape {tuple(x.shape)} beside {n} records")
    kind = _kind(x)
    if kind in ("f4", "f8") or (ints_ok and kind == "i8"):
        return x
    if kind[0] in "iub" and ints_ok:
        return x.to(_lib.torch().int64) if _lib.is_tensor(x) else x.astype(np.int64)
    if kind[0] in "iub" or kind == "f2":
        return x.to(_lib.torch().float64) if _lib.is_tensor(x) else x.astype(np.float64)
    raise TypeError(f"{what}: columns are float32, float64 or integer, not {x.dtype}")


def check_inputs(groups, coord, ops):
    """-> (coord as a sorted host array of the ids' type, ops with their columns normalised); raises before any launch"""
    coord = np.asarray(_lib.to_host(coord) if _lib.is_tensor(coord) else coord)
    if coord.ndim != 1 or coord.dtype.kind not in "iu":
        raise ValueError("coord must be a 1-D integer array")
    if len(groups.shape) != 1 or _kind(groups)[0] not in "iu":
        raise ValueError("groups must be a 1-D integer column")
    if coord.size > 1 and not np.all(coord[1:] > coord[:-1]):
        raise ValueError("coord must be sorted and without repeats")
    n = int(groups.shape[0])
    done = []
    for op in ops:
        name, f, w, aux = (tuple(op) + (None, None, None))[:4]
        if name not in _lib.GROUP_OPS:
            raise ValueError(f"unknown group operation {name!r}")
        need = (name != "COUNT", name in _WEIGHTED, name in _THIRD)
        if any((col is None) == wanted for col, wanted in zip((f, w, aux), need)):
            raise ValueError(f"{name}: takes {sum(need)} column(s)")
        f = None if f is None else _column(f, n, name, name in _INT_IN)
        w = None if w is None else _column(w, n, name + " weights", False)
        aux = None if aux is None else _column(aux, n, name, name != "COMBINED_STD")
        done.append((name, f, w, aux))
    return coord, done


# ---- NumPy path -------------------------------------------------------------------------------------------------------
def _np_extreme(x, largest, skip):
    if x.dtype.kind == "f":
        nan = np.isnan(x)
        if skip:
            kept = np.flatnonzero(~nan)
            if kept.size == 0:
                return -1
            return int(kept[np.argmax(x[kept]) if largest else np.argmin(x[kept])])
        if nan.any():
            return int(np.argmax(nan))
    return int(np.argmax(x) if largest else np.argmin(x))


def _np_gradient(f, t):
    if f.size < 2:
        return np.full(f.size, np.nan)
    with np.errstate(all="ignore"):
        return np.gradient(f, t, edge_order=1)


def _np_one(name, f, w, aux, order, start):
    """one operation over the sorted runs; f, w, aux already gathered into run order (float columns as float64)"""
    first, n_groups = start[:-1], start.size - 1
    counts = np.diff(start)
    runs = [slice(int(b), int(e)) for b, e in zip(first, start[1:])]
    with np.errstate(all="ignore"):
        if name == "COUNT":
            return counts.astype(np.int64)
        if name in ("SUM", "MEAN"):
            ok = ~np.isnan(f)
            total = np.add.reduceat(np.where(ok, f, 0.0), first)
            return total if name == "SUM" else total / np.add.reduceat(ok.astype(np.float64), first)
        if name in ("MIN", "MAX"):
            if f.dtype.kind == "i":
                return (np.minimum if name == "MIN" else np.maximum).reduceat(f, first)
            return (np.fmin if name == "MIN" else np.fmax).reduceat(f, first)
        if name.startswith("PICK_"):
            at = np.array([_np_extreme(f[r], name.endswith("MAX"), "IDX" in name) for r in runs], np.int64).reshape(n_groups)
            return np.where(at >= 0, order[np.maximum(at, 0) + first], -1).astype(np.int64)
        if name == "WEIGHTED_AVERAGE":
            total = np.add.reduceat(w, first)
            return np.where(total == 0, np.nan, np.add.reduceat(f * w, first) / total)
        if name in ("COMBINED_MEAN", "COMBINED_STD"):
            mean = f if name == "COMBINED_MEAN" else aux
            ok = np.isfinite(mean) & np.isfinite(w)
            area = np.add.reduceat(np.where(ok, w, 0.0), first)
            combined = np.where(np.add.reduceat(ok.astype(np.int64), first) > 0,
                                np.add.reduceat(np.where(ok, mean * w, 0.0), first) / area, np.nan)
            if name == "COMBINED_MEAN":
                return combined
            ok &= np.isfinite(f)
            area = np.add.reduceat(np.where(ok, w, 0.0), first)
            spread = np.add.reduceat(np.where(ok, w * f, 0.0), first) + \
                np.add.reduceat(np.where(ok, w * (mean - np.repeat(combined, counts)) ** 2, 0.0), first)
            return np.where(np.add.reduceat(ok.astype(np.int64), first) > 0, np.sqrt(spread / area), np.nan)
        if name == "AVERAGE_UNCERTAINTY":
            total = np.add.reduceat(w, first)
            return np.where(total > 0, np.sqrt(np.add.reduceat(w ** 2 * f ** 2, first)) / total, np.nan)
        if name == "FIRST_MINUS_LAST":
            return f[first] - f[start[1:] - 1]
        if name == "LAST_MINUS_FIRST":
            return f[start[1:] - 1] - f[first]
        if name == "MAX_DIFF":
            return np.array([np.max(np.diff(f[r])) if r.stop - r.start > 1 else 0 for r in runs], f.dtype).reshape(n_groups)
        if name == "ANY_NAN":
            return (np.add.reduceat(np.isnan(f).astype(np.int64), first) > 0).astype(np.int64)
        grads = [_np_gradient(f[r], aux[r].astype(np.float64)) for r in runs]
        if name == "GRADIENT_MIN":
            return np.array([np.nanmin(g) if np.any(~np.isnan(g)) else np.nan for g in grads], np.float64).reshape(n_groups)
        at = np.array([_np_extreme(g, False, True) for g in grads], np.int64).reshape(n_groups)
        return np.where(at >= 0, order[np.maximum(at, 0) + first], -1).astype(np.int64)


def _np_reduce(groups, coord, ops):
    groups = np.asarray(groups)
    n_groups = coord.size
    rank = np.searchsorted(coord, groups)
    orphan = rank == n_groups
    orphan[~orphan] = coord[rank[~orphan]] != groups[~orphan]
    counts = np.bincount(rank[~orphan], minlength=n_groups)
    _raise_on_status(int(orphan.sum()), int((counts == 0).sum()))
    if n_groups == 0:
        return [np.zeros(0, np.int64 if _out_is_int(name, f) else np.float64) for name, f, _, _ in ops]
    order = np.argsort(rank, kind="stable")
    start = np.concatenate([[0], np.cumsum(counts)])

    def gathered(x, keep_int):
        if x is None:
            return None
        x = np.asarray(x)[order]
        return x if keep_int and x.dtype.kind == "i" else x.astype(np.float64)

    return [_np_one(name, gathered(f, True), gathered(w, False), gathered(aux, True), order, start) for name, f, w, aux in ops]


def _out_is_int(name, f):
    return name in _INT_OUT or (name in ("MIN", "MAX", "FIRST_MINUS_LAST", "LAST_MINUS_FIRST", "MAX_DIFF") and _kind(f) == "i8")


def _raise_on_status(orphans, empty):
    if orphans:
        raise ValueError(f"{orphans} record(s) whose group id is not in coord")
    if empty:
        raise ValueError(f"{empty} coord id(s) without a record")


# ---- device path ------------------------------------------------------------------------------------------------------
_DTYPE = {"f4": _lib.TF_F32, "f8": _lib.TF_F64, "i8": _lib.TF_I64}


def group_reduce_call(ids, coord_dev, ops, outs, status, tag="group_reduce"):
    """one tf_group_reduce call on contiguous device tensors (no checks beyond the library's own): ops as (name, f, w, aux)"""
    L = _lib.lib()
    n, n_groups = int(ids.shape[0]), int(coord_dev.shape[0])
    table = (_lib.GroupOp * max(len(ops), 1))()
    for entry, (name, f, w, aux), out in zip(table, ops, outs):
        entry.op = _lib.GROUP_OPS[name]
        for field, col in (("f", f), ("w", w), ("aux", aux)):
            setattr(entry, field, None if col is None else col.data_ptr())
            setattr(entry, field + "_dtype", _lib.TF_F64 if col is None else _DTYPE[_kind(col)])
        entry.out = out.data_ptr()
    nbytes = L.tf_group_reduce_workspace_bytes(n, n_groups)
    if nbytes == 0:
        raise ValueError("tf_group_reduce: more than 2^31 - 3 records or groups")
    ws = _lib.workspace(nbytes, tag)
    _lib.check(L.tf_group_reduce(_lib.ptr(ids), _lib.TF_I32 if _kind(ids) == "i4" else _lib.TF_I64, n, _lib.ptr(coord_dev), n_groups,
                                 table, len(ops), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_group_reduce")


def _dev_reduce(groups, coord, ops):
    t = _lib.torch()
    dev = _lib.device()
    ids = groups.to(dev)
    if _kind(ids) not in ("i4", "i8"):
        ids = ids.to(t.int64)
    ids = ids.contiguous()
    wide = _kind(ids) == "i8"
    if not wide and coord.size and (int(coord[-1]) > 2 ** 31 - 1 or int(coord[0]) < -2 ** 31):
        ids, wide = ids.to(t.int64), True
    coord_dev = t.from_numpy(np.ascontiguousarray(coord, np.int64 if wide else np.int32)).to(dev)
    n_groups = int(coord.size)

    def dev_col(x):
        return None if x is None else x.to(dev).contiguous()

    ops = [(name, dev_col(f), dev_col(w), dev_col(aux)) for name, f, w, aux in ops]
    outs = [t.empty(n_groups, dtype=t.int64 if _out_is_int(name, f) else t.float64, device=dev) for name, f, _, _ in ops]
    status = t.empty(2, dtype=t.int64, device=dev)
    for at in range(0, max(len(ops), 1), _lib.GROUP_MAX_OPS):
        group_reduce_call(ids, coord_dev, ops[at:at + _lib.GROUP_MAX_OPS], outs[at:at + _lib.GROUP_MAX_OPS], status)
    orphans, empty = (int(v) for v in status.cpu())
    _raise_on_status(orphans, empty)
    return outs


def reduce_groups(groups, coord, ops):
    """the operations `ops` per group id of `coord` over the records' `groups` column; see the module docstring"""
    if not _lib.is_tensor(groups):
        groups = np.asarray(groups)
    coord, ops = check_inputs(groups, coord, ops)
    tensors = [_lib.is_tensor(c) for op in ops for c in op[1:] if c is not None] + [_lib.is_tensor(groups)]
    if any(tensors) != all(tensors):
        raise TypeError("the columns of one table are all device tensors or all NumPy arrays")
    return _dev_reduce(groups, coord, ops) if tensors[0] else _np_reduce(groups, coord, ops)


def take(column, pick, missing=0):
    """column[pick] with `missing` where pick is -1; numpy or device"""
    if _lib.is_tensor(pick):
        t = _lib.torch()
        got = column.to(pick.device)[pick.clamp(min=0)]
        return t.where(pick >= 0, got, t.full_like(got, missing))
    column = np.asarray(column)
    got = column[np.maximum(pick, 0)]
    return np.where(pick >= 0, got, np.array(missing).astype(column.dtype)) if pick.size else got
