"""Cases and expected values for calculate_label_properties, get_label_stats and n_unique_along_axis.

The reference cannot be imported (it needs xarray), so what its dataset.py:705-1595, analysis.py:245-290 and
utils/stats_utils.py:23-30 compute is restated here with one plain numpy loop per label, sums in float64 --
test_props_cases_cpu.py holds this restatement against the reference's own primitives (scipy.ndimage.labeled_comprehension,
np.bincount, np.average on materialised stacks) called directly; the unique counts are counted with a Python set per line.  The GPU tests compare the
package with it."""
import functools

import numpy as np
import scipy.ndimage as ndi

from oracle import np_dataset

KINDS = (("core", "core"), ("thick_anvil", "anvil"), ("thin_anvil", "anvil"))
SHAPES = ((6, 40, 50), (5, 33, 67))
NAT = np.datetime64("NaT", "ns")


def same_times(a, b):
    """equality of two datetime64 / timedelta64 arrays with NaT equal to NaT"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.dtype.kind in "mM" and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def volumes(seed, shape=(6, 40, 50), density=0.35):
    """cores inside thick anvils inside thin anvils, like a detection output (the recipe of tests/test_gpu_dataset.py)"""
    rng = np.random.default_rng(seed)
    sm = ndi.gaussian_filter(rng.normal(size=shape), (0.7, 2.5, 2.5))
    thin = ndi.label(sm > np.quantile(sm, 1 - density))[0].astype(np.int32)
    thick = ndi.label(sm > np.quantile(sm, 1 - 0.6 * density))[0].astype(np.int32)
    core = ndi.label(sm > np.quantile(sm, 1 - 0.25 * density))[0].astype(np.int32)
    return core, thick, np.where(thick != 0, thick, thin + (thick.max() if thin.max() else 0) * (thin != 0)).astype(np.int32)


def grid(shape, seed=0, dtype=np.float64):
    """area (positive, varying), signed lat / lon planes, signed x / y vectors and an ascending t of a (T, H, W) case"""
    T, H, W = shape
    rng = np.random.default_rng(1000 + seed)
    y = np.linspace(0.09, -0.04, H)
    x = np.linspace(-0.07, 0.11, W)
    yy, xx = np.meshgrid(y, x, indexing="ij")
    lat = 400.0 * yy + 3.0 * np.sin(9.0 * xx)
    lon = -75.0 + 500.0 * xx - 40.0 * yy ** 2
    area = 4.0 / np.cos(2.0 * yy + xx) ** 2 * (1.0 + 0.05 * rng.random((H, W)))
    t = np.datetime64("2020-06-01T00:00", "ns") + np.arange(T) * np.timedelta64(600, "s")
    return {"area": area.astype(dtype), "lat": lat.astype(dtype), "lon": lon.astype(dtype), "x": x.astype(dtype),
            "y": y.astype(dtype), "t": t}


@functools.lru_cache(maxsize=None)
def _linked_case(seed, shape):
    core, thick, thin = volumes(seed, shape)
    ref = {"core_label": core.copy(), "thick_anvil_label": thick.copy(), "thin_anvil_label": thin.copy(), "coords": {}}
    np_dataset.add_label_coords(ref)
    np_dataset.link_cores_and_anvils(ref)
    np_dataset.add_step_labels(ref)
    np_dataset.add_label_coords(ref)
    np_dataset.link_step_labels(ref)
    return (core, thick, thin), ref


def raw_volumes(seed, shape):
    """the three label volumes before the script's steps (fresh copies)"""
    return tuple(v.copy() for v in _linked_case(seed, shape)[0])


def linked_case(seed, shape, dtype=np.float64, **overrides):
    """A case after the script's order (add_label_coords, link_cores_and_anvils, add_step_labels, add_label_coords,
    link_step_labels), made by the oracle's restatement of those steps: {name: array} plus "coords".  The label arrays
    are shared between calls and must not be written to."""
    ref = dict(_linked_case(seed, shape)[1])
    g = grid(shape, seed, dtype)
    g.update(overrides)
    ref["coords"] = dict(ref["coords"], x=g["x"], y=g["y"], t=g["t"])
    ref.update(area=g["area"], lat=g["lat"], lon=g["lon"])
    return ref


def with_nan_area(case):
    """one NaN area pixel inside a core (so inside an anvil too) (the first labelled pixel), one outside any region"""
    area = case["area"].copy()
    inside = np.argwhere(case["core_step_label"] != 0)[0]
    outside = np.argwhere(case["thin_anvil_label"].max(0) == 0)[0]
    area[inside[1], inside[2]] = np.nan
    area[outside[0], outside[1]] = np.nan
    return dict(case, area=area)


def _planes(case):
    lat, lon = np.asarray(case["lat"]), np.asarray(case["lon"])
    if lat.ndim == 1:                                             # dataset.py:1256-1259
        lon, lat = np.meshgrid(lon, lat)
    return np.asarray(case["area"]), lat, lon


def per_label(labels, ids, case, summing=np.float64, locations=True):
    """count, nansum of the area, first / last time and the four area-weighted means of every id, one loop pass per
    label.  summing=np.float64: explicit float64 sums.  summing=np.float32: the operands as float32 through numpy's own
    float32 np.nansum / np.average, i.e. what the reference's calls give for float32 inputs.  locations=False leaves the
    means out (the reference takes them of the step volumes only)."""
    area, lat, lon = _planes(case)
    x, y, t = (np.asarray(case["coords"][c]) for c in ("x", "y", "t"))
    n = len(ids)
    out = {"count": np.zeros(n, np.int64), "area": np.full(n, np.nan), "tmin": np.full(n, NAT), "tmax": np.full(n, NAT),
           "x": np.full(n, np.nan), "y": np.full(n, np.nan), "lat": np.full(n, np.nan), "lon": np.full(n, np.nan)}
    for k, i in enumerate(ids):
        tt, yy, xx = np.nonzero(labels == i)
        if tt.size == 0:
            continue
        a = area[yy, xx].astype(summing)
        out["count"][k] = tt.size
        out["tmin"][k], out["tmax"][k] = t[tt].min(), t[tt].max()
        values = {"x": x[xx], "y": y[yy], "lat": lat[yy, xx], "lon": lon[yy, xx]} if locations else {}
        if summing == np.float64:
            out["area"][k] = a[~np.isnan(a)].sum()
            if locations and a.sum() == 0:
                raise ZeroDivisionError("Weights sum to zero, can't be normalized")
            for c, v in values.items():
                out[c][k] = (a * v.astype(np.float64)).sum() / a.sum()
        else:
            out["area"][k] = np.nansum(a)
            for c, v in values.items():
                out[c][k] = np.average(v.astype(summing), weights=a)
    return out


def first_max_step(step_ids, step_parent, step_area, parents):
    """positions chosen by `step[parent == i][np.argmax(area[parent == i])]` (dataset.py:771-778), steps taken in
    ascending id order"""
    order = np.argsort(step_ids, kind="stable")
    out = []
    for i in parents:
        sel = order[np.asarray(step_parent)[order] == i]
        out.append(sel[np.argmax(np.asarray(step_area)[sel])])
    return np.asarray(out, np.int64)


def first_step(step_ids, step_parent, parents):
    """positions chosen by np.nanmin(step[parent == i]) (dataset.py:1334-1339)"""
    out = []
    for i in parents:
        sel = np.nonzero(np.asarray(step_parent) == i)[0]
        out.append(sel[np.argmin(np.asarray(step_ids)[sel])])          # ValueError on an empty selection, as np.nanmin
    return np.asarray(out, np.int64)


def expected_properties(case, summing=np.float64):
    """{name: (dims, array)} of every variable calculate_label_properties writes (dataset.py:705-1595, the commented-out
    ones left out), from per_label and the two per-core choices"""
    out = {}
    f32 = lambda v: np.asarray(v).astype(np.float32)              # noqa: E731
    steps = {}
    for kind, dim in KINDS:
        ids, step_ids = case["coords"][dim], case["coords"][kind + "_step"]
        p = per_label(case[kind + "_label"], ids, case, summing, locations=False)
        s = steps[kind] = per_label(case[kind + "_step_label"], step_ids, case, summing)
        if kind == "core":
            out["core_pixel_count"] = (("core",), p["count"].astype(np.int32))
        if kind != "thin_anvil":
            out[kind + "_total_area"] = ((dim,), f32(p["area"]))
        out[kind + "_start_t"] = ((dim,), p["tmin"])
        out[kind + "_end_t"] = ((dim,), p["tmax"])
        out[kind + "_lifetime"] = ((dim,), p["tmax"] - p["tmin"])
        d = (kind + "_step",)
        out[kind + "_step_pixel_count"] = (d, s["count"].astype(np.int32))
        out[kind + "_step_area"] = (d, f32(s["area"]))
        out[kind + "_step_t"] = (d, s["tmin"])
        for c in ("x", "y", "lat", "lon"):
            out[f"{kind}_step_{c}"] = (d, f32(s[c]))
    core, core_step, parent = case["coords"]["core"], case["coords"]["core_step"], case["core_step_core_index"]
    widest = first_max_step(core_step, parent, out["core_step_area"][1], core)
    out["core_max_area"] = (("core",), out["core_step_area"][1][widest])
    out["core_max_area_t"] = (("core",), out["core_step_t"][1][widest])
    first = first_step(core_step, parent, core)
    for c in ("x", "y", "lat", "lon"):
        out[f"core_start_{c}"] = (("core",), out[f"core_step_{c}"][1][first])
    return out


# ---- unique counts -----------------------------------------------------------------------------------------------------
def distinct_nonzero(a, axis=0):
    """number of distinct non-zero values along `axis`, by a Python set per line"""
    moved = np.moveaxis(np.asarray(a), axis, 0)
    flat = moved.reshape(moved.shape[0], -1)
    out = np.array([len(set(flat[:, j].tolist()) - {0}) for j in range(flat.shape[1])], np.int64)
    return out.reshape(moved.shape[1:])


def column_volume(T, seed=0, negatives=True):
    """(T, 3, 70) int32: row 0 holds hand-made columns at x = 0 .. 5 -- a,0,a / a,b,a / no zero at all / all T values
    distinct / all zero / (with `negatives`) negative ids -- and random sparse labels everywhere else"""
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, 9, (T, 3, 70)) * (rng.random((T, 3, 70)) < 0.6)).astype(np.int32)
    a, b = 7, 3
    v[:, 0, 0] = np.resize([a, 0, a], T)
    v[:, 0, 1] = np.resize([a, b, a], T)
    v[:, 0, 2] = np.resize([a, a, b, b, 5], T)
    v[:, 0, 3] = 100 + np.arange(T)
    v[:, 0, 4] = 0
    if negatives:
        v[:, 0, 5] = np.resize([-2, 0, -2, -5], T)
    return v
