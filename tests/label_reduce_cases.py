"""Cases of the generic per-label reductions (labeled_comprehension / apply_func_to_labels with a recognised reducer):
plain NumPy inputs, shared by tests/golden/make_label_reduce_golden.py (which hands them to the reference), the CPU
restatement and the GPU tests.  The shapes are the smallest at which the kernels can still go wrong: a tail that is no
multiple of 4, a plane with hw % 4 != 0 and one with hw < 4, the workgroup seam at voxel 4096, one voxel.

A case is a dict: labels (int32), field (broadcasts against labels), index (array or None), default, dtype (or None),
offset (1: the GPU test hands the volume over through a view that starts one element into a larger buffer), apply (False:
the case is for labeled_comprehension only).  The float32 fields hold positive values (plus the listed specials), so a
bound relative to the result is meaningful for the sums."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "label_reduce_ref.npz")

REDUCERS = {"sum": np.sum, "nansum": np.nansum, "mean": np.mean, "nanmean": np.nanmean, "std": np.std, "nanstd": np.nanstd,
            "var": np.var, "nanvar": np.nanvar, "min": np.min, "max": np.max, "nanmin": np.nanmin, "nanmax": np.nanmax,
            "ptp": np.ptp, "any": np.any, "all": np.all, "count_nonzero": np.count_nonzero, "size": np.size, "len": len,
            "median": np.median, "nanmedian": np.nanmedian}
EXACT = ("min", "max", "nanmin", "nanmax", "ptp", "any", "all", "count_nonzero", "size", "len", "median", "nanmedian")
SUMS = ("sum", "nansum", "mean", "nanmean")
SPREADS = ("std", "nanstd", "var", "nanvar")
SHAPE = (3, 5, 67)                                                # n = 1005: no multiple of 4; hw = 335: neither


def _run_labels(shape, rng, n_ids=14, background=0.4):
    """runs of equal labels of random length along the raveled volume, ids 1 .. n_ids"""
    n = int(np.prod(shape))
    flat = np.zeros(n, np.int32)
    i = 0
    while i < n:
        length = int(rng.integers(1, 40))
        flat[i:i + length] = 0 if rng.random() < background else rng.integers(1, n_ids + 1)
        i += length
    return flat.reshape(shape)


def _tail_volume():
    """(labels, float32 field): the specials sit in regions of their own, ids 15 .. 30 written over the runs"""
    rng = np.random.default_rng(5)
    labels = _run_labels(SHAPE, rng)
    field = (200 + 100 * rng.random(SHAPE)).astype(np.float32)    # sums that are not exact in float32
    flat, x = labels.reshape(-1), field.reshape(-1)
    exact = flat == 3
    x[exact] = (1600 + rng.integers(0, 800, int(exact.sum()))).astype(np.float32) / 8      # small integers / 8: exact sums
    at = [600]

    def region(label, values):
        k = at[0]
        flat[k:k + len(values)] = label
        x[k:k + len(values)] = values
        flat[k + len(values)] = 0
        at[0] += len(values) + 1

    nan, inf = np.nan, np.inf
    region(15, [210.5, nan, 230.25, 220.0])                       # a NaN inside
    region(16, [nan, nan, nan])                                   # all NaN
    region(17, [250.0, inf, 201.0])
    region(18, [-inf, 250.0, 260.5])
    region(19, [inf, 222.0, -inf, 240.0])                         # both
    region(20, [0.0, -0.0, 0.0])                                  # zeros only: any / all / count_nonzero
    region(21, [-0.0, 1e-40, 3.0])                                # a zero, a denormal
    region(22, [231.5])                                           # 1, 2, 3, 4 values
    region(23, [231.5, 212.25])
    region(24, [231.5, 212.25, 250.0])
    region(25, [231.5, 212.25, 250.0, 212.25])
    region(26, [240.5, 220.5, 240.5, 220.5, 240.5, 220.5])        # ties at the median (even count)
    region(27, [240.5, 240.5, 240.5, 220.5, 260.0])               # ties at the median (odd count)
    region(28, [250.5] * 7)                                       # equal values: variance exactly 0
    return labels, field


def build():
    """{name: case}"""
    rng = np.random.default_rng(11)
    nan = np.nan
    labels, field = _tail_volume()
    T, H, W = SHAPE
    cases = {}

    def case(name, labels, field, index=None, default=nan, dtype=None, offset=0, apply=True):
        cases[name] = dict(labels=np.ascontiguousarray(labels, np.int32), field=np.ascontiguousarray(field),
                           index=None if index is None else np.asarray(index, np.int64), default=default, dtype=dtype,
                           offset=offset, apply=apply)

    case("tail_f32", labels, field)
    case("tail_f32_misaligned", labels, field, offset=1)
    case("index_mixed", labels, field, index=[7, 3, 3, 0, -4, 99999, 5, 29, 15, 2, 31])   # 29: absent, 31: above the largest
    case("empty_index", labels, field, index=[])
    finite = np.where(np.isfinite(field), field, np.float32(205.75))
    case("as_int32", labels, finite, dtype=np.int32, default=0)
    # layouts: one plane for every frame (float64 values that differ only below float32 precision), one value per frame
    plane = 1.0 + rng.integers(0, 32, (H, W)) * 2.0 ** -40
    case("plane_f64", labels, plane)
    case("plane_f64_misaligned", labels, plane[None], offset=1)
    small = np.array([[1, 1, 2], [2, 2, 0], [1, 0, 3], [3, 3, 3], [0, 2, 1]], np.int32).reshape(5, 1, 3)
    case("plane_small", small, (200 + rng.random((1, 3))).astype(np.float32))
    case("frame_f32", labels, np.array([250.5, nan, 210.25], np.float32)[:, None, None])
    # seams: one label across the workgroup seam at 4096, labels that change inside and exactly at 4- and 16-voxel
    # boundaries; a region of 4101 voxels for the order statistics
    seam = np.zeros((1, 1, 4101), np.int32)
    seam[0, 0, 4090:4101] = 1
    seam[0, 0, 0:4] = 2
    seam[0, 0, 4:16] = 3
    seam[0, 0, 16:18] = 2
    seam[0, 0, 18:37] = 4
    seam[0, 0, 1022:1026] = 5                                     # across a wave's 1024 voxels
    seam[0, 0, 250:262] = 6                                       # across a step's 256 voxels
    seam_field = (200 + 100 * rng.random((1, 1, 4101))).astype(np.float32)
    case("seams", seam, seam_field)
    case("seam_region", np.full((1, 1, 4101), 5, np.int32), seam_field)
    # degenerate
    case("one_labelled", np.ones((1, 1, 1), np.int32), np.full((1, 1, 1), 231.5, np.float32))
    case("one_unlabelled", np.zeros((1, 1, 1), np.int32), np.full((1, 1, 1), 231.5, np.float32))
    case("all_background", np.zeros((2, 3, 5), np.int32), (200 + rng.random((2, 3, 5))).astype(np.float32), index=[1, 2], default=0)
    # ids: up to 70 001 with sparse presence, index=None for both functions
    sparse = np.zeros((2, 8, 16), np.int32)
    sparse[0, 2:4, 3:9] = 3
    sparse[1, 5, 1:15] = 70001
    sparse[1, 0:2, 7:9] = 40000
    case("sparse_ids", sparse, (200 + 100 * rng.random((2, 8, 16))).astype(np.float32))
    # integer and bool fields
    ints = rng.integers(-50, 50, SHAPE).astype(np.int32)
    ints.reshape(-1)[labels.reshape(-1) == 4] = np.iinfo(np.int32).max
    ints.reshape(-1)[np.flatnonzero(labels.reshape(-1) == 5)[::2]] = np.iinfo(np.int32).min
    ints.reshape(-1)[np.flatnonzero(labels.reshape(-1) == 6)] = np.iinfo(np.int32).max
    ints.reshape(-1)[np.flatnonzero(labels.reshape(-1) == 6)[:1]] = np.iinfo(np.int32).min
    case("int32_extremes", labels, ints, default=0)
    case("int32_as_f64", labels, ints, default=nan, dtype=np.float64)
    case("bool_field", labels, rng.random(SHAPE) < 0.7, default=False)
    negative = labels.copy()
    negative[labels == 2] = -3
    case("negative_labels", negative, field, apply=False)
    return cases


def mode_cases():
    """{name: (labels, int32 field, index, background)} for find_overlap_mode: a tie (the smaller value wins), a region of
    background only, background=2"""
    labels = np.zeros((2, 4, 9), np.int32)
    labels[0, :2] = 1
    labels[0, 2:] = 2
    labels[1, :, :4] = 3
    labels[1, :, 5:] = 5
    field = np.zeros((2, 4, 9), np.int32)
    field[0, 0, :4] = 7
    field[0, 1, :4] = 4                                           # label 1: four 7s, four 4s, ten 0s -> 4
    field[0, 2:, :] = 2                                           # label 2: 2 only
    field[1, :, :2] = 9
    field[1, 0, 2] = 2                                            # label 3: eight 9s, one 2, zeros
    index = np.array([1, 2, 3, 4, 5, 6], np.int64)                # 5: background only; 4, 6: absent
    return {"mode_bg0": (labels, field, index, 0), "mode_bg2": (labels, field, index, 2)}


def golden():
    return np.load(GOLDEN)


# ---- what a result is held to ------------------------------------------------------------------------------------------
U64, U32 = 2.0 ** -53, 2.0 ** -24


def expected_error(gold, key):
    """the exception type the reference raised for `key`, or None"""
    for e in gold["errors"]:
        k, kind = str(e).split(":")
        if k == key:
            return {"ValueError": ValueError, "IndexError": IndexError, "OverflowError": OverflowError, "TypeError": TypeError}[kind]
    return None


def ids_of(fn, c):
    """the label ids a call works on: `index`, or the reference's default for labeled_comprehension ("lc": the distinct
    non-zero labels) and apply_func_to_labels ("af": 1 .. the largest label)"""
    if c["index"] is not None:
        return c["index"]
    labels = c["labels"]
    return np.unique(labels[labels != 0]) if fn == "lc" else np.arange(1, max(int(labels.max()), 0) + 1)


def hold(fn, name, reducer, got, c, gold):
    """`got` (NumPy) against the reference's own result gold[fn/name/reducer]: shape and dtype; the exact classes equal; the
    bounded classes (sums, means, variances of float fields; variances of integer fields) equal where the reference is not
    finite or the id has no voxel, and elsewhere within the contract's bound of float64 NumPy plus the one rounding to the
    result's dtype and -- for a reference value computed in float32 -- within (n + 4) 2^-24 relative of it.  Returns the largest
    observed share of the bounds, for the test to print."""
    import scipy.ndimage as ndi
    want = gold[f"{fn}/{name}/{reducer}"]
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (fn, name, reducer, got.shape, got.dtype, want.shape, want.dtype)
    field, labels = c["field"], c["labels"]
    integer = field.dtype.kind in "iub"
    if reducer in EXACT or (integer and reducer in SUMS):
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), (fn, name, reducer)
        return 0.0
    ids = np.asarray(ids_of(fn, c)).reshape(-1)
    lab, x = np.broadcast_arrays(labels, field.astype(np.float64))
    with np.errstate(all="ignore"):
        truth = ndi.labeled_comprehension(x, lab, ids, REDUCERS[reducer], np.float64, np.nan)
        n = ndi.labeled_comprehension(x, lab, ids, np.size, np.float64, 0)
        kept = ndi.labeled_comprehension(x, lab, ids, lambda v: np.sum(~np.isnan(v)), np.float64, 0)
        a = ndi.labeled_comprehension(x, lab, ids, lambda v: np.nansum(np.abs(v)), np.float64, 0)
    g, w = got.reshape(-1).astype(np.float64), want.reshape(-1).astype(np.float64)
    bounded = (n > 0) & np.isfinite(w) & np.isfinite(truth)
    assert np.array_equal(g[~bounded], w[~bounded], equal_nan=True), (fn, name, reducer)
    if want.dtype.kind != "f":                                    # a result cast to an integer dtype: NumPy's cast of the truth
        with np.errstate(all="ignore"):
            assert np.array_equal(g[bounded], truth[bounded].astype(want.dtype)) and np.all(np.abs(g - w)[bounded] <= 1), (fn, name, reducer)
        return 0.0
    ref32 = field.dtype == np.float32                             # the reference's value was computed in float32
    rounding = U32 if want.dtype == np.float32 or (fn == "af" and ref32) else U64       # af rounds to NumPy's result dtype
    if reducer in SUMS:
        bound = n * U64 * a / (np.maximum(kept, 1) if "mean" in reducer else 1) + (rounding + U64) * np.abs(truth)
    else:
        bound = (32 * n * U64 + rounding) * np.abs(truth)
    err = np.abs(g - truth)
    assert np.all(err[bounded] <= bound[bounded]), (fn, name, reducer, float(np.max((err / bound)[bounded & (bound > 0)], initial=0)))
    share = float(np.max((err / bound)[bounded & (bound > 0)], initial=0))
    if ref32:
        near = (n + 4) * U32 * np.abs(w)
        off = np.abs(g - w)
        assert np.all(off[bounded] <= near[bounded]), (fn, name, reducer, float(np.max((off / near)[bounded & (near > 0)], initial=0)))
        share = max(share, float(np.max((off / near)[bounded & (near > 0)], initial=0)))
    return share
