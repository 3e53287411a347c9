"""Cases, yardstick and bounds for get_bulk_stats / get_spatial_stats / get_temporal_stats (tf_field_stats).

Everything is seeded and exists as float32 and as float64.  A case is a named (t, y, x) volume; a geometry cuts it into
slices: "all" (one slice), "frame" (one per t) or "time" (one per pixel).

The yardstick.  Per slice, over the float64-widened non-NaN values x_1 .. x_n:
  count n, max, min, and the median of the values in the field's own dtype (np.sort; (a + b) rounded in that dtype, then
  halved -- the mean of two that np.median takes), all exact;
  m^ = fsum(x) / n and s^ = sqrt(fsum((x - m^)^2) / n), math.fsum being the exactly rounded sum.  A slice that holds an
  infinity takes NumPy's float64 nanmean / nanstd, which is IEEE arithmetic on inf and NaN: the contract there is "the same
  NaN or infinity", not a bound.

The bounds (u = 2^-53).  The device adds n float64 values in SOME order that is fixed by the shape.  Whatever the order,
every partial sum is bounded by sum|x| and each of the n - 1 additions rounds once, so the computed sum is off by at most
(n - 1) u sum|x| (Higham, Accuracy and Stability, (4.4), to first order); the mean divides by n, exactly up to one more
rounding of the result:
    |mean - m^| <= eps_m = n u (sum|x| / n) + u |m^|
(the second term also covers the rounding of the yardstick's own division).  For the deviations, with mean = m^ + e,
|e| <= eps_m:  sum (x - mean)^2 = sum (x - m^)^2 + n e^2, so the exact root about the device's centre is at most
sqrt(v + e^2) <= sqrt(v) + |e| = s^ + eps_m.  Each term (x - mean)^2 carries two roundings (relative 2 u + ..), the sum of n
non-negative terms at most (n - 1) u relative, the division and the root one each; the root halves a relative error, so
(2 + n - 1 + 1) / 2 + 1 < n + 8 with room for the yardstick's own four roundings:
    |std - s^| <= (n + 8) u s^ + eps_m
A public float32 result is the float32 rounding of such a value: |got - y^| <= bound + ulp32(y^) / 2.

NumPy's own float32 results (the fixture) are held to what float32 summation can promise: pairwise inside blocks of 128 and,
at worst, one after the other across blocks and along a strided axis: `f32_depth` roundings of relative size 2^-24.
"""
import functools
import hashlib
import math
import os

import numpy as np

from tobac_flow_amd.ndimage_dev import FIELD_STATS_LDS_FRAMES

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "field_stats_ref.npz")
DTYPES = ("float32", "float64")
GEOMETRIES = ("all", "frame", "time")
STATS = ("mean", "std", "median", "max", "min")
U = 2.0 ** -53
PLAIN_SHAPES = ((1, 1, 1), (1, 1, 7), (2, 5, 13), (3, 63, 65), (4, 129, 257))
SPECIAL_LENGTHS = (16, 1200)           # plus FIELD_STATS_LDS_FRAMES[dtype]


def lds_frames(dtype):
    return FIELD_STATS_LDS_FRAMES[np.dtype(dtype)]


def frame_counts(dtype):
    L = lds_frames(dtype)
    return (1, 2, 3, 16, 17, L, L + 1, 2 * L + 3)


# ---- contents ------------------------------------------------------------------------------------------------------------
def near(rng, shape, dtype):
    return (250.0 + 20.0 * rng.standard_normal(shape)).astype(dtype)


def mixed(rng, shape, dtype):
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-30, 30, shape)).astype(dtype)


def special_slices(n, dtype, seed):
    """{name: vector of n values}; n even and >= 16.  What each is for is its name."""
    assert n % 2 == 0 and n >= 16
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    fi = np.finfo(dtype)
    out = {}

    def shuffled(*parts):
        v = np.concatenate([np.asarray(p, dtype).ravel() for p in parts])
        assert v.size == n, (v.size, n)
        return rng.permutation(v)

    def with_nans(k):
        v = near(rng, n, dtype)
        v[rng.choice(n, k, replace=False)] = np.nan
        return v

    h = (n - 2) // 2
    lows, highs = lambda k: 100 + rng.random(k), lambda k: 300 + rng.random(k)       # noqa: E731
    out["all_nan"] = np.full(n, np.nan, dtype)
    out["one_value"] = with_nans(n - 1)
    out["even_count"] = with_nans(4)
    out["odd_count"] = with_nans(3)
    c = dtype.type(250.1)
    out["last_bit"] = shuffled(lows(h), highs(h), [c, np.nextafter(c, dtype.type(np.inf))])
    d = 1000 if n >= 1200 else n // 2
    out["duplicates"] = shuffled(lows((n - d) // 2), np.full(d, 250.0), highs(n - d - (n - d) // 2))
    out["constant"] = np.full(n, 251.375, dtype)
    out["negative"] = -near(rng, n, dtype)
    out["plus_inf"] = shuffled(near(rng, n - 1, dtype), [np.inf])
    out["both_inf"] = shuffled(near(rng, n - 2, dtype), [np.inf, -np.inf])
    tiny = fi.smallest_subnormal
    out["subnormal"] = shuffled((np.arange(n) - n // 3).astype(np.float64) * float(tiny))
    big = np.finfo(np.float32).max                # the two middle values' float32 sum overflows; every float64 sum stays finite
    out["overflow_pair"] = shuffled(-lows(h), [0.75 * big, 0.75 * big], np.full(h, 0.9 * big))
    out["signed_zero"] = shuffled(np.full(n // 4, -1.0), np.full(n // 4, 0.0), np.full(n // 4, -0.0), np.full(n - 3 * (n // 4), 1.0))
    for v in out.values():
        assert v.dtype == dtype and v.shape == (n,)
    return out


def _frame_shape(n):
    h = 4 if n == 16 else 30 if n == 1200 else 8
    assert n % h == 0
    return h, n // h


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """{name: (t, y, x) array of `dtype`}, read-only"""
    dtype = np.dtype(dtype)
    out = {}
    for i, shape in enumerate(PLAIN_SHAPES):
        out["near_%dx%dx%d" % shape] = near(np.random.default_rng(100 + i), shape, dtype)
        out["mixed_%dx%dx%d" % shape] = mixed(np.random.default_rng(200 + i), shape, dtype)
    for T in frame_counts(dtype):
        out["near_T%d" % T] = near(np.random.default_rng(300 + T), (T, 3, 67), dtype)
    out["mixed_T%d" % frame_counts(dtype)[-1]] = mixed(np.random.default_rng(400), (frame_counts(dtype)[-1], 3, 67), dtype)
    # a pixel column without a value and a frame without a value in an ordinary volume
    v = near(np.random.default_rng(500), (5, 9, 11), dtype)
    v[:, 4, 7] = np.nan
    v[2] = np.nan
    v[0, 0, :3] = np.nan
    out["nan_frame_and_column"] = v
    for n in SPECIAL_LENGTHS + (lds_frames(dtype),):
        sp = special_slices(n, dtype, 600 + n)
        names = sorted(sp)
        stack = np.stack([sp[k] for k in names])                                   # (K, n)
        out["special_frames_n%d" % n] = stack.reshape((len(names),) + _frame_shape(n)).copy()
        # the same slices as pixel columns, in two rows (the second row in reverse column order)
        cols = stack.T                                                              # (n, K)
        out["special_columns_n%d" % n] = np.stack([cols, cols[:, ::-1]], 1).copy()  # (n, 2, K)
        for k in names:
            out["special_%s_n%d" % (k, n)] = sp[k].reshape(1, 1, n).copy()          # for the bulk form
    for a in out.values():
        a.setflags(write=False)
    return out


def special_names():
    return sorted(special_slices(16, "float32", 0))


def geometries_of(name):
    """the geometries a case is meant for (the special stacks are built for one each; the rest take all three)"""
    if name.startswith("special_frames"):
        return ("frame",)
    if name.startswith("special_columns"):
        return ("time",)
    if name.startswith("special_"):
        return ("all",)
    return GEOMETRIES


def fingerprint(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- slices and the yardstick ----------------------------------------------------------------------------------------------
def slices(a, over):
    """(result shape, (S, n) view-or-copy of the slices)"""
    if over == "all":
        return (), a.reshape(1, -1)
    assert a.ndim == 3
    if over == "frame":
        return (a.shape[0],), a.reshape(a.shape[0], -1)
    return a.shape[1:], a.reshape(a.shape[0], -1).T


def _median_own_dtype(vals):
    """of non-NaN values in their own dtype, as np.median combines the middle: one value, or (a + b) rounded, then halved"""
    s = np.sort(vals)
    n = s.size
    if n % 2:
        return s[n // 2]
    with np.errstate(all="ignore"):
        return (s[n // 2 - 1] + s[n // 2]) / s.dtype.type(2)


def slice_yardstick(row, bulk):
    """{count, mean, std, median, max, min, sum_abs} of one slice; floats are Python floats (float64)"""
    keep = row[~np.isnan(row)]
    n = int(keep.size)
    nan = float("nan")
    if n == 0:
        return dict(count=0, mean=nan, std=nan, median=nan, max=nan, min=nan, sum_abs=0.0)
    x = keep.astype(np.float64)
    if np.isinf(x).any():
        with np.errstate(all="ignore"):
            mean, std = float(np.mean(x)), float(np.std(x))
        sum_abs = float("inf")
    else:
        mean = math.fsum(x) / n
        std = math.sqrt(math.fsum((x - mean) ** 2) / n)
        sum_abs = math.fsum(np.abs(x))
    median = nan if bulk and n != row.size else float(_median_own_dtype(keep))
    return dict(count=n, mean=mean, std=std, median=median, max=float(x.max()), min=float(x.min()), sum_abs=sum_abs)


@functools.lru_cache(maxsize=None)
def yardstick(name, dtype, over):
    """{key: float64 array of the result shape} for a case (computed once, shared, read-only); count is int64"""
    shape, rows = slices(cases(dtype)[name], over)
    recs = [slice_yardstick(r, over == "all") for r in rows]
    out = {k: np.array([r[k] for r in recs], np.int64 if k == "count" else np.float64).reshape(shape) for k in recs[0]}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def eps_mean(y):
    n = np.maximum(y["count"], 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return n * U * (y["sum_abs"] / n) + U * np.abs(y["mean"])


def bound(y, key):
    """the contract's bound on |got - yardstick| for the float64 results `mean` and `std` (NaN / inf where the yardstick is)"""
    if key == "mean":
        return eps_mean(y)
    with np.errstate(invalid="ignore"):
        return (y["count"] + 8.0) * U * y["std"] + eps_mean(y)


def half_ulp32(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def f32_depth(n, over):
    """roundings a float32 NumPy sum of n values can stack up: one after the other along t, pairwise inside blocks of 128
    (16 in a lane, 3 across lanes, the tree above) and at worst one after the other across them otherwise"""
    n = np.maximum(np.asarray(n, np.float64), 2)
    return n - 1 if over == "time" else np.minimum(n - 1, 32 + np.ceil(n / 128))


def numpy_bound(y, key, dtype, over):
    """what NumPy's own sums in `dtype` may differ from the yardstick by, result rounding included"""
    fi = np.finfo(dtype)
    u = float(fi.eps) / 2
    depth = f32_depth(y["count"], over)
    n = np.maximum(y["count"], 1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        # a sum of magnitudes beyond the format's range may overflow on the way: no promise then (infinite bound)
        e_mean = np.where(y["sum_abs"] > float(fi.max), np.inf, (depth + 2) * u * (y["sum_abs"] / n) + float(fi.smallest_subnormal))
        if key == "mean":
            return e_mean
        # x - mean, the square, the sum, the division, the root; the centre is off by e_mean.  The squares leave the
        # format's range above sqrt(max) (no promise) and lose their low bits below its smallest normal number
        top = np.maximum(np.abs(y["max"]), np.abs(y["min"]))
        e_std = (depth + 8) * u * y["std"] + e_mean + math.sqrt(float(fi.smallest_subnormal))
        return np.where(top * top * n > float(fi.max), np.inf, e_std)


def hold_values(got, want, what):
    """equal as values: NaN where NaN, +0.0 == -0.0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def hold_bound(got, want, tol, what):
    """|got - want| <= tol where want is finite (nothing is asked where tol is infinite); the same NaN or infinity elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    hold_values(np.where(fin, 0, got), np.where(fin, 0, want), what + " (non-finite)")
    fin = fin & np.isfinite(tol)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(got - want), 0)
        bad = fin & ~(err <= tol)
    worst = float(np.max(np.where(fin & (tol > 0), err / np.where(tol > 0, tol, 1), 0), initial=0))
    print(what, "largest error / bound:", worst)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5], tol[bad][:5])


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def fixture_cases(dtype):
    """the cases the fixture carries reference results for: everything but the largest plain volume (size limit)"""
    return [k for k in cases(dtype) if "4x129x257" not in k]


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
