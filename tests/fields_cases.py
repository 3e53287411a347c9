"""The NumPy restatement of the reference's field preparation and the cases the field tests share.

xarray is not installed, so the reference's loaders cannot be run; as for the point binning the yardstick is NumPy written
after the reference's lines (paths relative to the reference's tobac_flow/):

    decode                  xarray's CF decoding of a packed variable (mask the _FillValue, then raw * scale + offset in float32)
    stripe_deviation        dataloader.py:234-237 with xarray's skipna rule
    frame_table             goes_dataloader:78-94 (keep), load_mcmip:316-317 (sortby), :131-132 (duplicates),
                            fill_time_gap_nan:341-357 with create_nan_slice:324-338
    prepare                 load_mcmip:260-313, seviri_dataloader:640-653, seviri_nat_dataloader:875-884

Every case asserts while it is built that no row's deviation lies within MARGIN of the threshold: no flag hangs on rounding."""
import functools
import warnings
from datetime import timedelta

import numpy as np

THRESHOLD = 2.0
MARGIN = 1e-6
SHAPES = ((5, 37, 67), (2, 70, 1100), (1, 1030, 40))
VIEW = (slice(None), slice(3, -2), slice(5, -1))                  # the [3:-2, 5:-1] cut of a larger frame
VIEW_PAD = ((0, 0), (3, 2), (5, 1))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def stored(raw, unsigned):
    """the stored integers of an int16 array: as they are, or its bits as uint16 (netCDF's _Unsigned)"""
    return raw.view(np.uint16) if unsigned else raw


def decode(raw, scale, offset, fill=None, unsigned=False):
    """CF decoding: raw == fill gives NaN, anything else np.float32(raw) * np.float32(scale) + np.float32(offset); `fill`
    in the stored type"""
    s = stored(raw, unsigned)
    out = s.astype(np.float32) * np.float32(scale) + np.float32(offset)
    assert out.dtype == np.float32
    if fill is not None:
        out[s == fill] = np.nan
    return out


def dqf_float(dqf, fill=None):
    """a DQF plane as xarray hands it out when it has a _FillValue: float64, the fill NaN"""
    out = dqf.astype(np.float64)
    if fill is not None:
        out[dqf == fill] = np.nan
    return out


def stripe_terms(da):
    """(da - da.mean("y")) / (da.std("y") + 1e-8) of dataloader.py:237, skipna"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # all-NaN columns: NaN, as xarray gives without a warning
        y_mean = np.nanmean(da, 1, keepdims=True)
        y_std = np.nanstd(da, 1, keepdims=True)
    return (da - y_mean) / (y_std + 1e-8)


def stripe_deviation(da):
    """get_stripe_deviation (dataloader.py:234-237) of a float64 (T, H, W) plane: (T, H)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.abs(np.nanmean(stripe_terms(da), 2))


def stripe_deviation_kernel_form(dqf, fill=None):
    """the same as the kernels evaluate it: count and sum of the valid elements of a column as exact integers, the
    mean their quotient; the variance np.nanstd's second pass in its own order -- (D - mean)^2 added down the column row by
    row --; the row mean a plain float64 sum over the count.  Returns `(dev, mean, std)`."""
    valid = np.ones(dqf.shape, bool) if fill is None else dqf != fill
    n = valid.sum(1).astype(np.int64)
    s1 = np.where(valid, dqf.astype(np.int64), 0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        nf = n.astype(np.float64)
        mean = s1.astype(np.float64) / nf
        acc = np.zeros(mean.shape)
        for y in range(dqf.shape[1]):
            diff = dqf[:, y, :].astype(np.float64) - mean
            acc = acc + np.where(valid[:, y, :], diff * diff, 0.0)
        std = np.sqrt(acc / nf)
        terms = np.where(valid, (dqf.astype(np.float64) - mean[:, None]) / (std[:, None] + 1e-8), 0.0)
        count = valid.sum(2)
        return np.where(count > 0, np.abs(terms.sum(2) / count), np.nan), mean, std


def dev_bound(da):
    """how far a float64 row sum in another order, of terms rounded three times each, may lie from NumPy's: per row
    (W + 4) 2^-53 mean_x |term|"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return (da.shape[2] + 4) * 2.0 ** -53 * np.nanmean(np.abs(stripe_terms(da)), 2)


def get_datetime_from_coord(t):
    import pandas as pd
    return pd.to_datetime(np.asarray(t)).to_pydatetime().tolist()


def frame_table(t, time_gap=None, keep=None):
    """`(src, t_out)`: the frames the reference ends up with, as indices into the input (-1: a NaN slice), and their times"""
    t = np.asarray(t)
    idx = np.arange(t.size)
    if keep is not None and not np.all(keep):
        idx = idx[np.asarray(keep)]                               # bt[wh_valid_t]
    if idx.size > 1:
        idx = idx[np.argsort(t[idx], kind="stable")]              # bt.sortby(bt.t)
    ts = t[idx]
    if np.unique(ts).size < ts.size:
        raise RuntimeError("Duplicate time steps in input index values")
    if time_gap is None:
        return idx.astype(np.int32), ts
    where_time_gap = np.where(np.diff(get_datetime_from_coord(ts)) > time_gap)[0] if ts.size > 1 else np.zeros(0, int)
    src, t_out, last = [], [], 0
    for t_ind in where_time_gap:
        src += list(idx[last:t_ind + 1]) + [-1]
        t_out += list(ts[last:t_ind + 1]) + [ts[t_ind] + (ts[t_ind + 1] - ts[t_ind]) / 2]
        last = t_ind + 1
    src += list(idx[last:])
    t_out += list(ts[last:])
    return np.asarray(src, np.int32), np.asarray(t_out, dtype=t.dtype)


def prepare(channels, recipes, t, dqf=(), time_gap=None, keep=None, threshold=THRESHOLD):
    """The fields of `recipes` -- (a, b or None, floor or None) over the decoded float32 `channels` -- with the joint masks
    of load_mcmip:288-313 (`dqf`: float64 planes, fill NaN), then the frames of frame_table.  Returns
    `(fields, n_masked, t_out)`."""
    fields = []
    for a, b, floor in recipes:
        x = channels[a].copy() if b is None else channels[a] - channels[b]
        if floor is not None:
            x = np.maximum(x, np.float32(floor))
        assert x.dtype == np.float32
        fields.append(x)
    all_isnan = np.any([~np.isfinite(x) for x in fields], 0)
    for x in fields:
        x[all_isnan] = np.nan
    if len(dqf):
        all_dqf = np.any(list(dqf), 0)                            # NaN is true
        all_stripe = np.any([stripe_deviation(d) > threshold for d in dqf], 0)
        for x in fields:
            x[all_dqf] = np.nan
            x[all_stripe] = np.nan
    src, t_out = frame_table(t, time_gap, keep)
    out = []
    for x in fields:
        y = np.full((len(src),) + x.shape[1:], np.nan, np.float32)
        y[src >= 0] = x[src[src >= 0]]
        out.append(y)
    return out, np.isnan(out[0]).sum((1, 2)).astype(np.int32), t_out


# ---- cases -----------------------------------------------------------------------------------------------------------------
GOES_RECIPES = ((2, None, None), (0, 1, None), (2, 3, None))      # bt = C13, wvd = C08 - C10, swd = C13 - C15
SEVIRI_NAT_RECIPES = ((3, None, None), (0, 1, None), (2, 4, 0.0))  # bt = IR_108, wvd = WV_062 - WV_073, twd = max(IR_087 - IR_120, 0)
# scale_factor and add_offset of CMI_C08, C10, C13, C15 in an MCMIP file, _FillValue -1 on an _Unsigned short
GOES_PACKING = ((0.04224, 138.05), (0.04225, 126.91), (0.06145, 89.62), (0.05965, 97.38))
GOES_FILL = -1


def times(T, rng=None):
    """T scan times five minutes apart with one gap of 25 minutes (when T > 2), shuffled when `rng` is given"""
    minutes = np.arange(T) * 5
    if T > 2:
        minutes[T // 2:] += 20
    t = np.datetime64("2018-06-19T17:02:19.123456789") + minutes * np.timedelta64(60_000_000_001, "ns")
    return t[rng.permutation(T)] if rng is not None and T > 1 else t


def dqf_planes(shape, rng):
    """Four DQF planes, [(int array, fill or None)]: sparse flags everywhere; plane 0 (uint8) a full stripe row; plane 1
    (uint8) a partial stripe below the threshold and a constant column; plane 2 (int8, fill -1) fill values and a partial
    stripe above the threshold; plane 3 (uint8, fill 255) a column of nothing but fill"""
    T, H, W = shape
    planes = []
    for dtype, fill in ((np.uint8, None), (np.uint8, None), (np.int8, -1), (np.uint8, 255)):
        d = np.where(rng.random(shape) < 0.004, rng.integers(1, 4, shape), 0).astype(dtype)
        planes.append([d, fill])
    row = lambda k: (k * 7 + 3) % H
    planes[1][0][:, :, W // 2] = 2
    planes[2][0][rng.random(shape) < 0.003] = -1
    planes[3][0][rng.random(shape) < 0.003] = 255
    planes[3][0][:, :, W // 3] = 255
    planes[0][0][0, row(0), :] = 1

    def stripe(k, frame, value, from_right, wanted):
        """the shortest stripe in row(k) whose deviation is `wanted` (a predicate); lengths 2, 3, 4, 6, 8, 12, ..."""
        d, fill = planes[k]
        for n in sorted({min(W, m) for e in range(1, 12) for m in (2 ** e, 3 * 2 ** (e - 1))}):
            trial = d.copy()
            trial[frame, row(k), (W - n if from_right else 0):(W if from_right else n)] = value
            if wanted(stripe_deviation(dqf_float(trial, fill))[frame, row(k)]):
                planes[k][0] = trial
                return n
        raise AssertionError("no stripe length gives the wanted deviation")
    below = stripe(1, T - 1, 2, False, lambda dev: 1.0 < dev < 1.8)
    above = stripe(2, 0, 1, True, lambda dev: dev > 2.2)
    assert 2 <= below < W and above < W
    out = [(d, fill) for d, fill in planes]
    flagged = 0
    for d, fill in out:
        dev = stripe_deviation(dqf_float(d, fill))
        assert np.nanmin(np.abs(dev - THRESHOLD)) >= MARGIN, "a stripe row too close to the threshold"
        flagged += int((dev > THRESHOLD).sum())
    assert flagged >= 2, "the case flags a full and a partial stripe"
    assert not stripe_deviation(dqf_float(*out[1]))[T - 1, row(1)] > THRESHOLD, "the short stripe stays below the threshold"
    return out


@functools.lru_cache(maxsize=None)
def goes_case(shape, packed=True, seed=0):
    """A GOES-shaped case: four channels (packed unsigned int16 with fills in different channels, or float32 with NaN, +inf
    and -inf), four DQF planes, unsorted times with a gap; and what the restatement makes of it"""
    rng = np.random.default_rng([seed, *shape])
    raws, decoded = [], []
    for c, (scale, offset) in enumerate(GOES_PACKING):
        raw = rng.integers(900, 3600, shape).astype(np.uint16)
        raw[rng.random(shape) < 0.002 * (c + 1)] = 65535
        raw = raw.view(np.int16)
        raws.append(raw)
        decoded.append(decode(raw, scale, offset, 65535, unsigned=True))
    if not packed:
        for c, bad in enumerate((np.nan, np.inf, -np.inf, np.inf)):
            decoded[c][rng.random(shape) < 0.002] = bad
    dqf = dqf_planes(shape, rng)
    t = times(shape[0], rng)
    gap = timedelta(minutes=15)
    want, n_masked, t_out = prepare(decoded, GOES_RECIPES, t, [dqf_float(d, f) for d, f in dqf], gap)
    assert 0 < n_masked.sum() < want[0].size and (shape[0] < 3 or len(t_out) == shape[0] + 1)
    return dict(shape=shape, raws=raws, decoded=decoded, dqf=dqf, t=t, time_gap=gap, want=want, n_masked=n_masked, t_out=t_out)


@functools.lru_cache(maxsize=None)
def seviri_nat_case(shape, seed=1):
    """five float32 brightness temperatures with NaN and infinities; IR_087 - IR_120 has both signs, -inf among them (which
    the clamp lifts to 0: finite)"""
    rng = np.random.default_rng([seed, *shape])
    chans = [(200 + 100 * rng.random(shape)).astype(np.float32) for _ in range(5)]
    for c, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf)):
        chans[c][rng.random(shape) < 0.003] = bad
    t = times(shape[0])
    gap = timedelta(minutes=30)
    want, n_masked, t_out = prepare(chans, SEVIRI_NAT_RECIPES, t, time_gap=gap)
    assert (want[2] == 0).any() and (want[2] > 0).any() and len(t_out) == shape[0]
    return dict(shape=shape, chans=chans, t=t, time_gap=gap, want=want, n_masked=n_masked, t_out=t_out)
