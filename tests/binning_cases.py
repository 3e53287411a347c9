"""Cases and yardsticks of the point binning (tobac_flow_amd.binning / glm / nexrad, tf_bin_points): `restate()` is the
operator in NumPy -- np.searchsorted per axis with either library's last-edge rule, then the libraries' own sequential
np.bincount -- `bound()` the per-bin tolerance of a sum, and the recipe cases come with two host forms each: one call of
restate() over all frames, and the plain per-frame loop of np.histogram2d / scipy.stats.binned_statistic_dd calls in the
argument patterns of tobac_flow/glm.py:77-145, tobac_flow/nexrad.py:80-231 and scripts/grid_flux.py:65-73.

The tolerance.  A sum of n terms evaluated in ANY order lies within (n - 1) 2^-53 sum|term| of the exact sum (first-order
bound of recursive summation, every partial sum being bounded by sum|term|); the libraries' bincount is one such order
and the device's atomics another, so the two differ by at most bound() = 2 (n - 1) 2^-53 sum|term|, computed from the
inputs.  n <= 1 gives 0: bit equality.  A quotient a / b of two such sums with bounds A and B differs from the library's
by at most (A + |q| B) / (|b| - B) plus one rounding of each division, 2 * 2^-53 |q|: quotient_bound()."""
import os
from datetime import datetime, timedelta

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binning_ref.npz")
U = 2.0 ** -53
STATUS_COORD, STATUS_VALUE, STATUS_RULES_DIFFER = 1, 2, 4
EPOCH = datetime(1970, 1, 1)


def bound(n_terms, abs_sum):
    with np.errstate(invalid="ignore"):                           # 0 * inf where a one-term bin holds an infinite value
        return 2.0 * np.maximum(np.asarray(n_terms, dtype=np.float64) - 1, 0) * U * np.asarray(abs_sum, dtype=np.float64)


def quotient_bound(num, den, num_bound, den_bound):
    with np.errstate(all="ignore"):
        q = np.abs(num / den)
        return (num_bound + q * den_bound) / (np.abs(den) - den_bound) + 2 * U * q


def decimals_of(edges):
    return int(-np.log10(np.diff(np.asarray(edges)).min())) + 6


def scipy_edges(e, dtype):
    """the edges as SciPy uses them: cast to the sample's dtype ("preserve sample floating point precision in bin edges")"""
    return np.asarray(e, dtype=np.float64).astype(dtype)


def axis_bins(v, e, rule):
    """bin of every coordinate on one axis, -1 where the axis drops the point.  NumPy's rule compares in double
    (np.searchsorted widens float32 exactly); SciPy's works on scipy_edges(), which the caller passes, in v's dtype"""
    v, e = np.asarray(v), np.asarray(e)
    k = np.searchsorted(e.astype(np.float64), v.astype(np.float64), side="right") - 1
    if rule == "numpy":
        on_edge = v == e[-1]
    else:
        d = int(-np.log10(np.diff(e).min())) + 6
        last = e[-1].astype(v.dtype)
        on_edge = (v >= last) & (np.around(v, d) == np.around(last, d))
    k = k - on_edge
    return np.where((k >= 0) & (k < e.size - 1), k, -1)


def restate(coords, edges, rule="numpy", values=None, weights=None, keep=None, keep_value=None, finite_value=False,
            time=None, win_start=None, win_end=None, flip=(), outputs=("count", "count_v", "sum_w", "sum_wv")):
    """tf_bin_points in NumPy: {"count", "count_v" (int64), "sum_w", "sum_wv" (float64, the sequential bincount),
    "abs_w", "abs_wv" (sum |term| per bin, for bound()), "status"}, every grid shaped (T, n_0[, n_1[, n_2]])"""
    coords = [np.asarray(c) for c in coords]
    scipy = rule == "scipy"
    edges = [scipy_edges(e, coords[0].dtype) if scipy else np.asarray(e, dtype=np.float64) for e in edges]
    n = coords[0].size
    nb = [e.size - 1 for e in edges]
    n_bins = int(np.prod(nb))
    ks = [axis_bins(c, e, rule) for c, e in zip(coords, edges)]
    inside = np.all([k >= 0 for k in ks], axis=0) if n else np.zeros(0, bool)
    differ = np.zeros(n, bool)
    if scipy:
        for c, e, k in zip(coords, edges, ks):
            differ |= (k >= 0) != (axis_bins(c, e, "numpy") >= 0)
    flat = np.zeros(n, np.int64)
    for d, k in enumerate(ks):
        kk = np.where(k < 0, 0, k)
        flat = flat * nb[d] + (nb[d] - 1 - kk if d in flip else kk)
    finite = np.all([np.isfinite(c) for c in coords], axis=0) if n else np.zeros(0, bool)
    kp = np.ones(n, bool) if keep is None else np.asarray(keep).astype(bool)
    kv = np.ones(n, bool) if keep_value is None else np.asarray(keep_value).astype(bool)
    wd = np.ones(n) if weights is None else np.asarray(weights).astype(np.float64)
    if values is not None:
        values = np.asarray(values)
        term = (values if weights is None else values * np.asarray(weights)).astype(np.float64)   # NumPy's result type
        v_finite = np.isfinite(values)
    else:
        term, v_finite = np.zeros(n), np.ones(n, bool)
    if time is None:
        T, f0, f1 = 1, np.zeros(n, np.int64), np.ones(n, np.int64)
    else:
        T = len(win_start)
        f0 = np.searchsorted(np.asarray(win_end), np.asarray(time), side="right")
        f1 = np.searchsorted(np.asarray(win_start), np.asarray(time), side="right")
    want_value = any(o in outputs for o in ("count_v", "sum_w", "sum_wv"))
    res = {k: np.zeros((T, n_bins), np.int64 if k.startswith("count") else np.float64)
           for k in ("count", "count_v", "sum_w", "sum_wv", "abs_w", "abs_wv")}
    status = 0
    for f in range(T):
        sel = kp & (f0 <= f) & (f < f1)
        with_value = sel & kv & want_value
        bad = with_value & ~v_finite
        if finite_value:
            with_value &= v_finite
        elif scipy and bad.any():
            status |= STATUS_VALUE
            sel, with_value = sel & ~bad, with_value & ~bad
        if "count" not in outputs:
            sel = with_value
        if scipy:
            bad = sel & ~finite
            if bad.any():
                status |= STATUS_COORD
                sel, with_value = sel & ~bad, with_value & ~bad
            if (sel & differ).any():
                status |= STATUS_RULES_DIFFER
        sel, with_value = sel & inside, with_value & inside
        res["count"][f] = np.bincount(flat[sel], minlength=n_bins)
        res["count_v"][f] = np.bincount(flat[with_value], minlength=n_bins)
        for name, x in (("sum_w", wd), ("sum_wv", term)):
            res[name][f] = np.bincount(flat[with_value], weights=x[with_value], minlength=n_bins)
            res["abs_" + name[4:]][f] = np.bincount(flat[with_value], weights=np.abs(x[with_value]), minlength=n_bins)
    res = {k: v.reshape([T] + nb) for k, v in res.items()}
    res["status"] = status
    return res


# ---- axes and points -------------------------------------------------------------------------------------------------------
def coord_bin_edges(coord):
    c = np.asarray(coord).astype(np.float64)
    return np.concatenate([c[:1], (c[:-1] + c[1:]) / 2, c[-1:]])


def abi_x(n=67):
    """an ABI-like float32 scan-angle axis: its midpoints are not equidistant in double"""
    return (np.float32(-0.101332) + np.float32(5.6e-05) * np.arange(n, dtype=np.float32)).astype(np.float32)


def abi_y(n=33):
    return (np.float32(0.128212) - np.float32(5.6e-05) * np.arange(n, dtype=np.float32)).astype(np.float32)


def edge_points(edges, dtype, specials=True):
    """every edge, its neighbours in `dtype` on either side, the last edge again, just beyond both ends, +-inf and NaN"""
    e = np.asarray(edges, dtype=np.float64).astype(dtype)
    inf = dtype(np.inf)
    pts = [e, np.nextafter(e, inf), np.nextafter(e, -inf), e[-1:], np.nextafter(e[-1:], inf), np.nextafter(e[:1], -inf)]
    if specials:
        pts.append(np.array([np.inf, -np.inf, np.nan], dtype=dtype))
    return np.concatenate(pts).astype(dtype)


ZERO_WIDTH_EDGES = np.array([0.0, 1.0, 1.0, 2.0])
ZERO_WIDTH_POINTS = np.array([0.5, 1.0, 2.0])
SCIPY_WIDTHS = {1.0: 6, 0.003: 8, 250.0: 4}                       # smallest edge width -> SciPy's decimals


def scipy_rounding_case(width):
    """edges of smallest width `width` and points at last + 10^(-d-3), last + 10^(-d+1), nextafter(last) and last itself"""
    d = SCIPY_WIDTHS[width]
    edges = np.array([0.0, width, 3 * width, 4 * width + width])
    assert decimals_of(edges) == d
    last = edges[-1]
    return edges, np.array([last + 10.0 ** (-d - 3), last + 10.0 ** (-d + 1), np.nextafter(last, np.inf), last, last / 2])


def scattered(n, nd, seed, dtype=np.float64, edges=None):
    """n points around nd axes (ABI-like edges unless given); values and weights of both types, masks and times"""
    rng = np.random.default_rng(seed)
    if edges is None:
        edges = [coord_bin_edges(abi_y()[::-1]), coord_bin_edges(abi_x()), np.array([2500.0, 5000.0, 5000.5, 9000.0, 15000.0])][:nd]
    coords = []
    for e in edges:
        span = e[-1] - e[0]
        coords.append((e[0] - 0.05 * span + 1.1 * span * rng.random(n)).astype(dtype))
    v32 = (rng.integers(-1000, 1000, n) / 7).astype(np.float32)
    w32 = (rng.integers(1, 1000, n) / 3).astype(np.float32)
    return {"coords": coords, "edges": edges, "v32": v32, "v64": v32.astype(np.float64) * 1.0000001, "w32": w32,
            "w64": w32.astype(np.float64) * 0.9999999, "keep": rng.random(n) < 0.8, "keep_value": rng.random(n) < 0.7,
            "time": rng.integers(-2, 62, n).astype(np.int64)}


# overlapping (0, 1), abutting (1, 2), empty (3: start == end), a gap before 4; times exactly at starts and ends occur
WIN_START = np.array([0, 10, 20, 30, 50], dtype=np.int64)
WIN_END = np.array([12, 20, 30, 30, 60], dtype=np.int64)


def run_patterns(n_bins=67):
    """bin indices (as coordinates k + 0.5 on edges 0 .. n_bins) whose runs cross the 4-point vector, the 16-point lane
    chunk, the 256-point step and the 1024-point wave span; and one pattern with no run at all"""
    i = np.arange(3 * 4096 + 77)
    pats = {f"runs_{r}": (i // r) % n_bins for r in (3, 4, 5, 16, 17, 255, 256, 1000, 1024, 1025)}
    pats["alternating"] = i % 2 * (n_bins - 1)
    pats["no_run"] = (i * 29) % n_bins
    return {k: v.astype(np.float64) + 0.5 for k, v in pats.items()}, np.arange(n_bins + 1, dtype=np.float64)


# ---- the recipes -----------------------------------------------------------------------------------------------------------
def ticks(dt):
    return (dt - EPOCH) // timedelta(microseconds=1)


def glm_case():
    """5 frames of 33 x 67: frame 1 has no file in its window, frame 3 has a file without a flash, the gap between frames
    3 and 4 exceeds max_time_diff = 15 minutes; files exactly at a window's start and end (both excluded)"""
    rng = np.random.default_rng(11)
    t0 = datetime(2018, 6, 19, 17, 0, 20)
    goes_dates = [t0 + timedelta(minutes=m) for m in (0, 5, 10, 15, 45)]
    # windows (start, end): (-2.5, 2.5) (2.5, 7.5) (7.5, 12.5) (12.5, 22.5) (37.5, 52.5) minutes after t0
    file_minutes = [-2.5, -2.0, 0.3, 2.4, 2.5, 7.5, 8.0, 9.9, 12.0, 13.0, 22.5, 30.0, 37.6, 44.0, 52.4, 52.5, 60.0]
    file_times = [t0 + timedelta(minutes=m) for m in file_minutes]
    n_files = len(file_times)
    empty_file = file_minutes.index(13.0)                         # the only file of frame 3: no flash
    flash_file = rng.integers(0, n_files, 400)
    flash_file = flash_file[flash_file != empty_file]
    n = flash_file.size
    x, y = abi_x(), abi_y()
    x_bins, y_bins = coord_bin_edges(x), coord_bin_edges(y)
    fx = x_bins[0] - 2e-4 + (x_bins[-1] - x_bins[0] + 4e-4) * rng.random(n)
    fy = y_bins[-1] - 2e-4 + (y_bins[0] - y_bins[-1] + 4e-4) * rng.random(n)
    fx[:8] = [x_bins[0], x_bins[-1], x_bins[5], x_bins[66], np.nextafter(x_bins[-1], 1), x_bins[1], x_bins[33], x_bins[0]]
    fy[:8] = [y_bins[0], y_bins[-1], y_bins[5], y_bins[32], y_bins[-1], np.nextafter(y_bins[0], 1), y_bins[16], y_bins[-1]]
    return {"flash_x": fx, "flash_y": fy, "flash_file": flash_file.astype(np.int64),
            "file_times": np.array([ticks(t) for t in file_times], dtype=np.int64),
            "goes_dates": np.array([ticks(t) for t in goes_dates], dtype=np.int64), "x_bins": x_bins, "y_bins": y_bins}


def glm_windows_plain(goes_ticks, max_time_diff=15):
    dates = [EPOCH + timedelta(microseconds=int(t)) for t in goes_ticks]
    max_diff = max_time_diff * 60
    diffs = [(dates[i + 1] - dates[i]).total_seconds() for i in range(len(dates) - 1)]
    diffs = [td / 2 if td < max_diff else max_diff / 2 for td in diffs]
    diffs = [diffs[0]] + diffs + [diffs[-1]]
    return ([dates[i] - timedelta(seconds=diffs[i]) for i in range(len(dates))],
            [dates[i] + timedelta(seconds=diffs[i + 1]) for i in range(len(dates))])


def glm_loop(c, max_time_diff=15):
    """the plain per-frame loop: np.histogram2d over the flashes of the files inside each frame's open window"""
    starts, ends = glm_windows_plain(c["goes_dates"], max_time_diff)
    files = [EPOCH + timedelta(microseconds=int(t)) for t in c["file_times"]]
    grid = np.full((len(starts), c["y_bins"].size - 1, c["x_bins"].size - 1), -1)
    for i, (start, end) in enumerate(zip(starts, ends)):
        inside = [k for k, t in enumerate(files) if t > start and t < end]
        if not inside:
            continue
        sel = np.isin(c["flash_file"], inside)
        grid[i] = np.histogram2d(c["flash_y"][sel], c["flash_x"][sel], bins=(c["y_bins"][::-1], c["x_bins"]))[0][::-1]
    return grid


def glm_host(c, max_time_diff=15):
    """the same stack from ONE call of restate() with the windows as lower-open integer ranges"""
    starts, ends = glm_windows_plain(c["goes_dates"], max_time_diff)
    ws = np.array([ticks(s) + 1 for s in starts], dtype=np.int64)
    we = np.array([ticks(e) for e in ends], dtype=np.int64)
    got = restate([c["flash_y"], c["flash_x"]], [c["y_bins"][::-1], c["x_bins"]], time=c["file_times"][c["flash_file"]],
                  win_start=ws, win_end=we, flip=(0,))["count"]
    has_file = np.array([((c["file_times"] >= s) & (c["file_times"] < e)).any() for s, e in zip(ws, we)])
    got[~has_file] = -1
    return got


HALF_WINDOW = 150


def nexrad_case():
    """2 sites, 4 frames (two of them 4 minutes apart: overlapping windows) of 33 x 67.  Bin (5, 7) receives invalid gates
    only (-> -33 in regrid_nexrad), most bins nothing (-> NaN); frame 3 of site 1 has no valid gate at all (zeros) and
    gates exactly at the window's start (counted) and end (not), at min_alt and max_alt (not counted)"""
    t0 = datetime(2018, 6, 19, 18, 0, 0)
    goes_dates = np.array([ticks(t0 + timedelta(minutes=m)) for m in (0, 5, 9, 20)], dtype=np.int64)
    x, y = abi_x(), abi_y()
    x_bins, y_bins = coord_bin_edges(x), coord_bin_edges(y)
    sites = []
    for s in range(2):
        rng = np.random.default_rng(21 + s)
        n = 500
        cx, cy = x[20 + 25 * s], y[10 + 12 * s]
        gx = cx + 6e-4 * rng.standard_normal(n)
        gy = cy + 4e-4 * rng.standard_normal(n)
        alt = rng.uniform(1000, 17000, n)
        time = goes_dates[0] + rng.integers(-200, 1400, n).astype(np.int64) * 1_000_000
        ref = rng.uniform(-20, 60, n).astype(np.float32)
        ref[rng.random(n) < 0.2] = np.nan
        masked = rng.random(n) < 0.1
        # invalid gates only in bin (5, 7) of the flipped grid, in frame 0
        gx[:6], gy[:6], alt[:6], time[:6] = x[7], y[5], 5000, goes_dates[0]
        ref[:6] = np.nan
        far = (np.abs(gx - x[7]) < 4e-5) & (np.abs(gy - y[5]) < 4e-5)
        ref[far] = np.nan
        alt[6:10] = [2500, 15000, 2500.5, 14999.5]
        time[10:14] = [goes_dates[1] - 150_000_000, goes_dates[1] + 150_000_000, goes_dates[1] + 149_999_999, goes_dates[1] - 150_000_001]
        alt[10:14] = 6000
        if s == 1:
            in_3 = (time >= goes_dates[3] - 150_000_000) & (time < goes_dates[3] + 150_000_000)
            masked[in_3] = True
        sites.append({"time": time, "alt": alt, "x": gx, "y": gy, "ref": ref, "ref_valid": np.isfinite(ref) & ~masked})
    return {"sites": sites, "goes_dates": goes_dates, "x_bins": x_bins, "y_bins": y_bins}


def nexrad_hist_loop(site, x_bins, y_bins, start, end, min_alt=2500, max_alt=15000):
    """one frame with the libraries' calls in the reference's argument pattern"""
    from scipy import stats
    wh_t = (site["time"] >= start) & (site["time"] < end)
    mask = (site["alt"][wh_t] > min_alt) & (site["alt"][wh_t] < max_alt)
    x, y = site["x"][wh_t][mask], site["y"][wh_t][mask]
    ref, ref_mask = site["ref"][wh_t][mask], site["ref_valid"][wh_t][mask]
    raw = np.histogram2d(y, x, bins=(y_bins[::-1], x_bins))[0][::-1]
    masked = np.histogram2d(y[ref_mask], x[ref_mask], bins=(y_bins[::-1], x_bins))[0][::-1]
    if np.any(ref_mask):
        mean = stats.binned_statistic_dd((y[ref_mask], x[ref_mask]), ref[ref_mask], statistic="mean",
                                         bins=(y_bins[::-1], x_bins), expand_binnumbers=True)[0][::-1]
    else:
        mean = np.zeros(masked.shape)
    return raw, masked, mean


def nexrad_site_loop(site, c):
    half = HALF_WINDOW * 1_000_000
    frames = [nexrad_hist_loop(site, c["x_bins"], c["y_bins"], t - half, t + half) for t in c["goes_dates"]]
    return [np.stack(f) for f in zip(*frames)]


def nexrad_site_host(site, c):
    """(raw, masked, mean, bound of the mean) of one site from restate(): counts under NumPy's rule, the mean under SciPy's"""
    half = HALF_WINDOW * 1_000_000
    ws, we = c["goes_dates"] - half, c["goes_dates"] + half
    keep = (site["alt"] > 2500) & (site["alt"] < 15000)
    args = dict(values=site["ref"], keep=keep, keep_value=site["ref_valid"], time=site["time"], win_start=ws, win_end=we, flip=(0,))
    a = restate([site["y"], site["x"]], [c["y_bins"][::-1], c["x_bins"]], rule="numpy", **args)
    b = restate([site["y"], site["x"]], [c["y_bins"][::-1], c["x_bins"]], rule="scipy", **args)
    with np.errstate(all="ignore"):
        mean = np.where(b["count_v"] > 0, b["sum_wv"] / b["count_v"], np.nan)
        tol = np.where(b["count_v"] > 0, quotient_bound(b["sum_wv"], b["count_v"].astype(np.float64), bound(b["count_v"], b["abs_wv"]), 0.0), 0.0)
    for f in range(len(ws)):
        if not (keep & site["ref_valid"] & (site["time"] >= ws[f]) & (site["time"] < we[f])).any():
            mean[f] = 0
    return a["count"].astype(np.float64), a["count_v"].astype(np.float64), mean, tol


def nexrad_regrid(stacks):
    """nexrad.py:200-223 over the per-site (raw, masked, mean) stacks"""
    total, raw_total, valid_total = (np.zeros(stacks[0][0].shape) for _ in range(3))
    for raw, count, mean in stacks:
        with np.errstate(all="ignore"):
            wh = np.isfinite(mean * count)
        total[wh] += mean[wh] * count[wh]
        raw_total += raw
        valid_total += count
    with np.errstate(all="ignore"):
        grid = total / valid_total
    mask = raw_total == 0
    grid[mask] = np.nan
    grid[np.logical_and(~mask, np.isnan(grid))] = -33
    return grid, mask


def flux_case():
    """a 40 x 60 swath of float32 latitude, longitude, flux (with NaN and inf pixels) and pixel area onto a 2-degree grid"""
    rng = np.random.default_rng(31)
    i, j = np.meshgrid(np.arange(40, dtype=np.float32), np.arange(60, dtype=np.float32), indexing="ij")
    lat = (np.float32(-21.3) + np.float32(1.07) * i + np.float32(0.013) * j).astype(np.float32)
    lon = (np.float32(-30.7) + np.float32(1.04) * j - np.float32(0.021) * i).astype(np.float32)
    data = rng.uniform(-50, 400, lat.shape).astype(np.float32)
    data[rng.random(lat.shape) < 0.1] = np.nan
    data[3, 4] = np.inf
    area = rng.uniform(9, 25, lat.shape).astype(np.float32)
    lat[0, 0], lon[0, 0] = 20.0, 30.0                             # on both last edges
    return {"lat": lat, "lon": lon, "data": data, "area": area, "area64": area.astype(np.float64),
            "lat_bins": np.arange(-20.0, 20.1, 2.0), "lon_bins": np.arange(-30.0, 30.1, 2.0)}


def flux_loop(c, weights="area"):
    """scripts/grid_flux.py:65-73 with the libraries' calls"""
    from scipy.stats import binned_statistic_2d
    x, y, data, w = c["lat"], c["lon"], c["data"], c[weights]
    bins = (c["lat_bins"], c["lon_bins"])
    wh = np.isfinite(data)
    binned = binned_statistic_2d(x[wh], y[wh], data[wh] * w[wh], bins=bins, statistic="sum")[0]
    with np.errstate(all="ignore"):
        binned /= binned_statistic_2d(x[wh], y[wh], w[wh], bins=bins, statistic="sum")[0]
    return binned


def flux_host(c, weights="area"):
    """(weighted mean, its bound) from one restate() call"""
    r = restate([c["lat"].ravel(), c["lon"].ravel()], [c["lat_bins"], c["lon_bins"]], rule="scipy", values=c["data"].ravel(),
                weights=c[weights].ravel(), finite_value=True, outputs=("sum_w", "sum_wv"))
    with np.errstate(all="ignore"):
        mean = (r["sum_wv"] / r["sum_w"])[0]
        tol = quotient_bound(r["sum_wv"], r["sum_w"], bound(r["count_v"], r["abs_wv"]), bound(r["count_v"], r["abs_w"]))[0]
    return mean, np.where(r["count_v"][0] > 0, tol, 0.0)


_GOLDEN = None


def golden():
    """{name: array} of tests/golden/binning_ref.npz (written by tests/golden/make_binning_golden.py)"""
    global _GOLDEN
    if _GOLDEN is None:
        z = np.load(GOLDEN)
        _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN
