"""NEXRAD gates onto the ABI grid on the GPU: the array-level form of tobac_flow/nexrad.py:80-231 (get_nexrad_hist,
get_site_grids, regrid_nexrad).  Per site and per frame the reference re-masks all gates of the site and makes two
np.histogram2d calls and one scipy.stats.binned_statistic_dd; here one launch of tf_bin_points (tobac_flow_amd.binning)
bins the gates of a site onto the whole (T, H, W) stack and gives the raw counts, the counts of valid gates and the sum of
their reflectivity at once.  Reading the archives (pyart) stays with the caller.  The projection of the gates with its
parallax correction is map_nexrad_to_goes below (tf_geos_forward with the altitudes: one launch, device tensors in,
device tensors out), whose x and y go into the functions here as they are.  get_3d_nexrad_hist is not taken: nothing in
the reference calls it.

Counts equal the reference's bit for bit.  The mean is sum / count in double of a sum that differs from SciPy's by the
summation order only, and may differ in the last bits from run to run.  The counts follow np.histogram2d's
last-edge rule and the mean SciPy's: one launch under SciPy's rule serves both unless its status word reports a gate on
which the two rules disagree (a gate within 10^-d of the last edge) or the gates are float32 (SciPy then bins on edges
rounded to float32, NumPy on the edges as given), and only then the counts are binned again.  A
non-finite x or y of a gate inside the time window and the altitude range is a ValueError."""
import numpy as np

from tobac_flow_amd.binning import _is_tensor, _lib, _np_dtype, bin_points, time_ticks


def _one_tick(x):
    return int(np.asarray(time_ticks(np.asarray([x]))).reshape(-1)[0])


def _site_stack(time, alt, x, y, ref, ref_valid, x_bins, y_bins, win_start, win_end, min_alt, max_alt):
    """(counts_raw, counts_masked, ref_mean) of one site for the frames [win_start[f], win_end[f]): float64 device tensors"""
    lib = _lib()
    t = lib.torch()
    ticks = lib.to_dev(time_ticks(time))
    alt = lib.to_dev(alt)
    keep = (alt > min_alt) & (alt < max_alt)
    valid = lib.to_dev(ref_valid)
    valid = valid if valid.dtype == t.bool else valid != 0
    y_rev = y_bins.flip(0) if _is_tensor(y_bins) else np.ascontiguousarray(np.asarray(y_bins, dtype=np.float64)[::-1])
    common = dict(keep=keep, keep_value=valid, time=ticks, win_start=win_start, win_end=win_end, flip=(0,))
    got = bin_points([y, x], [y_rev, x_bins], rule="scipy", values=ref, outputs=("count", "count_v", "sum_wv"), **common)
    n_valid = got["count_v"].to(t.float64)
    mean = t.where(n_valid > 0, got["sum_wv"] / n_valid, t.full_like(n_valid, float("nan")))
    counts = got
    # np.histogram2d decides otherwise about some gate, or (float32 gates) SciPy has binned on float32-rounded edges
    if got["status"] & lib.BIN_STATUS_RULES_DIFFER or _np_dtype(x) == np.dtype(np.float32):
        counts = bin_points([y, x], [y_rev, x_bins], rule="numpy", outputs=("count", "count_v"), **common)
    # nexrad.py:108-117: zeros instead of SciPy's mean where the frame has no valid gate at all, inside the grid or not
    empty = (got["count_v"].flatten(1).amax(1) == 0).nonzero().flatten().tolist()
    ws, we = np.asarray(win_start), np.asarray(win_end)
    for f in empty:
        if not bool((keep & valid & (ticks >= int(ws[f])) & (ticks < int(we[f]))).any()):
            mean[f] = 0
    return counts["count"].to(t.float64), counts["count_v"].to(t.float64), mean


def _give(stacks, device, squeeze=False):
    lib = _lib()
    stacks = [s[0] if squeeze else s for s in stacks]
    return list(stacks) if device else [lib.to_host(s.contiguous()) for s in stacks]


def map_nexrad_to_goes(nexrad_lat, nexrad_lon, nexrad_alt, goes_ds):
    """nexrad.py:60-77: the scan angles `(x, y)` at which the ABI sees gates at (lat, lon) degrees and `alt` metres up --
    project, shift latitude and longitude by degrees(alt tan(...) / 6.371e6), project again.  goes_ds: what
    tobac_flow_amd.abi reads (`.goes_imager_projection`).  NumPy arrays in: NumPy out; device tensors in: one launch of
    tf_geos_forward, device tensors out.  Gates beyond the limb give +inf (NaN where the shifted position is undefined)."""
    from tobac_flow_amd.abi import get_abi_proj
    if not _is_tensor(nexrad_lat) and not _is_tensor(nexrad_lon) and np.size(nexrad_lat) == np.size(nexrad_lon) == 0:
        return np.array([]), np.array([])
    return get_abi_proj(goes_ds).forward_points(nexrad_lat, nexrad_lon, nexrad_alt)


def get_nexrad_hist(time, alt, x, y, ref, ref_valid, x_bins, y_bins, start_time, end_time, min_alt=2500, max_alt=15000):
    """nexrad.py:80-119 for one frame: `(counts_raw, counts_masked, ref_mean)`, float64 (H, W).  time, alt, x, y, ref,
    ref_valid: one entry per gate of the site -- time as datetime64 / datetimes / int64 microseconds, x and y the projected
    coordinates (float32 or float64, both the same), ref the reflectivity (float32 or float64), ref_valid what the
    reference computes as `isfinite(ref) & ~ref.mask`.  Gates with start_time <= time < end_time and min_alt < alt <
    max_alt count; y is binned on y_bins[::-1] and flipped back.  ref_mean is NaN over a bin without a valid gate, and all
    zeros when no gate of the frame is valid."""
    ws, we = np.array([_one_tick(start_time)], dtype=np.int64), np.array([_one_tick(end_time)], dtype=np.int64)
    device = any(_is_tensor(a) for a in (time, alt, x, y, ref, ref_valid))
    return tuple(_give(_site_stack(time, alt, x, y, ref, ref_valid, x_bins, y_bins, ws, we, min_alt, max_alt), device, True))


def _frame_windows(goes_dates, half_window):
    dates = time_ticks(goes_dates)
    dates = dates.cpu().numpy() if _is_tensor(dates) else dates
    half = getattr(half_window, "total_seconds", lambda: half_window)()
    half = int(round(half * 1e6))
    if dates.ndim != 1 or dates.size < 1 or (np.diff(dates) < 0).any():
        raise ValueError("goes_dates must be a non-empty, non-decreasing sequence of times")
    return dates - half, dates + half


def get_site_grids(time, alt, x, y, ref, ref_valid, x_bins, y_bins, goes_dates, half_window=150, min_alt=2500,
                   max_alt=15000):
    """nexrad.py:179-191: get_nexrad_hist for the window [t - half_window, t + half_window) of every frame time in
    goes_dates (half_window in seconds or a timedelta; the reference's 2.5 minutes), all frames in ONE launch:
    `[counts_raw, counts_masked, ref_mean]`, each float64 (T, H, W).  Windows of close frames overlap: a gate then counts
    in each of them."""
    ws, we = _frame_windows(goes_dates, half_window)
    device = any(_is_tensor(a) for a in (time, alt, x, y, ref, ref_valid))
    return _give(_site_stack(time, alt, x, y, ref, ref_valid, x_bins, y_bins, ws, we, min_alt, max_alt), device)


def regrid_nexrad(sites, x_bins, y_bins, goes_dates, half_window=150, min_alt=2500, max_alt=15000):
    """nexrad.py:194-231: the mean reflectivity of all sites on the (T, H, W) grid and the mask of cells that no gate
    reached -- `(ref_grid, ref_mask)`, float64 and bool.  sites: an iterable of `(time, alt, x, y, ref, ref_valid)` per
    site (get_nexrad_hist).  Per site mean * count is added where it is finite, as the reference does; the total is
    divided by the number of valid gates, set to NaN where no raw gate fell and to -33 where gates fell but none was
    valid."""
    ws, we = _frame_windows(goes_dates, half_window)
    lib = _lib()
    t = lib.torch()
    total = raw_total = valid_total = None
    device = False
    for site in sites:
        device = device or any(_is_tensor(a) for a in site)
        raw, count, mean = _site_stack(*site, x_bins, y_bins, ws, we, min_alt, max_alt)
        if total is None:
            total, raw_total, valid_total = t.zeros_like(mean), t.zeros_like(raw), t.zeros_like(count)
        product = mean * count
        total += t.where(t.isfinite(product), product, t.zeros_like(product))
        raw_total += raw
        valid_total += count
    if total is None:
        raise ValueError("no site")
    grid = total / valid_total
    mask = raw_total == 0
    grid[mask] = float("nan")
    grid[~mask & t.isnan(grid)] = -33
    if device:
        return grid, mask
    return lib.to_host(grid), lib.to_host(mask.to(t.uint8)).astype(bool)
