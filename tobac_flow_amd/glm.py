"""GLM flashes onto the ABI grid on the GPU: the array-level form of tobac_flow/glm.py:77-145 (regrid_glm with
get_uncorrected_glm_hist / get_corrected_glm_hist).  The reference opens every flash file inside the window of every
frame and calls np.histogram2d once per frame; here the flashes of all files are binned onto the whole (T, H, W) stack by
one launch of tf_bin_points (tobac_flow_amd.binning).  Reading the files stays with the caller.  The projection to ABI
coordinates is tobac_flow_amd.abi.get_abi_x_y (tf_geos_forward: device tensors in, device tensors out), whose x and y go
in here as they are.  The GLM parallax correction (get_glm_parallax_offsets and the lmatools coordinate systems behind it)
is not taken: for the "corrected" grid the caller hands in corrected coordinates.

The counts equal the reference's bit for bit.  The result feeds tobac_flow_amd.validation (`glm_grid`)."""
from datetime import datetime, timedelta

import numpy as np

from tobac_flow_amd.binning import _is_tensor, _lib, bin_points, time_ticks

_EPOCH = datetime(1970, 1, 1)


def _ticks_of(dt):
    return (dt - _EPOCH) // timedelta(microseconds=1)


def glm_windows(goes_dates, max_time_diff=15):
    """The window of every frame as glm.py:111-130 builds it: half the gap to the neighbouring frame on either side,
    gaps of `max_time_diff` minutes or more counted as max_time_diff, the first and the last gap used twice.  Returns
    (start, end), int64 microseconds; the reference takes a file with start < t < end."""
    ticks = time_ticks(goes_dates)
    if _is_tensor(ticks):
        ticks = ticks.cpu().numpy()
    if ticks.ndim != 1 or ticks.size < 2:
        raise ValueError("goes_dates must hold at least 2 frames")
    dates = [_EPOCH + timedelta(microseconds=int(v)) for v in ticks]
    max_diff = max_time_diff * 60
    gaps = [(b - a).total_seconds() for a, b in zip(dates[:-1], dates[1:])]
    half = [g / 2 if g < max_diff else max_diff / 2 for g in gaps]
    half = [half[0]] + half + [half[-1]]
    start = np.array([_ticks_of(d - timedelta(seconds=h)) for d, h in zip(dates, half[:-1])], dtype=np.int64)
    end = np.array([_ticks_of(d + timedelta(seconds=h)) for d, h in zip(dates, half[1:])], dtype=np.int64)
    return start, end


def regrid_glm(flash_x, flash_y, flash_file, file_times, goes_dates, x_bins, y_bins, max_time_diff=15):
    """The (T, H, W) flash counts of glm.py:107-145.  flash_x, flash_y: projected coordinates of all flashes (float32 or
    float64); flash_file: for every flash the index of its file in `file_times`; file_times: the files' times (the keys of
    the reference's `glm_files`); goes_dates: the T frame times, increasing; x_bins, y_bins: the bin edges of the grid
    (utils.get_coord_bin_edges of the ABI coordinates: y_bins decreases, it is binned on y_bins[::-1] and flipped back).
    A frame takes the files with start < t < end of glm_windows.  A frame with no FILE in its window stays -1 (the
    reference's missing value), a frame with files but no flash is 0.  int64 on the host like the reference, int32 on the
    device.  One launch for the whole stack; identical in every run."""
    start, end = glm_windows(goes_dates, max_time_diff)
    win_start, win_end = start + 1, end                           # lower-open: start < t  <=>  start + 1 <= t
    if (np.diff(win_start) < 0).any() or (np.diff(win_end) < 0).any():
        raise ValueError("goes_dates must increase")
    files = time_ticks(file_times)
    if _is_tensor(files):
        files = files.cpu().numpy()
    if files.ndim != 1:
        raise ValueError("file_times must be one-dimensional")
    has_file = np.array([bool(((files > s) & (files < e)).any()) for s, e in zip(start, end)])
    device = any(_is_tensor(a) for a in (flash_x, flash_y, flash_file))
    n_flash = int(flash_file.shape[0]) if hasattr(flash_file, "shape") else len(flash_file)
    if n_flash and (int(flash_file.min()) < 0 or int(flash_file.max()) >= files.size):
        raise ValueError("flash_file holds an index outside file_times")
    lib = _lib()
    t = lib.torch()
    if n_flash:
        time = lib.to_dev(files)[lib.to_dev(flash_file).to(t.int64)]
    else:
        time = t.zeros(0, dtype=t.int64, device=lib.device())
    y_rev = y_bins.flip(0) if _is_tensor(y_bins) else np.ascontiguousarray(np.asarray(y_bins, dtype=np.float64)[::-1])
    grid = bin_points([flash_y, flash_x], [y_rev, x_bins], time=time, win_start=win_start, win_end=win_end, flip=(0,),
                      outputs=("count",))["count"]
    if not has_file.all():
        grid[lib.to_dev((~has_file).astype(np.uint8)).to(t.bool)] = -1
    return grid if device else lib.to_host(grid).astype(np.int64)
