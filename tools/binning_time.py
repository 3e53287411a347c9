"""Time the point binning (tf_bin_points, tobac_flow_amd.binning) at the workload's own size on the GPU, next to the NumPy /
SciPy calls it replaces on this machine's CPU and to a traffic floor:

  glm      10^6 and 10^7 scattered points onto T x N^2 counts through T abutting time windows (regrid_glm's launch), the
           points in their random order and sorted by (frame, bin) beforehand -- with the time of torch.sort over N int64
           keys beside it, that is what a sort-then-sum form could gain at best and what its sort would cost;
  flux     a dense S^2 float32 swath (latitude, longitude, flux, pixel area) onto a 0.1 degree grid: weighted_binned_mean_2d;
  nexrad   2 * 10^6 gates onto T x N^2: raw count, valid count and reflectivity sum in one launch (get_site_grids's).

Per case: the entry point alone (HIP events, operands on the device, outputs allocated and zeroed beforehand: the launch
accumulates), the zero-fill of its outputs alone, and the floor = zero-fill + input bytes at the rate tf_copy16 reaches on
1 GiB; the public call end to end (wall, device-resident inputs); the libraries' calls on the CPU -- for the T-frame
cases ONE frame's calls on N / T points, since every frame costs the reference such a call.
Median of RUNS after WARM warm-ups.  Usage: python tools/binning_time.py [N] [T] [S] [output file]
(development aid; the figures are kept in profiles/point_binning.txt)"""
import ctypes
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch
from scipy import stats

from tobac_flow_amd import _lib, binning

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
S = int(sys.argv[3]) if len(sys.argv) > 3 else 3712
OUT = open(sys.argv[4], "w") if len(sys.argv) > 4 else None
WARM, RUNS = 1, 5


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def events(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(f, timer=events):
    for _ in range(WARM):
        f()
    return statistics.median(timer(f) for _ in range(RUNS))


def cpu(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def copy_rate():
    L = _lib.lib()
    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    ms = median(lambda: _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), n, _lib.stream_ptr()), "tf_copy16"))
    return n / (ms * 1e-3)                                        # bytes READ per second (as many are written beside)


def measure(name, coords, edges, n_inputs_bytes, rate, public=None, **kw):
    """entry point alone, zero-fill alone, floor; returns the outputs of the last launch"""
    L = _lib.lib()
    params, result, status, hold = binning.prepare(coords, edges, **kw)
    outs = [v for v in result.values()]
    launch = lambda: _lib.check(L.tf_bin_points(ctypes.byref(params), _lib.stream_ptr()), "tf_bin_points")   # noqa: E731
    kernel = median(launch)
    zero = median(lambda: [o.zero_() for o in outs])
    out_bytes = sum(o.numel() * o.element_size() for o in outs)
    floor = zero + n_inputs_bytes / rate * 1e3
    say(f"  {name}: tf_bin_points alone {kernel:.3f} ms; zero-fill of {out_bytes / 1e9:.2f} GB outputs {zero:.3f} ms; "
        f"floor (zero-fill + {n_inputs_bytes / 1e6:.0f} MB inputs at the copy rate) {floor:.3f} ms; "
        f"launch + zero-fill = {(kernel + zero) / floor:.2f} x floor")
    if public is not None:
        say(f"  {name}: public call end to end (allocates and zeroes its outputs) {median(public, wall):.3f} ms wall")
    del hold
    return kernel


def scattered(n, rng):
    edges = np.linspace(-0.151872, 0.151872, N + 1)
    y = rng.uniform(-0.16, 0.16, n)
    x = rng.uniform(-0.16, 0.16, n)
    t = rng.integers(0, T * 1000, n).astype(np.int64)
    return y, x, t, edges


def glm_case(n, rate):
    rng = np.random.default_rng(1)
    y, x, t, edges = scattered(n, rng)
    ws, we = np.arange(T, dtype=np.int64) * 1000, (np.arange(T, dtype=np.int64) + 1) * 1000
    say(f"glm: {n} scattered float64 points onto {T} x {N}^2 int32 counts, {T} abutting windows")
    dev = [_lib.to_dev(a) for a in (y, x, t)]
    public = lambda: binning.bin_points(dev[:2], [edges, edges], time=dev[2], win_start=ws, win_end=we, flip=(0,))   # noqa: E731
    measure("random order", dev[:2], [edges, edges], n * 24, rate, public, time=dev[2], win_start=ws, win_end=we, flip=(0,))
    key = (t // 1000) * N * N + np.clip(np.searchsorted(edges, y, "right") - 1, 0, N - 1) * N + np.clip(np.searchsorted(edges, x, "right") - 1, 0, N - 1)
    order = np.argsort(key, kind="stable")
    srt = [_lib.to_dev(np.ascontiguousarray(a[order])) for a in (y, x, t)]
    measure("sorted by (frame, bin) beforehand", srt[:2], [edges, edges], n * 24, rate, time=srt[2], win_start=ws, win_end=we, flip=(0,))
    keys = _lib.to_dev(key)
    say(f"  torch.sort of the {n} int64 keys alone: {median(lambda: torch.sort(keys)):.3f} ms")
    m = n // T
    ms = cpu(lambda: np.histogram2d(y[:m], x[:m], bins=(edges, edges)))
    say(f"  CPU: np.histogram2d of one frame's {m} points on {N + 1}-edge axes {ms:.0f} ms -> {T} frames {ms * T:.0f} ms")
    del dev, srt, keys
    torch.cuda.empty_cache()


def flux_case(rate):
    i, j = np.meshgrid(np.arange(S, dtype=np.float32), np.arange(S, dtype=np.float32), indexing="ij")
    lat = (np.float32(-81) + np.float32(162 / (S - 1)) * i + np.float32(0.003) * np.sin(j / 50, dtype=np.float32)).astype(np.float32)
    lon = (np.float32(-81) + np.float32(162 / (S - 1)) * j + np.float32(0.003) * np.sin(i / 50, dtype=np.float32)).astype(np.float32)
    rng = np.random.default_rng(2)
    data = rng.uniform(0, 400, lat.shape).astype(np.float32)
    data[rng.random(lat.shape) < 0.05] = np.nan
    area = rng.uniform(9, 25, lat.shape).astype(np.float32)
    bins = (np.arange(-82, 82.05, 0.1), np.arange(-82, 82.05, 0.1))
    say(f"flux: a dense {S}^2 float32 swath (lat, lon, flux with 5 % NaN, area) onto a {bins[0].size - 1}^2 grid of 0.1 degree")
    dev = [_lib.to_dev(a.ravel()) for a in (lat, lon, data, area)]
    public = lambda: binning.weighted_binned_mean_2d(*dev, bins=bins)   # noqa: E731
    measure("weighted mean", dev[:2], list(bins), lat.size * 16, rate, public, rule="scipy", values=dev[2], weights=dev[3],
            finite_value=True, outputs=("sum_w", "sum_wv"))

    # the same pixels ordered by bin: every lane's 16 points then share one bin, which is the most that merging runs
    # across the lanes of a wave (or sorting first) could reach on this case
    key = (np.searchsorted(bins[0], lat.ravel(), "right").astype(np.int64) * bins[1].size + np.searchsorted(bins[1], lon.ravel(), "right"))
    order = np.argsort(key, kind="stable")
    srt = [_lib.to_dev(np.ascontiguousarray(a.ravel()[order])) for a in (lat, lon, data, area)]
    measure("weighted mean, pixels ordered by bin beforehand", srt[:2], list(bins), lat.size * 16, rate, rule="scipy", values=srt[2],
            weights=srt[3], finite_value=True, outputs=("sum_w", "sum_wv"))
    del srt

    def reference():
        wh = np.isfinite(data)
        a = stats.binned_statistic_2d(lat[wh], lon[wh], data[wh] * area[wh], bins=bins, statistic="sum")[0]
        return a / stats.binned_statistic_2d(lat[wh], lon[wh], area[wh], bins=bins, statistic="sum")[0]
    with np.errstate(all="ignore"):
        say(f"  CPU: the two scipy.stats.binned_statistic_2d sums of grid_flux.py (one variable) {cpu(reference):.0f} ms")
    del dev
    torch.cuda.empty_cache()


def nexrad_case(n, rate):
    rng = np.random.default_rng(3)
    y, x, t, edges = scattered(n, rng)
    y, x = y * 0.3, x * 0.3                                       # a site covers part of the grid
    alt = rng.uniform(1000, 17000, n)
    ref = rng.uniform(-20, 60, n).astype(np.float32)
    valid = rng.random(n) < 0.7
    keep = (alt > 2500) & (alt < 15000)
    ws, we = np.arange(T, dtype=np.int64) * 1000 - 100, (np.arange(T, dtype=np.int64) + 1) * 1000 + 100       # overlapping
    say(f"nexrad: {n} float64 gates of one site onto {T} x {N}^2: int32 raw count, int32 valid count, float64 reflectivity sum")
    dev = [_lib.to_dev(a) for a in (y, x, t, ref, valid, keep)]
    kw = dict(rule="scipy", values=dev[3], keep=dev[5], keep_value=dev[4], time=dev[2], win_start=ws, win_end=we, flip=(0,),
              outputs=("count", "count_v", "sum_wv"))
    measure("three outputs", dev[:2], [edges, edges], n * 30, rate, lambda: binning.bin_points(dev[:2], [edges, edges], **kw), **kw)
    m = n // T
    ym, xm, rm, vm = y[:m][keep[:m]], x[:m][keep[:m]], ref[:m][keep[:m]], valid[:m][keep[:m]]

    def reference():
        np.histogram2d(ym, xm, bins=(edges, edges))
        np.histogram2d(ym[vm], xm[vm], bins=(edges, edges))
        stats.binned_statistic_dd((ym[vm], xm[vm]), rm[vm], statistic="mean", bins=(edges, edges), expand_binnumbers=True)
    ms = cpu(reference)
    say(f"  CPU: the two np.histogram2d and the binned_statistic_dd of one frame's {m} gates {ms:.0f} ms -> {T} frames {ms * T:.0f} ms")
    del dev
    torch.cuda.empty_cache()


def main():
    _lib.device()
    say(f"point binning, N = {N}, T = {T}, S = {S}; {torch.cuda.get_device_name(0)}; median of {RUNS} after {WARM} warm-up")
    rate = copy_rate()
    say(f"tf_copy16 on 1 GiB: {rate / 1e12:.2f} TB/s read (+ as much written)")
    glm_case(10 ** 6, rate)
    glm_case(10 ** 7, rate)
    flux_case(rate)
    nexrad_case(2 * 10 ** 6, rate)


if __name__ == "__main__":
    main()
