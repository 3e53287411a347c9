"""Time tf_field_stats on one T x N^2 float32 field (default 16 x 5424^2, 1.9 GB), everything device-resident.

  figure 1  the copy kernel (tf_copy16 over two buffers of the field's size): the practical ceiling, GB/s read + written
  figure 2  each geometry alone (HIP events around the library call): time, the reads of the volume it makes, the rate
            reads x bytes / time and that rate as a fraction of the copy kernel's
  figure 3  the per-pixel form's general path on T2 frames (default 65, one more than the single-read path takes)
  figure 4  the three public functions from a device tensor (wall time with a device synchronise)
  figure 5  the NumPy path of the three public functions on this machine's CPU, one run each (skipped with CPU=0)

Usage: python tools/field_stats_time.py [N] [T] [T2] [CPU] (development aid; the figures are kept in
profiles/field_stats.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from tobac_flow_amd import _lib, dataset, ndimage_dev as nd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
T2 = int(sys.argv[3]) if len(sys.argv) > 3 else 65
CPU = int(sys.argv[4]) if len(sys.argv) > 4 else 1
WARM, RUNS = 2, 7
READS = {"all": 5, "frame": 5, "time": 1}                          # float32: 2 moment sweeps + 3 digit passes; one tile read


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


def median(f, timer):
    for _ in range(WARM):
        f()
    ts = [timer(f) for _ in range(RUNS)]
    return statistics.median(ts), min(ts), max(ts)


def field(frames):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((frames, N, N), generator=g, device="cuda", dtype=torch.float32).mul_(20).add_(250)
    x[:, : N // 50, :] = float("nan")                               # off-disc rows, as a full-disc field has
    return x


def main():
    L = _lib.lib()
    x = field(T)
    gb = x.numel() * 4 / 1e9
    dst = torch.empty_like(x)
    med, lo, hi = median(lambda: _lib.check(L.tf_copy16(_lib.ptr(x), _lib.ptr(dst), x.numel() * 4, _lib.stream_ptr()), "tf_copy16"), events)
    copy_rate = 2 * gb / med * 1e3
    print(f"figure 1: copy kernel, {gb:.2f} GB read + written: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {copy_rate:.0f} GB/s", flush=True)
    del dst
    for over in ("all", "frame", "time"):
        med, lo, hi = median(lambda: nd.field_stats(x, over), events)
        rate = READS[over] * gb / med * 1e3
        print(f"figure 2: {T} x {N}^2 float32, over={over!r}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {READS[over]} read(s) of "
              f"{gb:.2f} GB = {rate:.0f} GB/s = {rate / copy_rate * 100:.0f} % of the copy kernel's rate per read", flush=True)
    got = {}
    for name in ("get_bulk_stats", "get_spatial_stats", "get_temporal_stats"):
        med, lo, hi = median(lambda: got.__setitem__(name, getattr(dataset, name)(x)), wall)
        print(f"figure 4: dataset.{name} from a device tensor: median {med:.2f} ms wall (min {lo:.2f}, max {hi:.2f})", flush=True)
    if T2:
        y = field(T2)
        reads = 19 if T2 > nd.FIELD_STATS_LDS_FRAMES["float32"] else 1
        med, lo, hi = median(lambda: nd.field_stats(y, "time"), events)
        g2 = y.numel() * 4 / 1e9
        print(f"figure 3: {T2} x {N}^2 float32, over='time': median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); {reads} read(s) of "
              f"{g2:.2f} GB = {reads * g2 / med * 1e3:.0f} GB/s nominal = {reads * g2 / med * 1e3 / copy_rate * 100:.0f} % of the copy "
              f"kernel's rate per read", flush=True)
        del y
    if CPU:
        import warnings
        warnings.simplefilter("ignore")
        h = x.cpu().numpy()
        for name in ("get_bulk_stats", "get_spatial_stats", "get_temporal_stats"):
            t0 = time.perf_counter()
            want = getattr(dataset, name)(h)
            t1 = time.perf_counter()
            same = [bool(np.array_equal(w, g.cpu().numpy(), equal_nan=True)) for w, g in zip(want, got[name])]
            print(f"figure 5: dataset.{name} on the CPU (NumPy path), one run: {(t1 - t0) * 1e3:.0f} ms; device result equal to it "
                  f"(mean, std, median, max, min): {same}", flush=True)


if __name__ == "__main__":
    main()
