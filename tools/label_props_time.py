"""Time calculate_label_properties and the three get_label_stats calls of the drop-in script on a synthetic detection
output (T x N^2 device-resident label volumes: cold blobs thresholded at three levels and labelled, then the script's own
add_label_coords / link_cores_and_anvils / add_step_labels / link_step_labels), and each kernel on its own against the
bytes it must read (4 B per voxel, the labels once).  Then the same two calls in their numpy form -- the reference's
calls, np.repeat stacks and a sort along the axis for the unique counts included -- on the CPU at T x CPU_N^2 (the full size takes minutes on the host).
Wall time around each call with a device synchronise, HIP events around each kernel; median of RUNS after WARM warm-ups.
Usage: python tools/label_props_time.py [N] [T] [CPU_N] (development aid; the figures are kept in
profiles/label_props_notes.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import scipy.ndimage as ndi
import torch

from tobac_flow_amd import _lib, analysis, dataset as D, ndimage_dev as nd
from tobac_flow_amd.utils.stats_utils import _sorted_form

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
CPU_N = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
WARM, RUNS = 1, 5
KINDS = ("core", "thick_anvil", "thin_anvil")


def detection_output(T, N, device_volumes):
    """a LabelDataset as the script holds it before calculate_label_properties"""
    from synth import blob_stack
    _lib.device()
    bt = blob_stack(T, N, N)
    bt = torch.nan_to_num(bt, nan=290.0)
    core, _ = nd.label(bt < 245.0)
    thick, n_thick = nd.label(bt < 262.0)
    thin, _ = nd.label(bt < 274.0)
    thin = torch.where(thick != 0, thick, (thin + n_thick) * (thin != 0)).to(torch.int32)
    del bt
    y, x = np.linspace(0.12, -0.12, N), np.linspace(-0.12, 0.12, N)
    yy, xx = np.meshgrid(y, x, indexing="ij")
    ds = D.LabelDataset(coords={"t": np.datetime64("2020-06-01T00:00", "ns") + np.arange(T) * np.timedelta64(300, "s"),
                                "x": x, "y": y})
    ds.add("area", 4.0 / np.cos(2.0 * yy + xx) ** 2, ("y", "x"))
    ds.add("lat", 400.0 * yy, ("y", "x"))
    ds.add("lon", -75.0 + 500.0 * xx, ("y", "x"))
    for name, v in (("core_label", core), ("thick_anvil_label", thick), ("thin_anvil_label", thin)):
        ds.add(name, v if device_volumes else v.cpu().numpy(), ("t", "y", "x"))
    for fn in (D.add_label_coords, D.link_cores_and_anvils, D.add_step_labels, D.add_label_coords, D.link_step_labels):
        fn(ds)
    return ds


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(f, timer):
    for _ in range(WARM):
        f()
    ts = [timer(f) for _ in range(RUNS)]
    return statistics.median(ts), min(ts), max(ts)


def gpu_part():
    ds = detection_output(T, N, True)
    sizes = {c: int(ds.coords[c].size) for c in ("core", "anvil", "core_step", "thick_anvil_step", "thin_anvil_step")}
    print(f"{T} x {N}^2 synthetic detection output, label volumes on the device; labels: {sizes}", flush=True)

    def props():
        D.calculate_label_properties(ds)

    def stats():
        for k in KINDS:
            analysis.get_label_stats(k + "_label", ds)

    for name, f in (("calculate_label_properties", props), ("3 x get_label_stats", stats)):
        med, lo, hi = median(f, wall)
        print(f"{name}: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}); {RUNS} runs after {WARM} warm-up", flush=True)

    # the kernels on their own: device operands, outputs and scratch allocated beforehand
    L = _lib.lib()
    dev = _lib.device()
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)     # noqa: E731
    area, lat, lon = (f64(ds[k]) for k in ("area", "lat", "lon"))
    x, y = (f64(ds.coords[k]) for k in ("x", "y"))
    rank = torch.arange(T, dtype=torch.int32, device=dev)
    gb = T * N * N * 4 / 1e9
    null = None
    for vol, coord, full in (("thin_anvil_step_label", "thin_anvil_step", True), ("thin_anvil_label", "anvil", False),
                             ("core_step_label", "core_step", True)):
        v = ds[vol]
        n = int(ds.coords[coord].max())
        acc = torch.empty((n + 1, 8), dtype=torch.float64, device=dev)
        ops = [_lib.ptr(area)] + ([_lib.ptr(k) for k in (x, y, lat, lon)] if full else [null] * 4) + [_lib.ptr(rank)]

        def run():
            _lib.check(L.tf_label_props(_lib.ptr(v), T, N, N, n, *ops, _lib.ptr(acc), _lib.stream_ptr()), "tf_label_props")

        med, lo, hi = median(run, events)
        print(f"tf_label_props {vol} ({'all sums' if full else 'count, area, times'}, {n} ids, "
              f"{float((v != 0).float().mean()) * 100:.1f} % labelled): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) "
              f"= {gb / med * 1e3:.0f} GB/s of the {gb:.2f} GB it must read", flush=True)
    v = ds["thin_anvil_label"]
    uniq, nz = torch.empty((N, N), dtype=torch.int32, device=dev), torch.empty((N, N), dtype=torch.int32, device=dev)

    def along_t():
        _lib.check(L.tf_unique_along_t(_lib.ptr(v), T, N, N, _lib.ptr(uniq), _lib.ptr(nz), None, None, 0, _lib.stream_ptr()),
                   "tf_unique_along_t")

    med, lo, hi = median(along_t, events)
    print(f"tf_unique_along_t thin_anvil_label: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {gb / med * 1e3:.0f} GB/s "
          f"of {gb:.2f} GB", flush=True)
    n = int(v.max())
    ws = torch.empty(L.tf_unique_per_frame_workspace_bytes(n), dtype=torch.uint8, device=dev)
    per, cnt = torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.int64, device=dev)

    def per_frame():
        _lib.check(L.tf_unique_per_frame(_lib.ptr(v), T, N * N, n, _lib.ptr(per), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "tf_unique_per_frame")

    med, lo, hi = median(per_frame, events)
    print(f"tf_unique_per_frame thin_anvil_label ({T} launches): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = "
          f"{gb / med * 1e3:.0f} GB/s of {gb:.2f} GB", flush=True)
    # the practical ceiling: torch's device-to-device copy of one volume (reads and writes 4 B per voxel each)
    dst = torch.empty_like(v)
    med, lo, hi = median(lambda: dst.copy_(v), events)
    print(f"copy_ of one volume: median {med:.3f} ms = {2 * gb / med * 1e3:.0f} GB/s read + written", flush=True)


# ---- the numpy form: the reference's calls (dataset.py:705-1595, analysis.py:245-290) on host arrays ---------------------
def _weighted(labels, field, weights):
    """np.average(field, weights=weights) per label 1 .. max, found the reference's way: a bincount and an argsort of the
    whole volume per call"""
    flat = labels.ravel()
    order = np.argsort(flat)
    ends = np.cumsum(np.bincount(flat))
    f, w = field.ravel(), weights.ravel()
    out = np.full(ends.size - 1, np.nan)
    for i in range(ends.size - 1):
        sel = order[ends[i]:ends[i + 1]]
        if sel.size:
            out[i] = np.average(f[sel], weights=w[sel])
    return out


def numpy_properties(ds):
    out = {}
    t = ds.coords["t"]
    area = ds["area"]
    for kind, dim in zip(KINDS, ("core", "anvil", "anvil")):
        for vol, ids in ((ds[kind + "_label"], ds.coords[dim]), (ds[kind + "_step_label"], ds.coords[kind + "_step"])):
            out[len(out)] = np.bincount(vol.ravel())
            out[len(out)] = ndi.labeled_comprehension(area[np.newaxis], vol, ids, np.nansum, np.float32, np.nan)
            out[len(out)] = ndi.labeled_comprehension(t[:, None, None], vol, ids, np.nanmin, "datetime64[ns]", None)
            out[len(out)] = ndi.labeled_comprehension(t[:, None, None], vol, ids, np.nanmax, "datetime64[ns]", None)
    area_stack = np.repeat(area[np.newaxis], t.size, 0)
    xx, yy = np.meshgrid(ds.coords["x"], ds.coords["y"])
    for plane in (xx, yy, ds["lat"], ds["lon"]):
        stack = np.repeat(plane[np.newaxis], t.size, 0)
        for kind in KINDS:
            out[len(out)] = _weighted(ds[kind + "_step_label"], stack, area_stack)
    return out


def numpy_label_stats(a):
    T = a.shape[0]
    return (np.count_nonzero(a, 0) / T, _sorted_form(a, 0), np.count_nonzero(a, (1, 2)) / (a.shape[1] * a.shape[2]),
            _sorted_form(a.reshape([T, -1]), 1))


def cpu_part():
    ds = detection_output(T, CPU_N, False)
    for k in list(ds):
        ds[k] = D._host(ds[k])
    t0 = time.perf_counter()
    numpy_properties(ds)
    t1 = time.perf_counter()
    for k in KINDS:
        numpy_label_stats(ds[k + "_label"])
    t2 = time.perf_counter()
    print(f"numpy form on the host at {T} x {CPU_N}^2 (one run): calculate_label_properties {(t1 - t0) * 1e3:.0f} ms, "
          f"3 x get_label_stats {(t2 - t1) * 1e3:.0f} ms", flush=True)
    f = lambda: D.calculate_label_properties(ds)                  # noqa: E731
    g = lambda: [analysis.get_label_stats(k + "_label", ds) for k in KINDS]      # noqa: E731
    (a, _, _), (b, _, _) = median(f, wall), median(g, wall)
    print(f"this package at {T} x {CPU_N}^2, HOST label volumes (uploads included): calculate_label_properties {a:.1f} ms, "
          f"3 x get_label_stats {b:.1f} ms", flush=True)


if __name__ == "__main__":
    gpu_part()
    _lib.release_workspaces()
    torch.cuda.empty_cache()
    cpu_part()
