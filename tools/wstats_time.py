"""Time the per-label weighted statistics of the post-processing scripts (tobac_flow_amd.postprocess) on a synthetic
T x N^2 detection output: three step-label volumes (cold blobs thresholded at three levels, labelled, cut per frame),
float32 fields with uncertainties and an (N, N) area plane as weights, everything device-resident.

  figure 1  add_weighted_stats_to_dataset for VARS variables x 3 step volumes: wall time with a device synchronise.  Per
            call the library launches k_wstats_init, k_wstats_pass1, k_wstats_pass2 and k_wstats_finish and allocates
            128 B + 80 B per label id; no array of T * N^2 elements is made (the allocator's peak is printed)
  figure 2  tf_label_wstats and tf_label_proportions alone (HIP events) against the bytes they must read -- 12 B per voxel
            in each pass over labels, field and weights(*), plus 4 B per LABELLED voxel for the errors in pass 1 -- next to
            torch's copy_ moving the same number of bytes.  (*) weights as a plane re-read every frame; as a volume too.
            `python tools/wstats_time.py kernels` runs only this part, e.g. under `rocprofv3 --kernel-trace --stats --`
            for the split between the two passes
  figure 3  the numpy form (a bincount-free stable argsort of the whole volume and a Python function per label: the
            package's own host path, which is what the reference's apply_func_to_labels does per call) at T x CPU_N^2 on
            the host, and this package on the same host arrays, uploads included

Usage: python tools/wstats_time.py [all|kernels] [N] [T] [CPU_N] [VARS] (development aid; the figures are kept in
profiles/weighted_stats_notes.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import torch

from tobac_flow_amd import _lib, label as _label, ndimage_dev as nd, postprocess as pp
from tobac_flow_amd.dataset import LabelDataset

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 5424
T = int(sys.argv[3]) if len(sys.argv) > 3 else 16
CPU_N = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
VARS = int(sys.argv[5]) if len(sys.argv) > 5 else 10
WARM, RUNS = 1, 5
KINDS = (("core", 245.0), ("thick_anvil", 262.0), ("thin_anvil", 274.0))


def output(T, N):
    """(dcc dataset with the three step-label volumes and their coordinates, field dataset, area plane), on the device"""
    from synth import blob_stack
    dev = _lib.device()
    bt = torch.nan_to_num(blob_stack(T, N, N), nan=290.0)
    dcc = LabelDataset()
    for kind, level in KINDS:
        labels, _ = nd.label(bt < level)
        step, n = _label.slice_labels_dev(labels)
        del labels
        dcc.add(kind + "_step_label", step, ("t", "y", "x"))
        dcc.coords[kind + "_step"] = np.arange(1, int(n) + 1, dtype=np.int32)
    err = (0.5 + 0.001 * (bt - 200.0)).contiguous()
    fields = LabelDataset()
    for k in range(VARS):                                         # the same two tensors under VARS names: the reads are the same
        fields["v%d" % k] = bt
        fields["v%d_uncertainty" % k] = err
    y, x = np.linspace(0.12, -0.12, N), np.linspace(-0.12, 0.12, N)
    yy, xx = np.meshgrid(y, x, indexing="ij")
    area = torch.from_numpy((4.0 / np.cos(2.0 * yy + xx) ** 2).astype(np.float32)).to(dev)
    return dcc, fields, area


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


def figure_1(dcc, fields, area):
    def run():
        for kind, _ in KINDS:
            for k in range(VARS):
                pp.add_weighted_stats_to_dataset(dcc, fields, area, "v%d" % k, kind + "_step")

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    med, lo, hi = median(run, wall)
    calls = 3 * VARS
    print(f"figure 1: {calls} add_weighted_stats_to_dataset calls ({VARS} variables with uncertainties x 3 step volumes): median "
          f"{med:.1f} ms (min {lo:.1f}, max {hi:.1f}) = {med / calls:.2f} ms per call; 4 library launches per call; peak device "
          f"memory above the inputs {(torch.cuda.max_memory_allocated() - base) / 1e6:.1f} MB (one field is {T * N * N * 4 / 1e6:.0f} MB)",
          flush=True)


def figure_2(dcc, fields, area):
    L, dev = _lib.lib(), _lib.device()
    n_vox = T * N * N
    x, e = fields["v0"], fields["v0_uncertainty"]
    wvol = area[None].expand(T, N, N).contiguous()
    for kind, _ in KINDS:
        lab = dcc[kind + "_step_label"]
        n = int(dcc.coords[kind + "_step"].size)
        f = float((lab != 0).float().mean())
        out = torch.empty((max(n, 1), 10), dtype=torch.float64, device=dev)
        ws = torch.empty(L.tf_label_wstats_workspace_bytes(n), dtype=torch.uint8, device=dev)
        for what, ep, w, plane in (("errors, plane weights", e, area, 1), ("no errors, plane weights", None, area, 1),
                                   ("errors, volume weights", e, wvol, 0)):
            def run():
                _lib.check(L.tf_label_wstats(_lib.ptr(lab), _lib.ptr(x), _lib.ptr(ep), _lib.ptr(w), _lib.TF_F32, T, N * N, plane,
                                             n, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_wstats")

            med, lo, hi = median(run, events)
            gb = (24 + (4 * f if ep is not None else 0)) * n_vox / 1e9
            print(f"figure 2: tf_label_wstats {kind}_step_label ({what}; {n} ids, {f * 100:.1f} % labelled): median {med:.3f} ms "
                  f"(min {lo:.3f}, max {hi:.3f}) = {gb / med * 1e3:.0f} GB/s of the {gb:.2f} GB both passes must read", flush=True)
    lab = dcc["thin_anvil_step_label"]
    n = int(dcc.coords["thin_anvil_step"].size)
    flags = (fields["v0"] > 270.0).to(torch.int32) + (fields["v0"] > 285.0).to(torch.int32)
    values = np.array([0, 1, 2, 3], np.int32)
    out = torch.empty((max(n, 1), 4), dtype=torch.float64, device=dev)
    ws = torch.empty(L.tf_label_proportions_workspace_bytes(n, 4), dtype=torch.uint8, device=dev)

    def prop():
        _lib.check(L.tf_label_proportions(_lib.ptr(lab), _lib.ptr(flags), _lib.ptr(area), T, N * N, 1, n, values.ctypes.data, 4,
                                          _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_proportions")

    med, lo, hi = median(prop, events)
    gb = 12 * n_vox / 1e9
    print(f"figure 2: tf_label_proportions thin_anvil_step_label (4 flag values, {n} ids): median {med:.3f} ms (min {lo:.3f}, "
          f"max {hi:.3f}) = {gb / med * 1e3:.0f} GB/s of {gb:.2f} GB", flush=True)
    # the practical ceiling: torch's device-to-device copy, 12 B per voxel read and 12 B written = one wstats call's reads
    src = torch.empty(3 * n_vox, dtype=torch.float32, device=dev).zero_()
    dst = torch.empty_like(src)
    med, lo, hi = median(lambda: dst.copy_(src), events)
    print(f"figure 2: copy_ of 12 B per voxel: median {med:.3f} ms = {24 * n_vox / 1e9 / med * 1e3:.0f} GB/s read + written "
          f"(24 B per voxel moved, as many as the two passes read)", flush=True)


def figure_3():
    dcc, fields, area = output(T, CPU_N)
    lab = dcc["thin_anvil_step_label"].cpu().numpy()
    ids = dcc.coords["thin_anvil_step"]
    host = {"v0": fields["v0"].cpu().numpy(), "v0_uncertainty": fields["v0_uncertainty"].cpu().numpy()}
    w = area.cpu().numpy()
    del dcc, fields, area
    t0 = time.perf_counter()
    want = pp._host_regions(lab, [host["v0"].astype(np.float64), host["v0_uncertainty"].astype(np.float64),
                                  np.broadcast_to(w, lab.shape).astype(np.float64)],
                            pp.stats_utils.weighted_stats_and_uncertainties, ids.astype(np.int64), 8)
    t1 = time.perf_counter()
    print(f"figure 3: numpy form on the host at {T} x {CPU_N}^2, one variable on thin_anvil_step_label ({ids.size} ids, one run): "
          f"{(t1 - t0) * 1e3:.0f} ms", flush=True)
    got = []
    med, lo, hi = median(lambda: got.append(pp.weighted_label_stats(lab, w, host, "v0", ids, "thin_anvil_step", uncertainty=True,
                                                                    dtype=np.float64)), wall)
    print(f"figure 3: this package on the same HOST arrays (uploads included): median {med:.1f} ms (min {lo:.1f}, max {hi:.1f})",
          flush=True)
    mine = np.stack([v for _, v in got[-1]], 1)
    same = np.array_equal(np.isnan(mine), np.isnan(want)) and np.allclose(mine, want, rtol=1e-9, atol=0, equal_nan=True)
    print("figure 3: results equal to the host form within rtol 1e-9:", same, flush=True)


if __name__ == "__main__":
    ds = output(T, N)
    print(f"{T} x {N}^2 synthetic output on the device; ids: " + ", ".join(f"{k}_step {ds[0].coords[k + '_step'].size}" for k, _ in KINDS),
          flush=True)
    if MODE == "all":
        figure_1(*ds)
    figure_2(*ds)
    del ds
    _lib.release_workspaces()
    torch.cuda.empty_cache()
    if MODE == "all":
        figure_3()
