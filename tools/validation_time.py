"""Time the GLM validation on a synthetic detection output (T x N^2 device-resident core labels: cold blobs thresholded
and labelled; a sparse float64 flash grid): get_marker_distance_cylinder with and without get_closest, validate_markers,
tf_edt2d_frames, tf_edt_cylinder and tf_label_nanmin on their own (the last on the sparse core labels and on dense anvil
labels, against the bytes it really reads), and three frames that take the transform apart: every voxel a feature (the
row scan stops at once: what is left is the column pass and the row pass's loads and stores), ONE feature in a corner (the
worst case of the pruned row scan, every pixel walks its row), and no feature (its rows are filled, not scanned).  Next to them scipy.ndimage.distance_transform_edt, the call the device path replaces, on
ONE frame of the same labels and on the single-feature frame, on this machine's CPU.  The 3-D transform with a time
sampling: get_marker_distance_ellipse_dev, tf_edt_time_envelope alone (with and without the nearest features), beside them
tf_edt_cylinder with sources, and SciPy's 3-D call with sampling (margin / time_margin, 1, 1) on as many frames of the
labels as it finishes in about SCIPY_SECONDS (two frames first, then the count their time predicts; 0 skips it).
Wall time around each call with a device synchronise, HIP events around the kernels; median of RUNS after WARM warm-ups.
Usage: python tools/validation_time.py [N] [T] [SCIPY_SECONDS] (development aid; the figures are kept in
profiles/validation_edt.txt and profiles/validation_ellipse.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import scipy.ndimage as ndi
import torch

from tobac_flow_amd import _lib, ndimage_dev as nd, validation

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
SCIPY_SECONDS = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
MARGIN, TIME_MARGIN = 10, 3                                       # the defaults of scripts/dcc_validation.py
WARM, RUNS = 1, 3


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


def report(name, f, timer=wall):
    med, lo, hi = median(f, timer)
    print(f"{name}: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}); {RUNS} runs after {WARM} warm-up", flush=True)
    return med


def main():
    from synth import blob_stack
    dev = _lib.device()
    bt = torch.nan_to_num(blob_stack(T, N, N), nan=290.0)
    labels, n_labels = nd.label(bt < 245.0)
    anvils, n_anvils = nd.label(bt < 262.0)                         # dense labels: the thick anvils around the cores
    del bt
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    near = nd.edt_squared_frames(labels)[0] < 40 * 40             # flashes fall near the cores, most of them
    chance = torch.rand((T, N, N), generator=gen, device=dev)
    grid = ((chance < 2e-4) & near) | (chance < 5e-6)
    grid = (grid * torch.randint(1, 4, (T, N, N), generator=gen, device=dev)).to(torch.float64)
    del near, chance
    print(f"{T} x {N}^2: {n_labels} core labels over {float((labels != 0).float().mean()) * 100:.2f} % of the voxels, "
          f"{int(grid.sum())} flashes in {int((grid != 0).sum())} voxels; margin {MARGIN}, time margin {TIME_MARGIN}", flush=True)

    report("get_marker_distance_cylinder(labels)", lambda: validation.get_marker_distance_cylinder(labels, TIME_MARGIN))
    report("get_marker_distance_cylinder(labels, get_closest=True)",
           lambda: validation.get_marker_distance_cylinder(labels, TIME_MARGIN, get_closest=True))
    report("get_marker_distance_ellipse_dev(labels)", lambda: validation.get_marker_distance_ellipse_dev(labels, TIME_MARGIN, MARGIN))
    report("get_marker_distance_cylinder(flash grid)", lambda: validation.get_marker_distance_cylinder(grid, TIME_MARGIN))
    glm_distance = validation.get_marker_distance_cylinder(grid, TIME_MARGIN)
    edge = torch.zeros((T, N, N), dtype=torch.bool, device=dev)      # get_edge_filter's result without gaps or missing data
    edge[TIME_MARGIN:T - TIME_MARGIN, MARGIN:N - MARGIN, MARGIN:N - MARGIN] = True
    grid = grid * edge
    n_in = float(grid.sum())
    coord = np.arange(1, n_labels + 1)
    out = {}

    def validate():
        out["r"] = validation.validate_markers(labels, grid, glm_distance, edge, n_in, coord=coord, margin=MARGIN, time_margin=TIME_MARGIN)

    report("validate_markers", validate)
    print(f"  POD {out['r'][3]:.4f}, FAR {out['r'][4]:.4f}, {out['r'][5]} of {n_labels} labels inside the margin", flush=True)
    report("tf_edt2d_frames (labels, d2 only)", lambda: nd.edt_squared_frames(labels), events)
    report("tf_edt2d_frames (labels, d2 and nearest)", lambda: nd.edt_squared_frames(labels, True), events)
    d2 = nd.edt_squared_frames(labels)[0]
    report("tf_edt_cylinder (distances only)", lambda: nd.edt_cylinder(d2, None, TIME_MARGIN), events)
    nearest = nd.edt_squared_frames(labels, True)[1]
    report("tf_edt_cylinder (distances and sources)", lambda: nd.edt_cylinder(d2, nearest, TIME_MARGIN), events)
    env = report(f"tf_edt_time_envelope alone (sampling {MARGIN}/{TIME_MARGIN}, distances and sources)",
                 lambda: nd.edt_time_envelope(d2, nearest, MARGIN / TIME_MARGIN), events)
    moved = d2.numel() * (4 + 4 + 8 + 8)                           # d2 once, nearest at the winners, dist and src once
    print(f"  = {moved / 1e6 / env:.0f} GB/s of the {moved / 1e9:.2f} GB it has to move (d2 and nearest read once, dist and src written)", flush=True)
    report(f"tf_edt_time_envelope alone (sampling {MARGIN}/{TIME_MARGIN}, distances only, no nearest)",
           lambda: nd.edt_time_envelope(d2, None, MARGIN / TIME_MARGIN), events)
    report("tf_edt_time_envelope alone (sampling 1e9: no frame looks beyond itself)", lambda: nd.edt_time_envelope(d2, nearest, 1e9), events)
    report("tf_edt_time_envelope alone (sampling 0.3: every scan runs to the ends of t)", lambda: nd.edt_time_envelope(d2, nearest, 0.3), events)
    del nearest
    # tf_label_nanmin alone (its init, pass and finish kernels; operands, outputs and scratch allocated beforehand).  It
    # reads 4 B of labels per voxel and the field only under the lanes that hold a label among their four voxels
    L = _lib.lib()
    for name, vol, n_ids in (("core labels", labels, n_labels), ("thick anvil labels", anvils, n_anvils)):
        ids = torch.arange(1, n_ids + 1, dtype=torch.int64, device=dev)
        out_min = torch.empty(n_ids, dtype=torch.float64, device=dev)
        out_count = torch.empty(n_ids, dtype=torch.int64, device=dev)
        ws = torch.empty(L.tf_label_nanmin_workspace_bytes(n_ids), dtype=torch.uint8, device=dev)

        def run():
            _lib.check(L.tf_label_nanmin(_lib.ptr(vol), _lib.ptr(glm_distance), _lib.TF_F64, vol.numel(), n_ids, _lib.ptr(ids), n_ids,
                                         _lib.ptr(out_min), _lib.ptr(out_count), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_nanmin")

        groups = int((vol.reshape(-1, 4) != 0).any(1).sum())
        read = vol.numel() * 4 + groups * 32
        med, lo, hi = median(run, events)
        print(f"tf_label_nanmin alone, float64 field, {name} ({n_ids} ids, {float((vol != 0).float().mean()) * 100:.2f} % labelled): median "
              f"{med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {read / 1e6 / med:.0f} GB/s of the {read / 1e9:.2f} GB it reads "
              f"({vol.numel() * 12 / 1e9:.2f} GB if it read the whole field)", flush=True)
    del anvils

    full = torch.ones((T, N, N), dtype=torch.uint8, device=dev)
    report(f"tf_edt2d_frames, {T} frames, every voxel a feature (column pass + loads and stores of the row pass)",
           lambda: nd.edt_squared_frames(full, True), events)
    del full
    one = torch.zeros((1, N, N), dtype=torch.uint8, device=dev)
    report("tf_edt2d_frames, ONE frame without a feature (rows filled, not scanned)", lambda: nd.edt_squared_frames(one, True), events)
    one[0, -1, -1] = 1
    worst = report("tf_edt2d_frames, ONE frame with a single feature (worst case of the row scan)",
                   lambda: nd.edt_squared_frames(one, True), events)
    frame = labels[T // 2].cpu().numpy()
    t0 = time.perf_counter()
    ndi.distance_transform_edt(frame == 0, return_indices=True)
    t1 = time.perf_counter()
    ndi.distance_transform_edt(one[0].cpu().numpy() == 0, return_indices=True)
    t2 = time.perf_counter()
    print(f"scipy.ndimage.distance_transform_edt with indices on this machine's CPU, ONE {N}^2 frame (one run): labels "
          f"{(t1 - t0) * 1e3:.0f} ms, single feature {(t2 - t1) * 1e3:.0f} ms (device, single feature: {worst:.1f} ms)", flush=True)
    if SCIPY_SECONDS > 0:
        sampling = (MARGIN / TIME_MARGIN, 1, 1)
        host = labels.cpu().numpy() == 0
        frames = min(2, T)
        while True:
            t0 = time.perf_counter()
            ndi.distance_transform_edt(host[:frames], return_indices=True, sampling=sampling)
            seconds = time.perf_counter() - t0
            print(f"scipy.ndimage.distance_transform_edt, 3-D with indices, sampling ({MARGIN}/{TIME_MARGIN}, 1, 1), on this machine's CPU, "
                  f"{frames} x {N}^2 frames (one run): {seconds:.1f} s = {seconds / frames:.2f} s per frame", flush=True)
            more = min(T, int(frames * SCIPY_SECONDS / seconds))
            if more <= frames or frames > 2:
                break
            frames = more


if __name__ == "__main__":
    main()
