"""Time Flow.label with and without subsegmentation on a synthetic T x N^2 mask (cold blobs below 262 K, device-resident;
zero flow vectors): flow.label(mask, overlap=0.5, absolute_overlap=4, subsegment_shrink=0.1) against subsegment_shrink=0 on
the same build, subsegment_labels alone, and its stages on their own.  Where scikit-image is importable, the reference's
recipe (tobac_flow/label.py:13-80, restated with scikit-image's own peak_local_max and watershed) on ONE frame on this
machine's CPU; where it is not, the script says so.  Wall time around each call with a device synchronise; median of RUNS
after WARM warm-ups.
Usage: python tools/subsegment_time.py [N] [T] (development aid; the figures are kept in profiles/subsegment.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import scipy.ndimage as ndi
import torch

from tobac_flow_amd import _lib, label, ndimage_dev as nd
from tobac_flow_amd.flow import Flow

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
SHRINK, MIN_DISTANCE = 0.1, 5                                     # Flow.label's peak_min_distance default
WARM, RUNS = 1, 2


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(name, f):
    for _ in range(WARM):
        f()
    ts = [wall(f) for _ in range(RUNS)]
    print(f"{name}: median {statistics.median(ts):.0f} ms (min {min(ts):.0f}, max {max(ts):.0f}); {RUNS} runs after {WARM} warm-up", flush=True)


def reference_frame(frame, shrink, distance):
    """label.py:13-80 on one (H, W) frame with scikit-image's own functions"""
    from skimage.feature import peak_local_max
    from skimage.segmentation import watershed
    labels = ndi.label(frame)[0]
    dist = ndi.distance_transform_edt(labels)
    dist /= ((np.bincount(labels.ravel()) / np.pi) ** 0.5)[labels]
    seeds = dist > shrink
    seeds[tuple(peak_local_max(dist, min_distance=distance, threshold_abs=1e-8).T)] = True
    markers = ndi.label(seeds)[0]
    markers[labels == 0] = -1
    return watershed(-dist, markers, mask=labels != 0)


def main():
    from synth import blob_stack
    dev = _lib.device()
    mask = torch.nan_to_num(blob_stack(T, N, N), nan=290.0) < 262.0
    still = torch.zeros((T, N, N, 2), dtype=torch.float32, device=dev)
    flow = Flow(still, still)
    flat = nd.flat_label(mask)
    print(f"{T} x {N}^2 mask: {float(mask.float().mean()) * 100:.1f} % set, {int(flat.max())} per-frame regions; shrink {SHRINK}, "
          f"peak_min_distance {MIN_DISTANCE}", flush=True)
    del flat
    out = {}

    def split():
        out["stats"] = []
        out["flat"] = label.subsegment_labels_dev(mask, SHRINK, MIN_DISTANCE, stats=out["stats"])

    report(f"flow.label(mask, overlap=0.5, absolute_overlap=4, subsegment_shrink=0)",
           lambda: flow.label(mask, overlap=0.5, absolute_overlap=4, subsegment_shrink=0))
    report(f"flow.label(mask, overlap=0.5, absolute_overlap=4, subsegment_shrink={SHRINK})",
           lambda: flow.label(mask, overlap=0.5, absolute_overlap=4, subsegment_shrink=SHRINK, peak_min_distance=MIN_DISTANCE))
    report("subsegment_labels alone", split)
    print(f"  {int(out['flat'].max())} subsegments, {int(((out['flat'] == 0) & mask).sum())} mask voxels without a label", flush=True)
    del out["flat"]
    for frame, st in out["stats"][:1] + out["stats"][-1:]:
        print(f"  flood of frame {frame}: sweeps {st['sweeps']}, chain depth {st['chain_depth']}, root phases {st['root_phases']}, "
              f"reference order {st['reference_order']}, {st['reference_order_detail']}", flush=True)

    labels = nd.flat_label(mask)
    report("  flat_label", lambda: nd.flat_label(mask))
    report("  edt_squared_frames", lambda: nd.edt_squared_frames(labels == 0))
    d2 = nd.edt_squared_frames(labels == 0)[0]
    n_labels = int(labels.max())
    counts = label._label_sizes_dev(labels, n_labels)
    dist = torch.empty((T, N, N), dtype=torch.float64, device=dev)
    shrunk = torch.empty((T, N, N), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    report("  tf_subseg_prepare", lambda: _lib.check(L.tf_subseg_prepare(
        _lib.ptr(labels), _lib.ptr(d2), _lib.ptr(counts), n_labels, labels.numel(), SHRINK, _lib.ptr(dist), _lib.ptr(shrunk),
        _lib.stream_ptr()), "tf_subseg_prepare"))
    report("  peak_local_max_2d, all frames", lambda: [nd.peak_local_max_2d(dist[i], MIN_DISTANCE, 1e-8) for i in range(T)])
    rank = torch.empty((N, N), dtype=torch.float32, device=dev)

    def ranks():
        for i in range(T):
            keys = torch.unique(dist[i])
            _lib.check(L.tf_subseg_rank(_lib.ptr(dist[i]), N * N, _lib.ptr(keys), keys.numel(), _lib.ptr(rank), _lib.stream_ptr()), "tf_subseg_rank")
        out["keys"] = keys.numel()

    report("  torch.unique + tf_subseg_rank, all frames", ranks)
    print(f"  {out['keys']} distinct keys in the last frame", flush=True)

    try:
        import skimage
    except ImportError:
        print("scikit-image is not importable on this machine: no figure for the reference's subsegment_labels on its CPU", flush=True)
        return
    frame = mask[T // 2].cpu().numpy()
    t0 = time.perf_counter()
    reference_frame(frame, SHRINK, MIN_DISTANCE)
    print(f"the reference's recipe with scikit-image {skimage.__version__} on this machine's CPU, ONE {N}^2 frame (one run): "
          f"{time.perf_counter() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
