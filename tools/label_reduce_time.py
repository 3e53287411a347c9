"""Time the generic per-label reductions (tf_label_reduce, tf_label_order and the device path of
utils.label_utils.labeled_comprehension) on a synthetic T x N^2 label volume: the flat labels of the cold blobs below
262 K of tools/synth.py (2.4 % of the voxels labelled at 16 x 5424^2), everything device-resident.

  figure 1  tf_label_reduce alone (HIP events): pass 1, and pass 1 + 2 (want = 1), for a float32 volume field, a float64
            volume field and a float32 (N, N) plane field, against the bytes the call must read -- 4 B per voxel of labels
            per pass plus the field under the labelled voxels' 16-byte pieces at most -- and as a fraction of the copy
            kernel's rate (tf_copy16 over buffers of the label volume's size) measured in the same run
  figure 2  tf_label_order alone (HIP events; the records come from a tf_label_reduce call outside the timing)
  figure 3  labeled_comprehension(bt, labels, np.nanmean) and (..., np.median) from device tensors: wall time with a
            device synchronise, index=None included (torch.unique of the labelled voxels)
  figure 4  the same two calls through the host code (SciPy's argsort of the volume and a Python call per label) on the
            CPU, on CPU_T frames of the same volume (default: all of them), and whether the device results equal its

Usage: python tools/label_reduce_time.py [N] [T] [CPU_T] (development aid; the figures are kept in
profiles/label_reduce.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import torch

from tobac_flow_amd import _lib, ndimage_dev as nd
from tobac_flow_amd.utils import label_utils as lu

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
CPU_T = int(sys.argv[3]) if len(sys.argv) > 3 else T
WARM, RUNS = 1, 5


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


def main():
    from synth import blob_stack
    L, dev = _lib.lib(), _lib.device()
    bt = torch.nan_to_num(blob_stack(T, N, N), nan=290.0)
    labels = nd.flat_label(bt < 262.0)
    labels = (labels[0] if isinstance(labels, tuple) else labels).to(torch.int32).contiguous()
    n_vox, top = labels.numel(), int(labels.max())
    share = float((labels != 0).float().mean())
    print(f"{T} x {N}^2 labels: {share * 100:.1f} % labelled, {top} labels", flush=True)

    # the practical ceiling: the library's copy kernel over two buffers of the label volume's size
    src = torch.zeros(n_vox, dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    med, lo, hi = median(lambda: _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), 4 * n_vox, _lib.stream_ptr()), "tf_copy16"), events)
    copy_rate = 8 * n_vox / 1e9 / med * 1e3
    print(f"copy kernel: {4 * n_vox / 1e9:.2f} GB read + written in median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {copy_rate:.0f} GB/s",
          flush=True)
    del src, dst

    rec = torch.empty((top, 8), dtype=torch.int64, device=dev)
    ws = torch.empty(L.tf_label_reduce_workspace_bytes(1, top), dtype=torch.uint8, device=dev)
    y, x = np.linspace(0.12, -0.12, N), np.linspace(-0.12, 0.12, N)
    area = torch.from_numpy((4.0 / np.cos(2.0 * y[:, None] + x[None]) ** 2).astype(np.float32)).to(dev)
    fields = (("float32 volume", bt, _lib.TF_F32, 0, 4), ("float64 volume", bt.double(), _lib.TF_F64, 0, 8),
              ("float32 plane", area, _lib.TF_F32, 1, 4))
    for what, f, code, layout, width in fields:
        for want in (0, 1):
            def run():
                _lib.check(L.tf_label_reduce(_lib.ptr(labels), _lib.ptr(f), code, layout, T, N * N, 1, top, want, _lib.ptr(rec),
                                             _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_reduce")

            med, lo, hi = median(run, events)
            passes = 1 + want
            gb = passes * 4 * n_vox / 1e9
            print(f"figure 1: tf_label_reduce {what}, {'pass 1 + 2' if want else 'pass 1'}: median {med:.3f} ms (min {lo:.3f}, max "
                  f"{hi:.3f}); the labels alone are {gb:.2f} GB = {gb / med * 1e3:.0f} GB/s = {gb / med * 1e3 / copy_rate * 100:.0f} % "
                  f"of the copy kernel's rate (the field adds at most {passes * width * share * n_vox / 1e9:.3f} GB under labelled "
                  f"voxels)", flush=True)
    del fields

    _lib.check(L.tf_label_reduce(_lib.ptr(labels), _lib.ptr(bt), _lib.TF_F32, 0, T, N * N, 1, top, 0, _lib.ptr(rec), None, 0,
                                 _lib.stream_ptr()), "tf_label_reduce")
    n_keys = int(rec[:, 1].sum())
    mid = torch.empty((top, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(L.tf_label_order_workspace_bytes(1, top, n_keys, _lib.TF_F32), dtype=torch.uint8, device=dev)

    def order():
        _lib.check(L.tf_label_order(_lib.ptr(labels), _lib.ptr(bt), _lib.TF_F32, 0, T, N * N, 1, top, _lib.ptr(rec), n_keys,
                                    _lib.ptr(mid), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_order")

    med, lo, hi = median(order, events)
    gb = 4 * n_vox / 1e9
    print(f"figure 2: tf_label_order float32 volume ({n_keys} keys, workspace {ws.numel() / 1e6:.0f} MB): median {med:.3f} ms (min "
          f"{lo:.3f}, max {hi:.3f}); one read of the labels = {gb / med * 1e3:.0f} GB/s = {gb / med * 1e3 / copy_rate * 100:.0f} % of "
          f"the copy kernel's rate", flush=True)
    del rec, mid, ws

    got = {}
    for name, func in (("np.nanmean", np.nanmean), ("np.median", np.median)):
        med, lo, hi = median(lambda: got.__setitem__(name, lu.labeled_comprehension(bt, labels, func, default=np.nan)), wall)
        print(f"figure 3: labeled_comprehension(bt, labels, {name}) from device tensors, index=None: median {med:.1f} ms (min "
              f"{lo:.1f}, max {hi:.1f})", flush=True)

    bt_h, labels_h = bt[:CPU_T].cpu().numpy(), labels[:CPU_T].cpu().numpy()
    ids = np.unique(labels_h[labels_h != 0])
    for name, func in (("np.nanmean", np.nanmean), ("np.median", np.median)):
        t0 = time.perf_counter()
        want = lu.labeled_comprehension(bt_h, labels_h, func, default=np.nan)
        t1 = time.perf_counter()
        print(f"figure 4: the host code on {CPU_T} of the {T} frames ({ids.size} labels), {name}, one run: {(t1 - t0) * 1e3:.0f} ms",
              flush=True)
        if CPU_T == T:
            print("figure 4: device result equal to the host's within 1e-6 relative:",
                  bool(np.allclose(got[name].cpu().numpy(), want, rtol=1e-6, equal_nan=True)), flush=True)


if __name__ == "__main__":
    main()
