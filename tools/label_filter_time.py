"""Time the label filter of the multichannel growth recipe on one GPU.

(a) tf_label_filter with the recipe's three criteria (w_s >= upper, b_s <= -upper, wvd > -5, three float32 fields) on a
    synthetic T x N^2 label volume (flat labels of the cold blobs below 262 K).  The raw entry point with the largest label
    known (no Python glue), and the Python form end to end.  (profiles/label_filter.txt also has the threshold passes and the
    one-mask-per-call entry point this kernel retired.)
(b) detect_growth_markers_multichannel device-resident (DeviceField in, tensors out) and on host arrays, against
    _detect_growth_markers_multichannel_host, on a T x H x W scene with a Farneback flow; then the device form stage by stage.
(c) the recipes that end in a label filter -- get_anvil_markers, detect_anvils, relabel_anvils, detect_growth_markers,
    detect_cores -- device-resident on the same T x H x W scene (profiles/label_extent_retired.txt).

Wall time around each call with a device synchronise; median of RUNS after WARM warm-ups.
Usage: python tools/label_filter_time.py [N] [T] [H] [W] [a|b|c|abc] (development aid; the figures are kept in profiles/label_filter.txt, those of part c in profiles/label_extent_retired.txt)"""
import statistics
import sys
import time
import warnings

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import torch

from tobac_flow_amd import _lib, ndimage_dev as nd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
H = int(sys.argv[3]) if len(sys.argv) > 3 else 1500
W = int(sys.argv[4]) if len(sys.argv) > 4 else 2500
UPPER = 0.5
WARM, RUNS = 1, 5
PARAMS = dict(min_length=2, lower_threshold=0.05, upper_threshold=0.1)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(name, f, runs=RUNS, warm=WARM):
    for _ in range(warm):
        f()
    ts = [wall(f) for _ in range(runs)]
    print(f"{name}: median {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}); {runs} runs after {warm} warm-up", flush=True)
    return statistics.median(ts)


def part_a():
    from synth import blob_stack
    L = _lib.lib()
    bt = torch.nan_to_num(blob_stack(T, N, N), nan=290.0)
    labels = nd.flat_label(bt < 262.0)
    n = int(labels.max())
    set_share = float((labels != 0).float().mean())
    wvd = (250.0 - bt) / 2.0 - 10.0
    del bt
    gen = torch.Generator(device="cuda").manual_seed(7)
    w_s = torch.randn((T, N, N), generator=gen, device="cuda", dtype=torch.float32) * 0.3
    b_s = torch.randn((T, N, N), generator=gen, device="cuda", dtype=torch.float32) * 0.3
    print(f"(a) {T} x {N}^2 labels: {set_share * 100:.1f} % set, {n} labels; criteria w_s >= {UPPER}, b_s <= {-UPPER}, wvd > -5 "
          f"(float32 fields)", flush=True)
    criteria = [(w_s, ">=", UPPER), (b_s, "<=", -UPPER), (wvd, ">", -5)]

    crit = (_lib.LabelCriterion * 3)()
    for k, (f, op, th) in enumerate(criteria):
        crit[k] = _lib.LabelCriterion(f.data_ptr(), _lib.TF_F32, _lib.CMP_OPS[op], th)
    rec = torch.empty((n + 1, 4), dtype=torch.int32, device="cuda")
    none = (_lib.LabelCriterion * 1)()
    fused = report("  tf_label_filter, three criteria", lambda: _lib.check(L.tf_label_filter(
        _lib.ptr(labels), T, N, N, n, crit, 3, _lib.ptr(rec), _lib.stream_ptr()), "tf_label_filter"))
    report("  tf_label_filter, no criterion (lengths only)", lambda: _lib.check(L.tf_label_filter(
        _lib.ptr(labels), T, N, N, n, none, 0, _lib.ptr(rec), _lib.stream_ptr()), "tf_label_filter"))

    voxels = T * N * N
    print(f"  bytes per voxel, algorithmic: 4 (labels) + 12 under the {set_share * 100:.1f} % labelled voxels at most = "
          f"{4 + 12 * set_share:.2f}: {voxels * (4 + 12 * set_share) / fused / 1e6:.0f} GB/s of that", flush=True)

    # the Python form end to end (finds the largest label on the device first and downloads the small result)
    _, hits, _ = nd.label_filter(labels, criteria)
    report("  ndimage_dev.label_filter(labels, three criteria)", lambda: nd.label_filter(labels, criteria))
    print(f"  {int(hits.all(1).sum())} of {n} labels satisfy all three criteria", flush=True)


def part_b():
    import scipy.ndimage as ndi
    import tobac_flow_amd.flow as tf
    from synth import blob_stack, field_with_time
    from tobac_flow_amd import detection as det
    from tobac_flow_amd.utils import get_time_diff_from_coord
    bt_d = torch.nan_to_num(blob_stack(T, H, W), nan=290.0)
    grow = torch.linspace(0.6, 1.4, T, device="cuda")[:, None, None]          # deepening cold tops, so that growth is detected
    bt_d = (290.0 - (290.0 - bt_d) * grow).contiguous()
    wvd_d = ((250.0 - bt_d) / 2.0 - 10.0).contiguous()
    bt_h, wvd_h = field_with_time(bt_d.cpu().numpy(), 5), field_with_time(wvd_d.cpu().numpy(), 5)
    flow = tf.create_flow(bt_h, vr_steps=1, smoothing_passes=1, interp_method="cubic")
    bt_f, wvd_f = field_with_time(bt_d, 5), field_with_time(wvd_d, 5)
    print(f"(b) detect_growth_markers_multichannel on {T} x {H} x {W}, {PARAMS}", flush=True)
    out = {}

    def run(fn, *fields):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["r"] = fn(flow, *fields, **PARAMS)
    dev = report("  device-resident (DeviceField in, tensors out)", lambda: run(det.detect_growth_markers_multichannel, wvd_f, bt_f), runs=3)
    dev_markers = out["r"][2].cpu().numpy()
    report("  host arrays in and out (upload, recipe in HBM, download)", lambda: run(det.detect_growth_markers_multichannel, wvd_h, bt_h), runs=3)
    assert np.array_equal(out["r"][2], dev_markers)
    host = report("  _detect_growth_markers_multichannel_host (SciPy glue)", lambda: run(det._detect_growth_markers_multichannel_host, wvd_h, bt_h),
                  runs=1, warm=0)
    same = np.array_equal(out["r"][2], dev_markers)
    print(f"  {int(dev_markers.max())} markers survive; device and host form agree: {same}; host / device = x{host / dev:.0f}", flush=True)

    # the device form stage by stage (the statements of detect_growth_markers_multichannel, one timer each)
    dt = torch.from_numpy(np.asarray(get_time_diff_from_coord(wvd_f.t))).cuda()[:, None, None]
    s = {}
    report("    rates and moving averages, both channels", lambda: s.update(
        w=det.filtered_tdiff(flow, flow.diff(wvd_d, method="linear") / dt), b=det.filtered_tdiff(flow, flow.diff(bt_d, method="linear") / dt)), runs=3)
    report("    two curvature filters", lambda: s.update(cw=det.get_curvature_filter(wvd_d), cb=det.get_curvature_filter(bt_d, direction="positive")), runs=3)
    lo, up = PARAMS["lower_threshold"], PARAMS["upper_threshold"]
    report("    marker mask (torch element-wise) and opening", lambda: s.update(
        m=nd.binary_opening(((s["w"] * s["cw"]) >= lo) | ((s["b"] * s["cb"]) <= -lo), det._plane_struct())), runs=3)
    report("    flow.label", lambda: s.update(l=flow.label(s["m"], overlap=0.5, subsegment_shrink=0)), runs=3)
    report("    count_nonzero + label_filter, three criteria", lambda: s.update(
        c=int(torch.count_nonzero(s["l"]).item()), f=nd.label_filter(s["l"], [(s["w"], ">=", up), (s["b"], "<=", -up), (wvd_d, ">", -5)])), runs=3)
    lengths, hits, _ = s["f"]
    report("    remap_labels", lambda: nd.remap_labels(s["l"], (lengths >= PARAMS["min_length"]) & hits.all(1)), runs=3)
    lab_h = s["l"].cpu().numpy()
    masks_h = [(s["w"] >= up).cpu().numpy(), (s["b"] <= -up).cpu().numpy(), (wvd_d > -5).cpu().numpy()]
    from tobac_flow_amd import analysis
    report("    host: filter_labels_by_length_and_multimask_legacy on the same labels (NumPy)",
           lambda: analysis.filter_labels_by_length_and_multimask_legacy(lab_h.copy(), masks_h, PARAMS["min_length"]), runs=1, warm=0)
    report("    host: ndi.binary_opening of the marker mask (SciPy)",
           lambda: ndi.binary_opening(s["m"].cpu().numpy() != 0, structure=ndi.generate_binary_structure(2, 1)[np.newaxis, ...]), runs=1, warm=0)


def part_c():
    import contextlib
    import io
    import tobac_flow_amd.flow as tf
    from synth import blob_stack, field_with_time
    from tobac_flow_amd import detection as det
    bt_d = torch.nan_to_num(blob_stack(T, H, W), nan=290.0)
    grow = torch.linspace(0.6, 1.4, T, device="cuda")[:, None, None]          # deepening cold tops, so that growth is detected
    cold = ((290.0 - bt_d) * grow).contiguous()
    bt_d = 290.0 - cold
    flow = tf.create_flow(field_with_time(bt_d.cpu().numpy(), 2), vr_steps=1, smoothing_passes=1, interp_method="cubic")
    bt_f, wvd_f = field_with_time(bt_d, 2), field_with_time((cold / 2.0 - 30.0).contiguous(), 2)
    swd_f = field_with_time((8 - (cold - 40.0).clamp(min=0) / 8).clamp(min=0).contiguous(), 2)     # small inside the cold tops
    print(f"(c) recipes, device-resident (DeviceField in, tensor out), on {T} x {H} x {W}", flush=True)
    out = {}

    def timed(name, fn, *args):
        def run():
            with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
                warnings.simplefilter("ignore")
                try:
                    out[name] = fn(flow, *args)
                except ValueError as e:                               # (a filter stage that leaves nothing: the reference's error)
                    out[name] = e
        report(f"  {name}", run, runs=3)
        r = out[name][1] if isinstance(out[name], tuple) else out[name]
        print(f"    -> {type(r).__name__ if isinstance(r, Exception) else int(r.max())} labels", flush=True)

    timed("get_anvil_markers", det.get_anvil_markers, wvd_f)
    timed("detect_anvils", lambda f, x: det.detect_anvils(f, x, markers=out["get_anvil_markers"]), wvd_f)
    timed("relabel_anvils", lambda f: det.relabel_anvils(f, out["detect_anvils"], markers=out["get_anvil_markers"]))
    timed("detect_growth_markers", det.detect_growth_markers, wvd_f)
    timed("detect_cores", det.detect_cores, bt_f, wvd_f, swd_f)


if __name__ == "__main__":
    which = sys.argv[5] if len(sys.argv) > 5 else "abc"
    if "a" in which:
        part_a()
        torch.cuda.empty_cache()
    if "b" in which:
        part_b()
        torch.cuda.empty_cache()
    if "c" in which:
        part_c()
