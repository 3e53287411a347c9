"""bench.py's own multi-rank path (reference: scripts/linking_parallel.py:26-27 -- windows of one
sequence processed by several workers, label ids linked afterwards): the driver starts `bench.py --gpus N` on an 8-GPU node
at round end, the builder's box has one GPU, so the launcher, the rank set-up (RANK / LOCAL_RANK / WORLD_SIZE), the
per-rank segment of the synthetic sequence and stitch_rank_windows over the ranks' windows are rehearsed here with two ranks
on ONE device over gloo -- as a fresh child process each, like the driver's call -- and compared with the one-process run of
the same 44-frame sequence."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*extra, reports=False, env_extra=None):
    """one bench.py run as a fresh child process; reports=True keeps what --full runs after the timed region (the CPU
    baseline, the raster sub-report), which the other calls switch off"""
    skip = [] if reports else ["--no-cpu-baseline", "--no-raster-subreport"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C", "--steps", "1", "--warmup", "0", "--rotate", "1", *skip, *extra]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, "bench.py %s failed:\n%s" % (" ".join(extra), r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line on rank 0, got %d" % len(lines)
    return json.loads(lines[0])


def test_two_ranks_on_one_device_equal_the_one_process_run():
    """rank r holds frames 20 r .. 20 r + 23 of one sequence (two 14-frame windows each, consecutive ranks share four frames);
    one process holding frames 0 .. 43 as four windows floods the same four windows: same objects after the stitch."""
    two = _bench("--gpus", "2", "--single-device", "--backend", "gloo")
    one = _bench("--frames", "44", "--n-windows", "4")
    assert two["n_gpus"] == 2 and two["rccl_world_size"] == 2 and one["n_gpus"] == 1
    assert two["config"]["frames_delivered_per_step"] == 24 and two["scaling"] == "weak"
    assert two["watershed"]["tie_order"] == "reference" and two["watershed"]["labels_bit_exact_with_the_reference_by_construction"]
    assert two["config"]["objects_after_stitch"] == one["config"]["objects_after_stitch"] > 10
    # whole-job value: both ranks' frames over the slower rank's time
    assert two["value"] > 0 and abs(two["value"] - 2 * 24 * 1500 * 2500 / (two["ms_per_step"] * 1e-3) / 1e6) < 0.02 * two["value"]
    # round 5: several timed steps are ONE detect_stack_sequence call (the end of a stack beside the next stack's flow); under
    # --gpus N the stitch of every stack is a collective issued from the flood threads of the ranks, in the same order
    two_p = _bench("--gpus", "2", "--single-device", "--backend", "gloo", "--steps", "2")
    one_p = _bench("--frames", "44", "--n-windows", "4", "--steps", "2")
    assert two_p["steps_pipelined"]["on"] and one_p["steps_pipelined"]["on"] and not two["steps_pipelined"]["on"]
    n_obj = one["config"]["objects_after_stitch"]
    assert two_p["config"]["objects_after_stitch_per_step"] == [n_obj, n_obj] == one_p["config"]["objects_after_stitch_per_step"]
    assert len(two_p["step_ms"]) == 2 and two_p["n_gpus"] == 2


def test_strong_sharding_of_one_stack_equals_the_one_process_run():
    """bench.py --scaling strong (BASELINE configs 4 - 5 as worded: ONE stack "frame-sharded" over the GPUs; the reference's
    analogue: one window job per process, scripts/dcc_detect_seviri_nat.py:152 + scripts/linking_parallel.py:26-27): a 44-frame
    stack of four windows, rank r taking two of them and the 24 frames they cover -- the same objects after the stitch as the
    one-process run of the same stack, `value` = the ONE stack's pixels over the wall time (not times N), and N = 1 under
    --scaling strong is the plain run."""
    one = _bench("--frames", "44", "--n-windows", "4")
    two = _bench("--frames", "44", "--n-windows", "4", "--gpus", "2", "--single-device", "--backend", "gloo", "--scaling", "strong")
    solo = _bench("--frames", "44", "--n-windows", "4", "--scaling", "strong")
    assert two["scaling"] == "strong" and two["n_gpus"] == 2 and solo["scaling"] == "strong" and one["scaling"] == "weak"
    assert two["config"]["frames_delivered_per_step"] == 44 == solo["config"]["frames_delivered_per_step"]
    assert two["config"]["objects_after_stitch"] == one["config"]["objects_after_stitch"] == solo["config"]["objects_after_stitch"] > 10
    assert abs(two["value"] - 44 * 1500 * 2500 / (two["ms_per_step"] * 1e-3) / 1e6) < 0.02 * two["value"]
    assert "STRONG" in two["config"]["sharding"] and "ONE 44x1500x2500" in two["config"]["workload"]
    # two steps: every rank's share of the stack goes through detect_stack_sequence, the stitch of each step a collective
    two_p = _bench("--frames", "44", "--n-windows", "4", "--gpus", "2", "--single-device", "--backend", "gloo", "--scaling", "strong", "--steps", "2")
    n_obj = one["config"]["objects_after_stitch"]
    assert two_p["config"]["objects_after_stitch_per_step"] == [n_obj, n_obj] and two_p["steps_pipelined"]["on"]


def test_bench_pipeline_equals_the_plain_calls():
    """bench.py's step -- windows begun from create_flow's callback while the later frames' flow is computed, floods in parts
    with their replays on worker threads, finished on a second stream, stitched in place -- against the same stack processed
    with the plain calls one after the other (create_flow, Flow.window, seeds, edge field, Flow.watershed, stitch_window_list):
    the same number of objects after the stitch, for the streaming and the non-streaming schedule."""
    import numpy as np
    import torch
    import tobac_flow_amd.flow as tf
    from tobac_flow_amd.detection import get_combined_edge_field
    from tobac_flow_amd.parallel import stitch_window_list, window_bounds
    from tools.synth import anvil_seeds, blob_stack
    T, H, W, n_win, overlap = 44, 1500, 2500, 4, 4
    bt = blob_stack(T, H, W, seed=20240601, t0=0)
    flow = tf.create_flow(bt, model="Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")
    labs = []
    for a, b in window_bounds(T, n_win, overlap):
        fl = flow.window(a, b)
        lin, seeds = anvil_seeds(bt[a:b])
        e = get_combined_edge_field(fl, lin, dtype=np.float32)
        labs.append(fl.watershed(e, seeds, connectivity=1))
    want = int(max(int(w.max()) for w in stitch_window_list(labs, overlap=overlap)))
    del flow, labs
    torch.cuda.empty_cache()
    streamed = _bench("--frames", "44", "--n-windows", "4")
    plain = _bench("--frames", "44", "--n-windows", "4", "--no-stream-windows")
    assert streamed["watershed"]["windows_begun_during_the_flow"] and not plain["watershed"]["windows_begun_during_the_flow"]
    assert streamed["config"]["objects_after_stitch"] == plain["config"]["objects_after_stitch"] == want > 10


def test_bench_dump_outputs_writes_the_last_steps_labels(tmp_path):
    """--dump-outputs DIR: the label ids the last timed step delivered, one float64 file per window.  Under --rotate 1 every
    step floods the same stack, so one plain step and two pipelined steps (detect_stack_sequence) write the same files; with
    three channels, the windows handed out with window-local ids and mapped by their tables write what the stitched windows do."""
    import numpy as np
    one = _bench("--frames", "44", "--n-windows", "4", "--dump-outputs", str(tmp_path / "one"))
    two = _bench("--frames", "44", "--n-windows", "4", "--steps", "2", "--dump-outputs", str(tmp_path / "two"))
    assert not one["steps_pipelined"]["on"] and two["steps_pipelined"]["on"] and two["steps"] == 2 and len(two["step_ms"]) == 2
    files = ["labels_w%02d.npy" % k for k in range(4)]
    assert one["outputs_dumped"]["files"] == two["outputs_dumped"]["files"] == files
    assert 0 < one["outputs_dumped"]["bytes"] <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f)
        assert a.dtype == np.float64 and (a > 0).any() and np.array_equal(a, b), f
    f3 = ("--config", "F3", "--frames", "14", "--n-windows", "2", "--height", "1500", "--width", "2500")
    handed = _bench(*f3, "--dump-outputs", str(tmp_path / "handed"))
    kept = _bench(*f3, "--no-hand-out", "--dump-outputs", str(tmp_path / "kept"))
    assert "handed out" in handed["config"]["delivery"] and "resident" in kept["config"]["delivery"]
    assert handed["outputs_dumped"]["files"] == kept["outputs_dumped"]["files"] == files[:2]
    for f in files[:2]:
        a, b = np.load(tmp_path / "handed" / f), np.load(tmp_path / "kept" / f)
        assert (a > 0).any() and np.array_equal(a, b), f


def test_bench_full_adds_the_untimed_reports_a_plain_run_leaves_out():
    """A plain run does only what its headline figure needs: set-up, warm-up, the timed steps, the line.  --full adds, after
    the timed region, one stack by itself, one step in raster tie order, the copy kernel's HBM ceiling, the CPU baseline with
    the library checked against the oracle on its sample (three frames here, TF_BENCH_CPU_FRAMES) and the OpenCV probe; the
    timed steps are the same ones."""
    args = ("--frames", "44", "--n-windows", "4", "--steps", "2")
    plain = _bench(*args, reports=True)
    full = _bench(*args, "--full", reports=True, env_extra={"TF_BENCH_CPU_FRAMES": "3"})
    assert plain["steps_pipelined"]["on"] and full["steps_pipelined"]["on"]
    assert plain["one_stack_by_itself_ms"] is None and "raster_order_subreport" not in plain["watershed"]
    assert "practical_peak" not in plain["roofline"] and "cpu_baseline" not in plain and "cv2_parity" not in plain
    assert plain["roofline"]["all_kernels"] and plain["ms_per_step"] > 0
    assert full["one_stack_by_itself_ms"] > 0 and full["watershed"]["raster_order_subreport"]["ms_per_step"] > 0
    assert full["roofline"]["practical_peak"] > 0 and full["roofline"]["frac_practical"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["library_vs_oracle_on_the_sample"] == {
        "flow_bit_identical": True, "edge_field_bit_identical": True, "labels_bit_identical": True}
    assert "status" in full["cv2_parity"]
    assert full["config"]["objects_after_stitch_per_step"] == plain["config"]["objects_after_stitch_per_step"]
