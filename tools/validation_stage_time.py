"""Time the validation stage on a synthetic detection product (T x N^2 device-resident label volumes: cold blobs
thresholded at three levels and labelled -- cores, thick anvils, anvil markers -- with core_anvil_index from
dataset.link_cores_and_anvils; a sparse float64 flash grid, most flashes near the cores), five marker sets, get_closest off
and on:

  * validate_detection, the stage as it is now;
  * the composition it replaces, kept here as `parent_stage`: the host get_edge_filter, then per marker set the full
    cylinder volumes and torch.repeat_interleave over every voxel (the body validate_markers had before the flash list),
    with the same device remaps for the two subsets -- in the same process on the same inputs, results compared;
  * one marker set alone, before and after, with the peak device memory it adds;
  * get_edge_filter_dev without and with a missing frame; tf_flash_count + tf_flash_list, tf_edt_cylinder_at and
    tf_edge_filter on their own;
  * the host get_edge_filter (SciPy's binary_dilation) with a missing frame, on the largest T x n^2 sub-volume that its time
    on a small one predicts to finish in about SCIPY_SECONDS (0 skips it).

Wall time around each call with a device synchronise, median of RUNS after WARM warm-ups (2 runs for the calls that go
through the host); HIP events around the kernels alone, median of KERNEL_RUNS after KERNEL_WARM.
Usage: python tools/validation_stage_time.py [N] [T] [SCIPY_SECONDS]  (development aid; the figures are kept in
profiles/validation_stage.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import numpy as np
import torch

from tobac_flow_amd import _lib, dataset, ndimage_dev as nd, validation as v

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
SCIPY_SECONDS = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
MARGIN, TIME_MARGIN = 10, 3                                       # the defaults of scripts/dcc_validation.py
WARM, RUNS = 1, 3                                                 # of the calls; the kernels alone: KERNEL_RUNS after KERNEL_WARM
KERNEL_WARM, KERNEL_RUNS = 3, 20


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


def report(name, f, timer=wall, warm=None, runs=None):
    warm = (KERNEL_WARM if timer is events else WARM) if warm is None else warm
    runs = (KERNEL_RUNS if timer is events else RUNS) if runs is None else runs
    for _ in range(warm):
        f()
    ts = [timer(f) for _ in range(runs)]
    med = statistics.median(ts)
    print(f"{name}: median {med:.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}); {runs} runs after {warm} warm-up", flush=True)
    return med


def peak_of(f):
    """MB of device memory the call adds at its peak to what is allocated when it starts"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


# ---- the composition before the flash list -------------------------------------------------------------------------------
def parent_validate_markers(labels, glm_grid, glm_distance, edge_filter, n_glm_in_margin, coord, margin, time_margin, get_closest):
    """validate_markers as it was: the cylinder volumes, then repeat_interleave over every voxel"""
    ids = v._label_ids(labels, coord)
    dist, closest = v._cylinder(labels, time_margin, bool(get_closest))
    if bool(((glm_grid < 0) | (glm_grid != glm_grid)).any()):
        raise ValueError("repeats may not contain negative values")
    repeats = glm_grid.to(torch.int64).reshape(-1)
    flash_distance = torch.repeat_interleave(dist.reshape(-1), repeats)
    flash_closest = torch.repeat_interleave(closest.reshape(-1), repeats) if get_closest else None
    pod = float((flash_distance <= margin).sum()) / n_glm_in_margin if n_glm_in_margin > 0 else np.nan
    inside, missing = v._label_nanmin(labels, edge_filter, ids)
    margin_flag = (inside != 0) & ~missing
    marker_distance = v._label_nanmin(labels, glm_distance, ids)[0]
    n_in = int(margin_flag.sum())
    far = float((marker_distance[margin_flag] > margin).sum()) / n_in if n_in > 0 else np.nan
    return flash_distance, flash_closest, marker_distance, pod, far, n_in, margin_flag


def marker_sets(ds):
    core, anvil, index = (np.asarray(ds.coords["core"]), np.asarray(ds.coords["anvil"]), np.asarray(ds["core_anvil_index"]))
    with_anvil = core[index != 0]
    with_core = anvil[np.isin(anvil, np.unique(index))]
    return (("core", lambda: ds["core_label"], core),
            ("core_with_anvil", lambda: v._keep_labels(ds["core_label"], with_anvil, int(core.max())), with_anvil),
            ("anvil", lambda: ds["thick_anvil_label"], anvil),
            ("anvil_with_core", lambda: v._keep_labels(ds["thick_anvil_label"], with_core, int(anvil.max())), with_core),
            ("anvil_marker", lambda: ds["anvil_marker_label"], np.asarray(ds.coords["anvil_marker"])))


def parent_sets(ds, grid, glm_distance, edge, n_in, get_closest):
    return {name: parent_validate_markers(labels(), grid, glm_distance, edge, n_in, coord, MARGIN, TIME_MARGIN, get_closest)
            for name, labels, coord in marker_sets(ds)}


def parent_stage(ds, flash_ds, get_closest):
    ds = v._cut_to_present(ds)                                    # the script's own step, before and now
    grid = flash_ds["glm_flashes"]
    glm_distance = v.get_marker_distance_cylinder(grid, TIME_MARGIN)
    edge = _lib.to_dev(v.get_edge_filter(flash_ds, MARGIN, TIME_MARGIN)).to(torch.bool)
    grid = torch.where(edge, grid, 0.0)
    return parent_sets(ds, grid, glm_distance, edge, float(torch.nansum(grid)), get_closest)


def main():
    from synth import blob_stack
    dev = _lib.device()
    bt = torch.nan_to_num(blob_stack(T, N, N), nan=290.0)
    ds = dataset.LabelDataset()
    for name, level in (("core_label", 245.0), ("anvil_marker_label", 252.0), ("thick_anvil_label", 262.0)):
        ds.add(name, nd.label(bt < level)[0], ("t", "y", "x"))
    ds.add("thin_anvil_label", ds["thick_anvil_label"], ("t", "y", "x"))
    del bt
    dataset.add_label_coords(ds)
    dataset.link_cores_and_anvils(ds, add_cores_to_anvils=False)
    ds.coords["anvil_marker"] = dataset._present_ids(ds["anvil_marker_label"])
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    near = nd.edt_squared_frames(ds["core_label"])[0] < 40 * 40     # flashes fall near the cores, most of them
    chance = torch.rand((T, N, N), generator=gen, device=dev)
    grid = ((chance < 2e-4) & near) | (chance < 5e-6)
    grid = (grid * torch.randint(1, 4, (T, N, N), generator=gen, device=dev)).to(torch.float64)
    del near, chance
    times = np.datetime64("2018-06-19T17:00:00", "ns") + (300 * np.arange(T)).astype("timedelta64[s]").astype("timedelta64[ns]")
    flash_ds = {"glm_flashes": grid, "t": times}
    print(f"{T} x {N}^2, margin {MARGIN}, time margin {TIME_MARGIN}: {ds.coords['core'].size} cores "
          f"({int((ds['core_anvil_index'] != 0).sum())} with an anvil), {ds.coords['anvil'].size} anvils, {ds.coords['anvil_marker'].size} "
          f"anvil markers; {int(grid.sum())} flashes in {int((grid != 0).sum())} voxels", flush=True)

    # ---- the stage, now and before ------------------------------------------------------------------------------------
    out = {}
    for get_closest in (False, True):
        def now():
            out["now"] = v.validate_detection(ds, flash_ds, MARGIN, TIME_MARGIN, get_closest=get_closest)

        def before():
            out["before"] = parent_stage(ds, flash_ds, get_closest)

        a = report(f"validate_detection, five sets, get_closest={get_closest}", now)
        b = report(f"the composition it replaces (host get_edge_filter, volumes + repeat_interleave), get_closest={get_closest}", before, runs=2)
        print(f"  = {b / a:.1f} x", flush=True)
        for name, result in out["before"].items():                # the same numbers, as float32 / int32 where the wrappers store them
            new = out["now"]
            assert torch.equal(new[f"flash_{name}_distance"], result[0].float()), name
            assert not get_closest or torch.equal(new[f"flash_{name}_index"], result[1].int()), name
            assert torch.allclose(new[f"{name}_glm_distance"], result[2].float(), rtol=0, atol=0, equal_nan=True), name
            assert torch.equal(new[f"{name}_margin_flag"], result[6]), name
            assert np.array_equal(new[f"{name}_pod"], np.float32(result[3]), equal_nan=True) and new[f"{name}_count_in_margin"] == result[5]
        print("  results equal: flash and marker distances, closest labels, flags, POD and counts of all five sets; POD / FAR: " +
              ", ".join(f"{n} {float(out['now'][n + '_pod']):.3f} / {float(out['now'][n + '_far']):.3f}" for n, _, _ in marker_sets(ds)), flush=True)

    # ---- the parts ----------------------------------------------------------------------------------------------------
    glm_distance = v.get_marker_distance_cylinder(grid, TIME_MARGIN)
    report("get_edge_filter (host NumPy, no missing data: download, NumPy, upload)",
           lambda: _lib.to_dev(v.get_edge_filter(flash_ds, MARGIN, TIME_MARGIN)), runs=2)
    report("get_edge_filter_dev, no missing data", lambda: v.get_edge_filter_dev(flash_ds, MARGIN, TIME_MARGIN), warm=2, runs=10)
    edge = v.get_edge_filter_dev(flash_ds, MARGIN, TIME_MARGIN)
    inside = torch.where(edge, grid, 0.0)
    n_in = float(inside.sum())
    for get_closest in (False, True):
        sets = {name: (labels(), coord) for name, labels, coord in marker_sets(ds)}
        flashes = v.flash_list(inside)
        for name in ("core", "anvil"):
            labels, coord = sets[name]
            new = lambda: v.validate_markers(labels, inside, glm_distance, edge, n_in, coord=coord, margin=MARGIN,     # noqa: E731
                                             time_margin=TIME_MARGIN, get_closest=get_closest, flashes=flashes)
            old = lambda: parent_validate_markers(labels, inside, glm_distance, edge, n_in, coord, MARGIN, TIME_MARGIN, get_closest)   # noqa: E731
            a = report(f"one set ({name}), shared flash list, get_closest={get_closest}", new)
            b = report(f"one set ({name}) as before, get_closest={get_closest}", old)
            print(f"  = {b / a:.2f} x; peak device memory added by the call: {peak_of(new):.0f} MB now, {peak_of(old):.0f} MB before", flush=True)
        del sets
    report("flash_list (tf_flash_count, the host reads the total, tf_flash_list)", lambda: v.flash_list(inside), warm=2, runs=10)
    labels = ds["core_label"]
    d2, nearest = nd.edt_squared_frames(labels, return_nearest=True)
    voxel = v.flash_list(inside).voxel
    report("tf_edt_cylinder_at alone, distances only", lambda: nd.edt_cylinder_at(d2, None, None, TIME_MARGIN, voxel, MARGIN), events)
    report("tf_edt_cylinder_at alone, distances and closest labels",
           lambda: nd.edt_cylinder_at(d2, nearest, labels, TIME_MARGIN, voxel, MARGIN, get_closest=True), events)
    report("tf_edt_cylinder alone (the volumes it replaces), distances and sources", lambda: nd.edt_cylinder(d2, nearest, TIME_MARGIN), events)
    del d2, nearest
    L = _lib.lib()
    mask = torch.empty((T, N, N), dtype=torch.uint8, device=dev)
    flag = torch.empty((), dtype=torch.int32, device=dev)
    report("tf_grid_has_missing alone (one read of the grid)",
           lambda: _lib.check(L.tf_grid_has_missing(_lib.ptr(grid), _lib.TF_F64, grid.numel(), _lib.ptr(flag), _lib.stream_ptr()), "scan"), events)
    report("tf_edge_filter alone, no missing data (the mask is written, the grid is not read)",
           lambda: _lib.check(L.tf_edge_filter(_lib.ptr(grid), _lib.TF_F64, T, N, N, MARGIN, TIME_MARGIN, None, 0, _lib.ptr(mask), None, 0,
                                               _lib.stream_ptr()), "tf_edge_filter"), events)
    missing = grid.clone()
    missing[T // 2] = -1                                          # regrid_glm writes -1 where no file covers a frame
    ws = torch.empty(L.tf_edge_filter_workspace_bytes(T, N, N, 1), dtype=torch.uint8, device=dev)
    report(f"tf_edge_filter alone, one missing frame (window OR, row counts, span lookups; workspace {ws.numel() / 1e6:.0f} MB)",
           lambda: _lib.check(L.tf_edge_filter(_lib.ptr(missing), _lib.TF_F64, T, N, N, MARGIN, TIME_MARGIN, None, 1, _lib.ptr(mask),
                                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_edge_filter"), events)
    del ws
    report("get_edge_filter_dev, one missing frame", lambda: v.get_edge_filter_dev({"glm_flashes": missing, "t": times}, MARGIN, TIME_MARGIN), warm=2, runs=10)
    few = grid.clone()
    few[T // 2, N // 2, N // 3], few[1, 5, 5] = -1, -1
    report("get_edge_filter_dev, two missing voxels", lambda: v.get_edge_filter_dev({"glm_flashes": few, "t": times}, MARGIN, TIME_MARGIN), warm=2, runs=10)
    del few

    if SCIPY_SECONDS > 0:
        host = missing.cpu().numpy()
        n, seconds = min(256, N), None
        while True:
            sub = {"glm_flashes": np.ascontiguousarray(host[:, :n, :n]), "t": times}
            t0 = time.perf_counter()
            want = v.get_edge_filter(sub, MARGIN, TIME_MARGIN)
            seconds = time.perf_counter() - t0
            got = v.get_edge_filter_dev(sub, MARGIN, TIME_MARGIN)
            assert np.array_equal(got.cpu().numpy(), want)
            print(f"get_edge_filter on this machine's CPU (SciPy's binary_dilation), one missing frame, {T} x {n}^2 (one run): "
                  f"{seconds:.1f} s = {seconds / (T * n * n) * 1e9:.0f} ns per voxel; the device result is equal", flush=True)
            more = min(N, int(n * (SCIPY_SECONDS / seconds) ** 0.5))
            if more <= n or n > 256:
                break
            n = more
        if n < N:
            print(f"  ({T} x {N}^2 has {(N / n) ** 2:.0f} x as many voxels as the {T} x {n}^2 sub-volume; it was not run on the CPU)", flush=True)


if __name__ == "__main__":
    main()
