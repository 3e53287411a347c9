"""Time the third stage on one GPU.

(a) one 16-operation tf_group_reduce call (the operations of process_core_properties) on tables of 10^6 records / 10^5
    groups and 10^7 / 10^6 in record order by time, group lengths geometric with mean 10 and eight runs of 2 000 to 4 000;
    the same call with an empty operation table (rank + sort + bounds), the walk as the difference; the bytes the call
    must move, and tf_copy16 over that many bytes in the same run.  Device events, median (min .. max).
(b) postprocess.process_core_properties on the 10^6-record table, device-resident (host clock to a synchronise) and on
    NumPy columns (one run).

Usage: python tools/group_reduce_time.py [output file] (development aid; figures in profiles/group_reduce.txt)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tobac_flow_amd import _groups, _lib, postprocess  # noqa: E402
from tobac_flow_amd.dataset import LabelDataset  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def lengths_mix(rng, n_groups, n_records):
    """about ten records per object, geometric, with a few objects of some thousand records"""
    lengths = rng.geometric(1.0 / (n_records / n_groups - 1.0), n_groups).astype(np.int64) + 1
    lengths[rng.choice(n_groups, 8, replace=False)] = rng.integers(2000, 4000, 8)
    lengths[-1] += n_records - lengths.sum() if lengths.sum() < n_records else 0
    while lengths.sum() > n_records:
        big = np.flatnonzero(lengths > 2)
        cut = rng.choice(big, min(big.size, int(lengths.sum() - n_records)), replace=False)
        lengths[cut] -= 1
    return lengths


def table(rng, n_groups, n_records):
    lengths = lengths_mix(rng, n_groups, n_records)
    owner = np.repeat(np.arange(n_groups), lengths)
    frame = np.concatenate([s + np.arange(m) for s, m in zip(rng.integers(0, 200, n_groups), lengths)])
    order = np.lexsort((owner, frame))
    owner, frame = owner[order], frame[order]
    n = owner.size
    c = {"ids": (owner + 1).astype(np.int32), "coord": np.arange(1, n_groups + 1, dtype=np.int32),
         "t": frame.astype(np.int64) * 300 * 10 ** 9, "area": rng.uniform(10, 500, n), "lengths": lengths}
    for name in ("x", "y", "lat", "lon", "bt_mean", "bt_std", "bt_min", "bt_max", "bt_mean_uncertainty", "bt_mean_combined_error",
                 "bt_min_error", "bt_max_error"):
        c[name] = rng.normal(250, 20, n)
    return c


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        samples.append(start.elapsed_time(stop))
    return float(np.median(samples)), float(np.min(samples)), float(np.max(samples))


def main():
    rng = np.random.default_rng(3)
    L = _lib.lib()
    say(f"device: {torch.cuda.get_device_name(0)}; tf_version {L.tf_version()}; median (min .. max) of repeated calls, device events")
    for n_records, n_groups in ((10 ** 6, 10 ** 5), (10 ** 7, 10 ** 6)):
        c = table(rng, n_groups, n_records)
        n = c["ids"].size
        say()
        say(f"== {n} records, {n_groups} groups; lengths mean {c['lengths'].mean():.1f}, median {int(np.median(c['lengths']))}, "
            f"max {int(c['lengths'].max())}")
        d = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "lengths"}
        ops = [("PICK_ARGMIN", d["t"]), ("PICK_ARGMAX", d["t"]), ("WEIGHTED_AVERAGE", d["x"], d["area"]), ("WEIGHTED_AVERAGE", d["y"], d["area"]),
               ("WEIGHTED_AVERAGE", d["lat"], d["area"]), ("WEIGHTED_AVERAGE", d["lon"], d["area"]), ("MEAN", d["area"]), ("SUM", d["area"]),
               ("MAX", d["area"]), ("PICK_ARGMAX", d["area"]), ("PICK_IDXMAX", d["area"]), ("PICK_ARGMIN", d["bt_mean"]),
               ("PICK_IDXMIN", d["bt_mean"]), ("GRADIENT_MIN", d["bt_mean"], None, d["t"]), ("COMBINED_MEAN", d["bt_mean"], d["area"]),
               ("COMBINED_STD", d["bt_std"], d["area"], d["bt_mean"])]
        ops = [(tuple(op) + (None, None, None))[:4] for op in ops]
        outs = [torch.empty(n_groups, dtype=torch.int64 if op[0].startswith("PICK") else torch.float64, device="cuda") for op in ops]
        status = torch.zeros(2, dtype=torch.int64, device="cuda")
        repeats = 20 if n_records <= 10 ** 6 else 8
        whole = timed(lambda: _groups.group_reduce_call(d["ids"], d["coord"], ops, outs, status), repeats)
        grouping = timed(lambda: _groups.group_reduce_call(d["ids"], d["coord"], [], [], status), repeats)
        assert status.tolist() == [0, 0]
        # what one call must read and write: ids, every operand of every operation once per operation, the outputs
        operand_bytes = sum(col.numel() * col.element_size() for op in ops for col in op[1:] if col is not None)
        distinct = {col.data_ptr(): col.numel() * col.element_size() for op in ops for col in op[1:] if col is not None}
        must = d["ids"].numel() * 4 + sum(distinct.values()) + 16 * n_groups * 8
        src = torch.empty(must, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copy = timed(lambda: _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), must, _lib.stream_ptr()), "tf_copy16"), repeats)
        say(f"one 16-op tf_group_reduce call        {whole[0]:9.3f} ms ({whole[1]:.3f} .. {whole[2]:.3f})")
        say(f"  rank + sort + bounds (0 operations) {grouping[0]:9.3f} ms ({grouping[1]:.3f} .. {grouping[2]:.3f})")
        say(f"  walk (difference of the medians)    {whole[0] - grouping[0]:9.3f} ms")
        say(f"bytes it must move (ids, each distinct column once, outputs): {must / 1e6:.1f} MB; operand reads as issued "
            f"(a column once per operation that takes it): {operand_bytes / 1e6:.1f} MB")
        say(f"tf_copy16 of {must / 1e6:.1f} MB (reads and writes that many)     {copy[0]:9.3f} ms ({copy[1]:.3f} .. {copy[2]:.3f})"
            f" -> the call costs {whole[0] / copy[0]:.1f} such copies")
        del src, dst

        if n_records > 10 ** 6:
            continue

        def dataset(cols, convert):
            ds = LabelDataset(coords={"core": c["coord"], "core_step": np.arange(1, n + 1, dtype=np.int32)})
            ds.add("core_step_core_index", convert(cols["ids"]), ("core_step",))
            for name in cols:
                if name not in ("ids", "coord", "lengths"):
                    ds.add(f"core_step_{name}", convert(cols[name]), ("core_step",))
            return ds

        def on_device():
            postprocess.process_core_properties(dataset(d, lambda x: x))

        on_device()
        torch.cuda.synchronize()
        samples = []
        for _ in range(5):
            t0 = time.perf_counter()
            on_device()
            torch.cuda.synchronize()
            samples.append((time.perf_counter() - t0) * 1e3)
        say(f"process_core_properties, device-resident table, host clock to synchronise: median {np.median(samples):.1f} ms "
            f"({min(samples):.1f} .. {max(samples):.1f})")
        t0 = time.perf_counter()
        postprocess.process_core_properties(dataset(c, lambda x: x))
        say(f"process_core_properties, the package's NumPy path on the same table, same machine: {(time.perf_counter() - t0) * 1e3:.0f} ms (one run)")


if __name__ == "__main__":
    main()
