"""Time the field preparation (tf_stripe_deviation, tf_prepare_fields, tobac_flow_amd.dataloader) on a GOES-shaped stack of
T x N^2 voxels with four packed channels and four DQF planes, once warm:

  the three kernels from the library's own event brackets (tf_profile_collect: stripe_columns -- with the variance
  kernel in its bracket --, stripe_rows, prepare_fields), the fused kernel's algorithmic bytes per second beside the rate
  tf_copy16 reaches on 2 x 1 GiB (read + written bytes, as bench.py --full's practical_peak counts them);
  goes_fields end to end from HOST arrays, packed int16 and float32 input;
  the NumPy restatement of tests/fields_cases.py on this machine's CPU, on CPU_FRAMES frames of the same size.

Median of RUNS after WARM warm-ups.  Usage: python tools/field_prep_time.py [N] [T] [output file]
(development aid; the figures are kept in profiles/field_prep.txt)"""
import statistics
import sys
import time
from datetime import timedelta

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import torch

import fields_cases as fc
from tobac_flow_amd import _lib, dataloader

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
T = int(sys.argv[2]) if len(sys.argv) > 2 else 16
OUT = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
WARM, RUNS, CPU_FRAMES = 1, 3, 2


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(f, timer):
    for _ in range(WARM):
        f()
    return statistics.median(timer(f) for _ in range(RUNS))


def copy_rate():
    L = _lib.lib()
    n = 1 << 30
    src, dst = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), n, _lib.stream_ptr()), "tf_copy16")
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    once()
    return 2 * n / (statistics.median(once() for _ in range(5)) * 1e-3)


def stack():
    """frames that are shifted copies of one random frame: raw counts with 0.2 % fill, DQF with 0.4 % flags and a stripe"""
    rng = np.random.default_rng(5)
    raws, dqf = [], []
    for c in range(4):
        frame = rng.integers(900, 3600, (N, N)).astype(np.uint16)
        frame[rng.random((N, N)) < 0.002] = 65535
        raws.append(np.stack([np.roll(frame, 17 * k, 1) for k in range(T)]).view(np.int16))
        flags = np.where(rng.random((N, N)) < 0.004, 1, 0).astype(np.uint8)
        d = np.stack([np.roll(flags, 29 * k, 0) for k in range(T)])
        d[c % T, 100 + c, :] = 1
        dqf.append(d)
    t = np.datetime64("2018-06-19T17:00:00", "ns") + np.arange(T) * np.timedelta64(300, "s")
    return raws, dqf, t


def main():
    _lib.device()
    say(f"field preparation, {T} x {N}^2, four packed channels, four DQF planes; {torch.cuda.get_device_name(0)}; "
        f"median of {RUNS} after {WARM} warm-up")
    rate = copy_rate()
    say(f"tf_copy16 on 2 x 1 GiB: {rate / 1e12:.2f} TB/s (read + written bytes)")
    raws, dqf, t = stack()
    gap = timedelta(minutes=15)
    packed = [dataloader.PackedChannel(r, s, o, fill_value=fc.GOES_FILL, unsigned=True) for r, (s, o) in zip(raws, fc.GOES_PACKING)]

    # the kernels, operands on the device
    dev_packed = [dataloader.PackedChannel(_lib.to_dev(r), s, o, fill_value=fc.GOES_FILL, unsigned=True) for r, (s, o) in zip(raws, fc.GOES_PACKING)]
    dev_dqf = [_lib.to_dev(d) for d in dqf]
    run = lambda: dataloader.goes_fields(*dev_packed, t, dqf=dev_dqf, time_gap=gap)   # noqa: E731
    run()
    torch.cuda.synchronize()
    _lib.profile_collect()
    _lib.profile_enable(True)
    for _ in range(RUNS):
        run()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    for name in ("stripe_columns", "stripe_rows", "prepare_fields"):
        calls, ms, nbytes = prof[name]
        per = "per plane" if name.startswith("stripe") else "per call"
        say(f"  {name}: {ms / calls:.3f} ms {per} ({calls} launches), {nbytes / calls / 1e9:.2f} GB algorithmic, "
            f"{nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {nbytes / (ms * 1e-3) / rate:.2f} of the copy rate")
    say(f"  goes_fields, operands on the device, end to end: {median(run, wall):.1f} ms wall")
    del dev_packed, dev_dqf
    torch.cuda.empty_cache()

    # from host arrays
    say(f"  goes_fields from host arrays, packed int16 ({sum(r.nbytes for r in raws) / 1e9:.2f} GB + {sum(d.nbytes for d in dqf) / 1e9:.2f} GB DQF): "
        f"{median(lambda: dataloader.goes_fields(*packed, t, dqf=dqf, time_gap=gap), wall):.0f} ms wall")
    decoded = [fc.decode(r, s, o, 65535, unsigned=True) for r, (s, o) in zip(raws, fc.GOES_PACKING)]
    say(f"  goes_fields from host arrays, float32 ({sum(x.nbytes for x in decoded) / 1e9:.2f} GB + DQF): "
        f"{median(lambda: dataloader.goes_fields(*decoded, t, dqf=dqf, time_gap=gap), wall):.0f} ms wall")
    del decoded

    # the restatement on the CPU: decode, differences, masks, stripes
    k = min(CPU_FRAMES, T)

    def reference():
        dec = [fc.decode(r[:k], s, o, 65535, unsigned=True) for r, (s, o) in zip(raws, fc.GOES_PACKING)]
        return fc.prepare(dec, fc.GOES_RECIPES, t[:k], [fc.dqf_float(d[:k]) for d in dqf], gap)
    t0 = time.perf_counter()
    want = reference()[0]
    ms = (time.perf_counter() - t0) * 1e3
    say(f"  CPU: the NumPy restatement on {k} frames {ms:.0f} ms = {ms / k:.0f} ms per frame -> {T} frames {ms / k * T / 1e3:.1f} s")
    got = dataloader.goes_fields(*[dataloader.PackedChannel(p.raw[:k], p.scale_factor, p.add_offset, p.fill_value, True) for p in packed],
                                 t[:k], dqf=[d[:k] for d in dqf], time_gap=gap, on_device=False)
    say("  the device fields of those frames equal the restatement bit for bit:",
        all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)))


if __name__ == "__main__":
    main()
