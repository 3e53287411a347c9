"""Time the normalisation of one frame pair per method (normalise_pair_dev / tf_norm8_pair) at 1500 x 2500 and 5424 x 5424.

  device  HIP events around the call, REPS repetitions after WARM warm-up calls: median, minimum and maximum in ms, and
          the rate against the bytes the method's passes must move per pixel pair (the table in csrc/norm_methods.hip)
  host    the host glue that calculate_flow used for a device tensor before the device forms existed, and still uses for
          host containers: download both frames, the numpy / SciPy method, to_8bit, upload the bytes -- end to end with a
          device synchronise, HOST_REPS repetitions

Usage: python tools/norm_time.py [all|device|host] (development aid; the figures are kept in profiles/norm_methods.txt)"""
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from tobac_flow_amd import _lib
from tobac_flow_amd.utils import normalisation_utils as nu

MODE = sys.argv[1] if len(sys.argv) > 1 else "all"
SIZES = ((1500, 2500), (5424, 5424))
WARM, REPS, HOST_REPS = 3, 20, 3
METHODS = (("linear", {}), ("linear", {"vmin": 200, "vmax": 300}), ("log", {}), ("inverse_log", {}), ("z_score", {}),
           ("uniform", {}), ("local_linear", {}))
# bytes per pixel pair: reduction 8; map 8 + 2; z_score one more reduction; uniform three histogram reads; local_linear the row
# filter (8 + 8), the column suffix pass (8 + 8) and the column prefix pass with the map (16 + 8 + 2)
BYTES = {"linear": 18, "log": 18, "inverse_log": 18, "z_score": 26, "uniform": 42, "local_linear": 66}


def pair(H, W):
    """a brightness-temperature-like pair: a few cold blobs on a warm gradient, the second frame shifted"""
    dev = _lib.device()
    y = torch.linspace(0, 1, H, device=dev)[:, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :]
    f = 290 - 10 * y - 5 * x
    for cy, cx, r, d in ((0.3, 0.4, 0.08, 70), (0.7, 0.6, 0.15, 50), (0.5, 0.2, 0.05, 80), (0.2, 0.8, 0.1, 40)):
        f = f - d * torch.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    f = (f + torch.rand((H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(1))).float().contiguous()
    return f, torch.roll(f, (3, -5), (0, 1)).contiguous()


def device_ms(method, kw, fa, fb, out):
    for _ in range(WARM):
        nu.normalise_pair_dev(method, fa, fb, out=out, check_finite=False, **kw)
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nu.normalise_pair_dev(method, fa, fb, out=out, check_finite=False, **kw)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def host_glue_ms(method, kw, fa, fb, out):
    func = nu.select_normalisation_method(method)
    ms = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = np.stack([fa.cpu().numpy(), fb.cpu().numpy()], 0)
        p8 = nu.to_8bit(func(p, **kw), 0, 1)
        out[0].copy_(_lib.to_dev(p8[0]))
        out[1].copy_(_lib.to_dev(p8[1]))
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


for H, W in SIZES:
    fa, fb = pair(H, W)
    out = (_lib.empty((H, W), torch.uint8), _lib.empty((H, W), torch.uint8))
    n = H * W
    for method, kw in METHODS:
        what = f"{H} x {W} {method}{' ' + str(kw) if kw else ''}"
        if MODE in ("all", "device"):
            ms = device_ms(method, kw, fa, fb, out)
            med = statistics.median(ms)
            print(f"device {what}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} runs), "
                  f"{BYTES[method]} B per pixel pair -> {BYTES[method] * n / med / 1e6:.0f} GB/s", flush=True)
        if MODE in ("all", "host") and (method != "linear" or kw):
            ms = host_glue_ms(method, kw, fa, fb, out)
            print(f"host glue {what}: median {statistics.median(ms):.0f} ms (min {min(ms):.0f}, max {max(ms):.0f}, {HOST_REPS} runs)",
                  flush=True)
