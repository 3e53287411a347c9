"""Time convolve_step on one device-resident 5424^2 frame triple (cubic, connectivity 1 and 3) against the way the
fused entry point gives the same stack: torch.stack of the three frames + convolve_dev(FUNC_STACK, t0=1, t1=2).
HIP events, outputs allocated beforehand, the two forms alternate; median of RUNS after WARM warm-ups.
Usage: python tools/step_api_time.py [size] (development aid; the figures are kept in profiles/step_api_notes.txt)"""
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np
import scipy.ndimage as ndi
import torch

from tobac_flow_amd import _lib
from tobac_flow_amd.convolve import convolve_dev, convolve_step

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
WARM, RUNS = 5, 25
dev = _lib.device()
gen = torch.Generator(device=dev).manual_seed(3)
yy, xx = torch.meshgrid(torch.arange(N, device=dev, dtype=torch.float32), torch.arange(N, device=dev, dtype=torch.float32), indexing="ij")


def frame(k):
    f = torch.sin(xx * (0.011 + 0.002 * k)) * torch.cos(yy * 0.013) + 0.05 * torch.randn((N, N), device=dev, generator=gen)
    f[torch.rand((N, N), device=dev, generator=gen) < 0.01] = float("nan")
    return f.contiguous()


def flow(k):
    return torch.stack([2.0 * torch.sin(yy * 0.004 + k) + 0.3, 1.5 * torch.cos(xx * 0.005 - k) - 0.2], -1).contiguous()


prev, same, nxt = frame(0), frame(1), frame(2)
fwd, bwd = flow(0), flow(1)
fwd3, bwd3 = fwd.expand(3, N, N, 2).contiguous(), bwd.expand(3, N, N, 2).contiguous()   # the fused form wants (T, H, W, 2)
del yy, xx


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for k in (1, 3):
    s = ndi.generate_binary_structure(3, k)
    n = int(s.sum())
    res = torch.empty((n, N, N), dtype=torch.float32, device=dev)
    out3 = torch.empty((n, 3, N, N), dtype=torch.float32, device=dev)

    def step():
        convolve_step(prev, same, nxt, fwd, bwd, structure=s, method="cubic", dtype=np.float32, res=res)

    def fused():
        vol = torch.stack([prev, same, nxt])
        convolve_dev(vol, fwd3, bwd3, s, "cubic", np.float32, float("nan"), _lib.FUNC_STACK, t0=1, t1=2, out=out3)

    for _ in range(WARM):
        step()
        fused()
    torch.cuda.synchronize()
    a, b = res, out3[:, 1]
    same_bits = bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    ts, tf = [], []
    for _ in range(RUNS):
        ts.append(timed(step))
        tf.append(timed(fused))
    print(f"{N}^2 cubic connectivity {k} ({n} taps): convolve_step median {statistics.median(ts):.3f} ms "
          f"(min {min(ts):.3f}, max {max(ts):.3f}); stack + convolve_dev median {statistics.median(tf):.3f} ms "
          f"(min {min(tf):.3f}, max {max(tf):.3f}); {RUNS} runs after {WARM} warm-ups; identical output: {same_bits}", flush=True)
    del res, out3
