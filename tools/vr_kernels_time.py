"""ms per refinement of one frame pair (both directions are the same work: one direction is timed) split by kernel, from the
library's own HIP events, and a sha1 of the refined flow (development aid).  One process per build of the library:

  TF_LIB_PATH=<other build> python tools/vr_kernels_time.py [size] [calls]
"""
import hashlib, sys
sys.path.insert(0, ".")
import numpy as np, torch
import tobac_flow_amd.flow as tf
from tobac_flow_amd import _lib
from tools.synth import blob_stack
H = W = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 6
bt = torch.as_tensor(blob_stack(2, H, W)).cuda().float()
lo, hi = bt.min(), bt.max()
a, b = [((bt[i] - lo) / (hi - lo) * 255).to(torch.uint8).contiguous() for i in (0, 1)]
g = torch.Generator(device="cuda").manual_seed(1)
flow0 = torch.randn((H, W, 2), device="cuda", generator=g)
vr = tf.VariationalRefinement.create()
for _ in range(2):
    f = flow0.clone(); vr.calc_dev(a, b, f)
torch.cuda.synchronize()
_lib.profile_enable(True); _lib.profile_collect()
for _ in range(calls):
    f = flow0.clone(); vr.calc_dev(a, b, f)
torch.cuda.synchronize()
prof = _lib.profile_collect(); _lib.profile_enable(False)
ms = {k: v[1] / calls for k, v in prof.items() if k.startswith("vr_")}
print("lib %s  %dx%d  " % (_lib.lib_path().split("/")[-1], H, W) + "  ".join("%s %.3f" % kv for kv in sorted(ms.items())) +
      "  sum %.3f  sha1 %s" % (sum(ms.values()), hashlib.sha1(f.cpu().numpy().tobytes()).hexdigest()[:16]), flush=True)
