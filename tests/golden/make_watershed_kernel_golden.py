"""Regenerate tests/golden/watershed_ref_kernel.npz: the labels of the reference's own compiled flood kernel
(_watershed.pyx's watershed_raveled, built into oracle/_ref by oracle/build_ref.py), fed by the oracle's restatement of
watershed.py (oracle/ws_oracle.py, use_ref=True), on every case of watershed_ref.npz:

  <case>/labels     the case as stored
  <case>/labels_q8  the same case with its field rounded to steps of 1/8 -- plateaus whose flood order the heap's
                    internal order of equal values decides

tests/test_oracle_golden.py::test_c_twin_matches_live_reference_kernel compares the C twin with these labels everywhere,
and with the kernel itself where oracle/_ref is built.  Run from the repository root, with oracle/_ref built:
    python3 tests/golden/make_watershed_kernel_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader, ws_oracle  # noqa: E402


def quantised(field):
    return (np.round(field * 8) / 8).astype(np.float32)


if __name__ == "__main__":
    if not ref_loader.available():
        sys.exit("oracle/_ref is not built: the reference kernel is needed to regenerate this fixture")
    z = np.load(os.path.join(HERE, "watershed_ref.npz"))
    out = {}
    for name in sorted({k.split("/")[0] for k in z.files if not k.startswith("neighbour_order")}):
        c = {k.split("/")[1]: z[k] for k in z.files if k.startswith(name + "/")}
        for key, field in (("labels", c["field"]), ("labels_q8", quantised(c["field"]))):
            out[name + "/" + key] = ws_oracle.watershed(c["fwd"], c["bwd"], field, c["markers"], c.get("mask"),
                                                        int(c["conn"]), use_ref=True)
    path = os.path.join(HERE, "watershed_ref_kernel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
