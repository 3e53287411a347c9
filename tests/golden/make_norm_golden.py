"""Generate tests/golden/norm_ref.npz and norm_ref_big.npz from the REFERENCE ITSELF: to_8bit(method(pair, **kwargs), 0, 1) for every case of
tests/norm_cases.py.  Run by hand where a checkout of the reference exists (numpy 2 and SciPy are all it needs):

    python tests/golden/make_norm_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/utils/normalisation_utils.py by path and stores the input fields and the expected
bytes.  Only data is written to the repository."""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import norm_cases  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)
assert int(np.__version__.split(".")[0]) >= 2, "the yardstick is numpy 2's promotion of Python scalars"
path = os.path.join(sys.argv[1], "tobac_flow", "utils", "normalisation_utils.py")
spec = importlib.util.spec_from_file_location("reference_normalisation_utils", path)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

fields = norm_cases.fields()
out, big = {"field/" + k: v for k, v in fields.items()}, {}
for name, (method, kw, field) in norm_cases.cases().items():
    pair = fields[field].copy()
    with np.errstate(all="ignore"):
        want = ref.to_8bit(ref.select_normalisation_method(method)(pair, **kw), 0, 1)
    assert want.dtype == np.uint8 and want.shape == pair.shape
    assert np.array_equal(pair, fields[field], equal_nan=True), "the reference changed its input"
    (big if field == "smooth_big" else out)["want/" + name] = want
    print(f"{name:40s} exact={norm_cases.is_exact(method, kw, pair)!s:5s} distinct bytes {np.unique(want).size}")
for target, content in ((norm_cases.GOLDEN, out), (norm_cases.GOLDEN_BIG, big)):
    np.savez_compressed(target, **content)
    print("wrote", target, os.path.getsize(target), "bytes")
print(len(norm_cases.cases()), "cases")
