"""Generate tests/golden/label_reduce_ref.npz from the REFERENCE ITSELF: labeled_comprehension and apply_func_to_labels with
every reducer the device path recognises, on the cases of tests/label_reduce_cases.py.  Run by hand where a checkout of the
reference exists:

    python tests/golden/make_label_reduce_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/utils/label_utils.py by path (it imports only NumPy and SciPy) and stores, per case and
reducer, `lc/<case>/<reducer>` = labeled_comprehension(field, labels, func, index, dtype, default) and, for the cases
that are for both functions, `af/<case>/<reducer>` = apply_func_to_labels(labels, field, func=func, index=index,
default=default).  Where the reference raises, the key goes into `errors` as "<key>:<exception type>" instead.  Only data
is written to the repository.  find_overlap_mode is not in here: its module imports xarray; the tests take its expected
values from scipy.stats.mode."""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import label_reduce_cases as lc  # noqa: E402

warnings.filterwarnings("ignore")
np.seterr(all="ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)
spec = importlib.util.spec_from_file_location("reference_label_utils",
                                              os.path.join(sys.argv[1], "tobac_flow", "utils", "label_utils.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

out, errors = {}, []


def keep(key, call):
    try:
        value = np.asarray(call())
        if value.dtype == object:
            raise TypeError("object result")
        out[key] = value
    except Exception as e:  # noqa: BLE001
        errors.append(f"{key}:{type(e).__name__}")


for name, c in lc.build().items():
    for reducer, func in lc.REDUCERS.items():
        keep(f"lc/{name}/{reducer}", lambda: ref.labeled_comprehension(c["field"], c["labels"], func, index=c["index"],
                                                                      dtype=c["dtype"], default=c["default"]))
        if c["apply"]:
            keep(f"af/{name}/{reducer}", lambda: ref.apply_func_to_labels(c["labels"], c["field"], func=func, index=c["index"],
                                                                         default=c["default"]))
out["errors"] = np.array(sorted(errors))
np.savez_compressed(lc.GOLDEN, **out)
print(len(out) - 1, "results,", len(errors), "errors,", os.path.getsize(lc.GOLDEN), "bytes")
for e in errors:
    print("  ", e)
