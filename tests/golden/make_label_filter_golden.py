"""Generate tests/golden/label_filter_ref.npz from the REFERENCE ITSELF: the ten label filters of tobac_flow/analysis.py
(find_object_lengths, mask_labels, the five filter_labels_by_* and their three *_legacy forms) on the volumes of
tests/label_filter_cases.py.  Run by hand where a checkout of the reference exists, with an interpreter whose NumPy still
has np.bool8 (filter_labels_by_multimask uses it; python 3.9 with numpy 1.26 and scipy 1.7 wrote the committed file):

    python3.9 tests/golden/make_label_filter_golden.py <path to the reference checkout>

It executes the reference's tobac_flow/analysis.py by path.  Empty stand-in modules replace xarray, tobac_flow.dataset and
tobac_flow.utils.legacy_utils (the five names analysis.py imports from them are None: the label filters use none of them).
Only data is written into the repository: the label volumes, the fields and masks (bool volumes bit-packed), and per
recorded call the reference's result or the name of the exception it raised.

Asserted while writing: the first volume's lengths are [2, 2, 1, 1], and every legacy form equals its successor wherever both
return."""
import importlib.util
import os
import sys
import types
import warnings

warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import label_filter_cases as lc  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
for name, names in (("xarray", ()), ("tobac_flow", ()), ("tobac_flow.utils", ()),
                    ("tobac_flow.dataset", ("add_dataarray_to_ds", "create_dataarray", "n_unique_along_axis")),
                    ("tobac_flow.utils.legacy_utils", ("apply_func_to_labels", "apply_weighted_func_to_labels"))):
    module = types.ModuleType(name)
    for n in names:
        setattr(module, n, None)
    sys.modules[name] = module
spec = importlib.util.spec_from_file_location("reference_analysis", os.path.join(sys.argv[1], "tobac_flow", "analysis.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

import scipy  # noqa: E402
out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__)}
for volume, make in lc.GENERATORS.items():
    case = make()
    labels = case["labels"]
    assert labels.dtype == np.int32 and labels.ndim == 3
    out[f"{volume}/labels"] = labels.astype(np.uint8)
    assert labels.min() >= 0 and labels.max() < 256
    for name, a in case["fields"].items():
        assert a.shape == labels.shape
        out[f"{volume}/field/{name}"] = np.packbits(a.ravel()) if a.dtype == bool else a
    masks = [np.asarray(lc.as_mask(case, q)) for q in case["criteria"]]
    assert all(m.dtype == bool for m in masks)
    results = {}
    for key, name, which, min_length in lc.calls(case):
        given = labels.copy()
        try:
            got = lc.call(ref, name, given, None if which is None else [masks[k] for k in which], min_length)
            got = np.asarray(got)
            if "legacy" in name:
                assert np.shares_memory(got, given)               # the legacy forms mutate their argument
            assert got.dtype != object
            results[key] = got
            out[f"{volume}/{key}"] = got.astype(np.uint8) if got.dtype == np.int32 else got
        except Exception as e:  # noqa: BLE001
            results[key] = type(e).__name__
            out[f"{volume}/{key}/raises"] = np.array(type(e).__name__)
            out[f"{volume}/{key}/message"] = np.array(str(e))
        shown = results[key] if isinstance(results[key], str) or results[key].size < 12 else f"max {int(results[key].max())}"
        print(f"{volume} {labels.shape} {key}: {shown}")
    for key, got in results.items():
        twin = key.replace("_legacy", "")
        if twin != key and not isinstance(got, str) and not isinstance(results[twin], str):
            assert np.array_equal(got, results[twin]), (volume, key)
    if volume == "odd":
        assert results["lengths"].tolist() == [2, 2, 1, 1]
        for ml in lc.MIN_LENGTHS:
            assert np.array_equal(results[f"by_length_and_multimask/4/{ml}"], results[f"by_length_and_multimask_legacy/4/{ml}"])

path = os.path.join(HERE, "label_filter_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("wrote", path, size, "bytes")
assert size < 250_000
