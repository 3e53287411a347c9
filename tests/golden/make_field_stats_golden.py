"""Generate tests/golden/field_stats_ref.npz from the REFERENCE ITSELF: get_bulk_stats, get_spatial_stats and
get_temporal_stats of tobac_flow/dataset.py:19-148.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_field_stats_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/dataset.py by path.  Empty modules stand in for xarray and for the tobac_flow.*
imports, none of which the three functions use, and for create_dataarray, which here records
(array.astype(dtype), dims, name).  Only data is written to the repository.

What comes from where (also stored as meta/provenance):
  * get_bulk_stats runs as the reference wrote it, on an object with the .data / .name / .long_name / .units / .dtype it
    reads: values, names, dims and dtypes are the reference's own arithmetic.
  * get_spatial_stats / get_temporal_stats run the reference's function too -- names, dims and dtypes are its own -- on a
    duck-typed `da` whose .mean / .std / .median / .max / .min are NumPy's nan-functions over the named axes: xarray's
    documented defaults for float data (skipna=True, ddof=0), xarray itself not being installed here.  Their VALUES are
    that restatement.

The inputs are the seeded cases of tests/field_stats_cases.py; the fixture stores a fingerprint of each input, not the
input, and the results per case, function and dtype."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import field_stats_cases as fc  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)

RECORDED = []


def create_dataarray(array, dims, name, long_name=None, units=None, dtype=None):
    rec = (np.asarray(array).astype(dtype), tuple(dims), name)
    RECORDED.append(rec)
    return rec


def stand_in(name, **attributes):
    module = types.ModuleType(name)
    for k, v in attributes.items():
        setattr(module, k, v)
    sys.modules[name] = module


stand_in("xarray", Dataset=None, DataArray=None)          # named in annotations only
stand_in("tobac_flow")
stand_in("tobac_flow.abi", get_abi_lat_lon=None, get_abi_pixel_area=None)
stand_in("tobac_flow.utils")
stand_in("tobac_flow.utils.xarray_utils", create_dataarray=create_dataarray, add_dataarray_to_ds=None)
stand_in("tobac_flow.utils.label_utils", apply_func_to_labels=None, labeled_comprehension=None, slice_labels=None, remap_labels=None)
stand_in("tobac_flow.utils.datetime_utils", get_datetime_from_coord=None)
stand_in("tobac_flow.utils.legacy_utils", apply_weighted_func_to_labels=None)
stand_in("tobac_flow.utils.stats_utils", find_overlap_mode=None, n_unique_along_axis=None)
spec = importlib.util.spec_from_file_location("reference_dataset", os.path.join(sys.argv[1], "tobac_flow", "dataset.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


class Reduced:
    def __init__(self, data):
        self.data = data


class DuckArray:
    """what the three functions read of a DataArray; the reductions are xarray's float defaults restated with NumPy"""
    AXIS = {"t": 0, "y": 1, "x": 2}

    def __init__(self, data, name):
        self.data, self.name, self.long_name, self.units, self.dtype = data, name, name, "1", data.dtype

    def _reduce(self, fn, dims):
        dims = (dims,) if isinstance(dims, str) else dims
        return Reduced(fn(self.data, axis=tuple(sorted(self.AXIS[d] for d in dims))))

    def mean(self, dims): return self._reduce(np.nanmean, dims)          # noqa: E704
    def std(self, dims): return self._reduce(np.nanstd, dims)            # noqa: E704
    def median(self, dims): return self._reduce(np.nanmedian, dims)      # noqa: E704
    def max(self, dims): return self._reduce(np.nanmax, dims)            # noqa: E704
    def min(self, dims): return self._reduce(np.nanmin, dims)            # noqa: E704


FUNCTIONS = {"all": ref.get_bulk_stats, "frame": ref.get_spatial_stats, "time": ref.get_temporal_stats}
out = {}
for dtype in fc.DTYPES:
    for name in fc.fixture_cases(dtype):
        a = fc.cases(dtype)[name]
        out[f"{dtype}/{name}/fingerprint"] = np.array(fc.fingerprint(a))
        for over in fc.geometries_of(name):
            del RECORDED[:]
            FUNCTIONS[over](DuckArray(np.array(a), "field"))
            assert len(RECORDED) == 5
            for stat, (values, dims, var) in zip(fc.STATS, RECORDED):
                assert values.dtype == a.dtype
                out[f"{dtype}/{name}/{over}/{stat}"] = values
                out.setdefault(f"meta/{over}/names", []).append(var)
                out.setdefault(f"meta/{over}/dims", []).append(",".join(dims))
for over in fc.GEOMETRIES:
    for key in ("names", "dims"):
        every = out[f"meta/{over}/{key}"]
        assert all(every[i] == every[i % 5] for i in range(len(every))), "names and dims do not depend on the case"
        out[f"meta/{over}/{key}"] = np.array(every[:5])
out["meta/provenance"] = np.array([
    "all: values, names, dims, dtypes -- the reference's get_bulk_stats as written (np.nanmean, np.nanstd, np.median, np.nanmax, np.nanmin)",
    "frame, time: names, dims, dtypes -- the reference's get_spatial_stats / get_temporal_stats as written; values -- NumPy's "
    "nan-functions over the named axes, restating xarray's float defaults skipna=True, ddof=0",
    "numpy " + np.__version__])
path = os.path.join(HERE, "field_stats_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
