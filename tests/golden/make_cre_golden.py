"""Generate tests/golden/cre_ref.npz from the REFERENCE ITSELF: add_cre_to_dataset (and through it get_cre) of
tobac_flow/postprocess.py:29-99.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_cre_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/postprocess.py by path.  Empty modules stand in for xarray and for the
tobac_flow.utils imports, none of which the two functions use.  The reference's function runs as written on a duck-typed
dataset: a dict with attribute access whose values are an ndarray subclass carrying the `.name` and the `.attrs`
(long_name, standard_name, valid_max) that get_cre reads and writes.  Values, dtypes, names and their order are therefore
the reference's own arithmetic on NumPy arrays.  Only data is written to the repository.

The inputs are the seeded planes of tests/field_props_cases.py (cre_inputs) as float32 and as float64; the fixture stores
them, the ten results per dtype, the names in the order the reference added them and a provenance line."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import field_props_cases as fc  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)


class AnyName(types.ModuleType):
    """a module every name can be imported from (the reference imports a dozen helpers it does not use here)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


for module in ("xarray", "tobac_flow", "tobac_flow.utils", "tobac_flow.utils.geo_utils"):
    sys.modules[module] = AnyName(module)
spec = importlib.util.spec_from_file_location("reference_postprocess", os.path.join(sys.argv[1], "tobac_flow", "postprocess.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


class DuckArray(np.ndarray):
    """what get_cre and add_cre_to_dataset read and write of a DataArray"""

    def __new__(cls, data, name):
        obj = np.asarray(data).view(cls)
        obj.name = name
        obj.attrs = {"long_name": name, "standard_name": name, "units": "W m-2", "valid_min": 0.0, "valid_max": 1500.0}
        return obj

    def __array_finalize__(self, obj):
        self.name = getattr(obj, "name", None)
        self.attrs = dict(getattr(obj, "attrs", {}))


class DuckDataset(dict):
    __getattr__ = dict.__getitem__


out, order = {}, None
for dtype in ("float32", "float64"):
    inputs = fc.cre_inputs(dtype)
    ds = DuckDataset({name: DuckArray(a.copy(), name) for name, a in inputs.items()})
    assert ref.add_cre_to_dataset(ds) is ds
    added = [name for name in ds if name not in inputs]
    assert order in (None, added) and len(added) == 10
    order = added
    for name, a in inputs.items():
        assert np.array_equal(np.asarray(ds[name]), a, equal_nan=True), "the reference does not modify its inputs"
        out[f"{dtype}/in/{name}"] = a
    for name in added:
        assert ds[name].dtype == np.dtype(dtype) and ds[name].name == name
        out[f"{dtype}/out/{name}"] = np.array(ds[name])
out["meta/names"] = np.array(order)
out["meta/provenance"] = np.array("values, dtypes, names and order: the reference's add_cre_to_dataset / get_cre as written, on an "
                                  "ndarray subclass with .name and .attrs; numpy " + np.__version__)
path = os.path.join(HERE, "cre_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays; order:", ", ".join(order))
