"""Generate tests/golden/validate_ref.npz from the REFERENCE ITSELF: the five validate_* wrappers of tobac_flow/validation.py
and its validate_markers, on the product of tests/validate_cases.py.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_validate_golden.py <path to the reference checkout>

validation.py is loaded by path, as tests/golden/make_validation_golden.py loads it: `xarray` is a stand-in with an empty
DataArray class, `tobac_flow.utils` carries the reference's own apply_func_to_labels, and `tobac_flow.dataset` carries a
recording create_dataarray / add_dataarray_to_ds that stores `array.astype(dtype)`, the dims and the name -- what
tobac_flow/utils/xarray_utils.py:5-22 hands to xarray.  The members of the detection dataset are an ndarray subclass with
`to_numpy`.  Only data is written to the repository.

Stored: the inputs (so that the CPU test can pin the case module to them); under `wrappers<c>/` the variables the five
wrappers write for the product as it is -- coordinates with an id that is in no volume -- at get_closest = c; under
`stage<c>/` the same after the script's own statements (scripts/dcc_validation.py:96-116, 149-155: coordinates cut to
the ids present, flash distance, edge filter, grid zeroed outside it), plus flash_count_total and flash_count_in_margin;
`<case>/dims` lists name=dim,dim for every variable.

The script asserts, for each of the five sets, 0 < POD < 1, 0 < FAR < 1 and at least two markers inside the margin, that
one flash count inside the margin is > 1, and that the flashes at which several labels are equally near are a minority
of the flashes -- and that the two core sets have one, so that the allowance for them is used."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import validate_cases as cases  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)


def load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(sys.argv[1], "tobac_flow", *parts))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def create_dataarray(array, dims, name, coords=None, long_name=None, units=None, dtype=None):
    return name, array.astype(dtype), tuple(dims)


def add_dataarray_to_ds(da, ds):
    ds[da[0]] = da[1:]


ref_labels = load("reference_label_utils", "utils", "label_utils.py")
for name, members in (("xarray", {"DataArray": type("DataArray", (), {})}), ("tobac_flow", {}),
                      ("tobac_flow.utils", {"apply_func_to_labels": ref_labels.apply_func_to_labels}),
                      ("tobac_flow.dataset", {"add_dataarray_to_ds": add_dataarray_to_ds, "create_dataarray": create_dataarray})):
    stand_in = types.ModuleType(name)
    stand_in.__dict__.update(members)
    sys.modules[name] = stand_in
ref = load("reference_validation", "validation.py")


class Member(np.ndarray):
    """the one DataArray method the wrappers and get_edge_filter call"""
    def to_numpy(self):
        return np.asarray(self)


def dataset(arrays):
    return types.SimpleNamespace(**{k: np.asarray(v).view(Member) for k, v in arrays.items()})


M, TM = cases.MARGIN, cases.TIME_MARGIN
product = cases.product()
raw = cases.flash_grid()
times = cases.flash_times()
out = {f"inputs/{k}": v for k, v in product.items()}
out["inputs/glm_grid_raw"], out["inputs/times"] = raw, times.astype(np.int64)

# scripts/dcc_validation.py:149-155
grid = raw.copy()
glm_distance = ref.get_marker_distance_cylinder(grid, TM)
n_total = np.nansum(grid[grid > 0])
edge = ref.get_edge_filter(types.SimpleNamespace(glm_flashes=grid.view(Member), t=times), M, TM)
grid[np.logical_not(edge)] = 0
n_in = np.nansum(grid)
assert (grid[edge] > 1).any() and not np.isnan(grid).any() and set(np.unique(raw[~np.isnan(raw)])) == {0, 1, 2, 3}
out["inputs/glm_grid"], out["inputs/glm_distance"], out["inputs/edge_filter"], out["inputs/n_glm_in_margin"] = grid, glm_distance, edge, n_in

WRAPPERS = (ref.validate_cores, ref.validate_cores_with_anvils, ref.validate_anvils, ref.validate_anvils_with_cores,
            ref.validate_anvil_markers)


def run(arrays, case, get_closest, extra=()):
    ds, written = dataset(arrays), dict(extra)
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")        # the wrappers print their progress
    try:
        for wrapper in WRAPPERS:
            wrapper(ds, written, grid, glm_distance, edge, n_in, M, TM, get_closest=get_closest)
    finally:
        sys.stdout = stdout
    for name, (value, dims) in written.items():
        out[f"{case}/{name}"] = np.asarray(value)
    out[f"{case}/dims"] = np.array([f"{name}={','.join(dims)}" for name, (_, dims) in written.items()])
    return written


for get_closest in (0, 1):
    run(product, f"wrappers{get_closest}", bool(get_closest))
    counts = {"flash_count_total": create_dataarray(n_total, (), "flash_count_total", dtype=np.int32)[1:],
              "flash_count_in_margin": create_dataarray(n_in, (), "flash_count_in_margin", dtype=np.int32)[1:]}
    written = run(cases.cut_to_present(product), f"stage{get_closest}", bool(get_closest), counts)
    for name in cases.SETS:
        pod, far, n = float(written[f"{name}_pod"][0]), float(written[f"{name}_far"][0]), int(written[f"{name}_count_in_margin"][0])
        assert 0 < pod < 1 and 0 < far < 1 and n >= 2, (name, pod, far, n)
        print(f"get_closest {get_closest} {name}: POD {pod:.4f} FAR {far:.4f} markers in margin {n} flashes {written[f'flash_{name}_distance'][0].size}")

for name, (labels, _) in cases.restate_subsets(product).items():
    ties = cases.tie_flashes(labels, grid, TM)[0]
    assert 2 * ties.sum() < ties.size and ties.any() == name.startswith("core"), (name, int(ties.sum()), ties.size)
    print(f"{name}: {int(ties.sum())} of {ties.size} flashes have several labels at the minimal distance")

# the tuple of validate_markers itself for one set, both get_closest values: validate_markers(flashes=...) is held to it
for get_closest in (0, 1):
    result = ref.validate_markers(product["anvil_marker_label"], grid, glm_distance, edge, n_in, coord=product["anvil_marker"],
                                  margin=M, time_margin=TM, get_closest=bool(get_closest))
    for name, value in zip(("flash_distance", "flash_closest", "marker_distance", "pod", "far", "n_marker_in_margin", "margin_flag"), result):
        if value is not None:
            out[f"markers{get_closest}/{name}"] = np.asarray(value)

path = os.path.join(HERE, "validate_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
