"""Generate tests/golden/validation_ref.npz from the REFERENCE ITSELF: flash / marker distances, POD and FAR.  Run by hand
where a checkout of the reference exists:

    python tests/golden/make_validation_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/utils/label_utils.py and tobac_flow/validation.py by path.  validation.py imports
xarray, tobac_flow.utils and tobac_flow.dataset at module level; stand-in modules replace them: `xarray` with an empty
DataArray class (the functions only ask isinstance of it), `tobac_flow.utils` carrying the loaded apply_func_to_labels,
`tobac_flow.dataset` with the two names the unused validate_* wrappers import.  Inputs come from tests/validation_cases.py
and are stored beside the reference's results; only data is written to the repository.

Stored, for the (6, 37, 70) volume of labelled boxes: get_marker_distance at time_range 1 and 2;
get_marker_distance_cylinder with and without get_closest at time_margin 0, 2 and 7 (>= T); the sequence of
scripts/dcc_validation.py:145-155 (flash distance, edge filter, flashes in margin) and the full validate_markers tuple
for both get_closest values; get_edge_filter without a time gap, with one > 900 s, and with missing GLM data;
get_min_dist_for_objects over a field with an all-NaN label, a label over inf and an absent id.  For the (4, 33, 300)
volume: get_marker_distance and the cylinder with get_closest at time_margin 1.

The script asserts that every volume has tie pixels (several features at the minimal distance) and pixels without, and
that POD and FAR are neither 0, 1 nor NaN."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import validation_cases as vc  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)


def load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(sys.argv[1], "tobac_flow", *parts))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


ref_labels = load("reference_label_utils", "utils", "label_utils.py")
for name, members in (("xarray", {"DataArray": type("DataArray", (), {})}), ("tobac_flow", {}),
                      ("tobac_flow.utils", {"apply_func_to_labels": ref_labels.apply_func_to_labels}),
                      ("tobac_flow.dataset", {"add_dataarray_to_ds": None, "create_dataarray": None})):
    stand_in = types.ModuleType(name)
    stand_in.__dict__.update(members)
    sys.modules[name] = stand_in
ref = load("reference_validation", "validation.py")


class Flashes(np.ndarray):
    """the one DataArray method get_edge_filter calls on glm_flashes"""
    def to_numpy(self):
        return np.asarray(self)


def has_ties_and_none(markers, time_margin):
    _, count, sets, _ = vc.brute_force(markers, time_margin)
    several_labels = (sets != 0) & ~vc.single_label(sets)
    assert (count > 1).any() and (count == 1).any() and several_labels.any(), "the case needs tie pixels and others"
    return int((count > 1).sum()), int(several_labels.sum())


out = {}
M, TM = vc.MARGIN, vc.TIME_MARGIN

labels = vc.boxes()
A = {"labels": labels}
for time_range in (1, 2):
    A[f"marker_distance_{time_range}"] = ref.get_marker_distance(labels, time_range)
for tm in (0, 2, 7):
    A[f"cylinder_{tm}"] = ref.get_marker_distance_cylinder(labels, tm)
    A[f"cylinder_{tm}_closest_distance"], A[f"cylinder_{tm}_closest"] = ref.get_marker_distance_cylinder(labels, tm, get_closest=True)
    assert np.array_equal(A[f"cylinder_{tm}"], A[f"cylinder_{tm}_closest_distance"])
    print("boxes, time margin", tm, "(pixels with several nearest features, with several nearest labels):", has_ties_and_none(labels, tm))

grid = vc.flash_grid(labels.shape)
A["glm_grid_raw"] = grid.copy()
ds = types.SimpleNamespace(glm_flashes=grid.copy().view(Flashes), t=vc.flash_times(labels.shape[0]))
A["times"] = ds.t.astype(np.int64)
A["glm_distance"] = ref.get_marker_distance_cylinder(grid, TM)
A["edge_filter"] = ref.get_edge_filter(ds, M, TM)
assert not A["edge_filter"][np.isnan(grid)].any(), "the NaN count must lie where the edge filter clears it"
grid[~A["edge_filter"]] = 0
A["glm_grid"] = grid
A["n_glm_in_margin"] = np.nansum(grid)
A["index"] = vc.label_index(labels)
for get_closest in (False, True):
    result = ref.validate_markers(labels, grid, A["glm_distance"], A["edge_filter"], A["n_glm_in_margin"], coord=A["index"],
                                  margin=M, time_margin=TM, get_closest=get_closest)
    names = ("flash_distance", "flash_closest", "marker_distance", "pod", "far", "n_marker_in_margin", "margin_flag")
    for name, value in zip(names, result):
        if value is not None:
            A[f"validate_{int(get_closest)}_{name}"] = np.asarray(value)
    pod, far = float(result[3]), float(result[4])
    assert 0 < pod < 1 and 0 < far < 1, (pod, far)
    print("validate_markers get_closest =", get_closest, "POD", pod, "FAR", far, "markers in margin", int(result[5]),
          "flashes", result[0].size)
ds_gap = types.SimpleNamespace(glm_flashes=ds.glm_flashes, t=vc.flash_times(labels.shape[0], gap_after=2))
A["times_gap"] = ds_gap.t.astype(np.int64)
A["edge_filter_gap"] = ref.get_edge_filter(ds_gap, M, TM)
assert A["edge_filter_gap"].sum() < A["edge_filter"].sum()
missing = vc.flash_grid(labels.shape)
missing[3, 18, 35] = -1
A["glm_grid_missing"] = missing
A["edge_filter_missing"] = ref.get_edge_filter(types.SimpleNamespace(glm_flashes=missing.view(Flashes), t=ds.t), M, TM)
assert A["edge_filter_missing"].sum() < A["edge_filter"].sum()
field, special = vc.distance_field_with_specials(labels, A["glm_grid_raw"])
A["special_field"] = field
A["special_min"] = ref.get_min_dist_for_objects(field, labels, index=A["index"])
row = {int(i): k for k, i in enumerate(A["index"])}
assert np.isnan(A["special_min"][row[special["all_nan"]]]) and np.isnan(A["special_min"][row[special["absent"]]])
assert np.isposinf(A["special_min"][row[special["over_inf"]]]) and np.isfinite(A["special_min"]).sum() >= 3

labels_b = vc.borders()
B = {"labels": labels_b, "marker_distance_1": ref.get_marker_distance(labels_b, 1)}
B["cylinder_1_closest_distance"], B["cylinder_1_closest"] = ref.get_marker_distance_cylinder(labels_b, 1, get_closest=True)
print("borders, time margin 1:", has_ties_and_none(labels_b, 1))

for case, arrays in (("boxes", A), ("borders", B)):
    for name, value in arrays.items():
        out[f"{case}/{name}"] = value
path = os.path.join(HERE, "validation_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
