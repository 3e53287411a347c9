"""Generate tests/golden/ellipse_ref.npz from the REFERENCE ITSELF: get_marker_distance_ellipse on the volumes of
tests/ellipse_cases.py at every sampling.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_ellipse_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/utils/label_utils.py and tobac_flow/validation.py by path, with the stand-in modules of
make_validation_golden.py for xarray, tobac_flow.utils and tobac_flow.dataset.  Stored per volume: the markers; per volume
and sampling: the reference's distances (float64) and closest markers, and the indices of
scipy.ndimage.distance_transform_edt(markers == 0, return_indices=True, sampling=(margin / time_margin, 1, 1)), the call
the reference makes (as int16: every axis is short).  The volume without a marker is stored as an input only: the
reference's result for it is meaningless.  Only data is written to the repository.

Asserted: the reference's distances are SciPy's, and SciPy's distance is its own expression E at its own index, bit for
bit; in every case at most 5 % of the voxels have several features within 4 eps of the brute-force minimum; the file
stays under 1 MB.  Printed per case: that share, and how many of those voxels the NumPy restatement of ellipse_cases.py
decides differently from SciPy."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ellipse_cases as ec  # noqa: E402

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

out = {}
for name, make in ec.VOLUMES.items():
    markers = make()
    out[f"{name}/markers"] = markers
    if not markers.any():
        continue
    for sname, (margin, time_margin) in ec.SAMPLINGS.items():
        s = ec.sampling(sname)
        distances, closest = ref.get_marker_distance_ellipse(markers, time_margin, margin)
        scipy_distances, indices = ndi.distance_transform_edt(markers == 0, return_indices=True, sampling=(s, 1, 1))
        assert np.array_equal(distances, scipy_distances) and distances.dtype == np.float64
        assert np.array_equal(distances, ec.at_indices(indices, s)), "SciPy's distance is not E at its own index"
        assert np.array_equal(closest, ec.closest_at(markers, indices)) and closest.dtype == markers.dtype
        assert max(markers.shape) < 2 ** 15
        out[f"{name}/{sname}/distances"] = distances
        out[f"{name}/{sname}/closest"] = closest
        out[f"{name}/{sname}/indices"] = indices.astype(np.int16)
        b = ec.brute_force(name, sname)
        several = b["count"] > 1
        assert several.mean() <= ec.TIE_SHARE_CAP, (name, sname, several.mean())
        assert (distances <= b["minimum"] * (1 + 4 * ec.EPS)).all()
        mine = ec.restate(markers, s)
        differ = (mine[0] != distances) | (mine[1] != indices).any(0)
        assert not differ[~several].any(), "the restatement differs from SciPy where the nearest feature is unique"
        print(f"{name} {markers.shape} at sampling {sname}: {several.mean() * 100:.2f} % of the voxels have several features "
              f"within 4 eps of the minimum; the restatement differs from SciPy at {int(differ.sum())} of them "
              f"(distance: {int((mine[0] != distances).sum())}); SciPy above the brute-force minimum at "
              f"{int((distances > b['minimum']).sum())} voxels")
path = os.path.join(HERE, "ellipse_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("wrote", path, size, "bytes")
assert size < 1_000_000, "the fixture must stay under 1 MB"
