"""Generate tests/golden/subsegment_ref.npz from the REFERENCE ITSELF: subsegment_labels (tobac_flow/label.py:13-80) on the
volumes of tests/subsegment_cases.py over the 3 x 3 grid of shrink_factor and peak_min_distance, and flow_label with
subsegment_shrink = 0.3 on the flow-linked case.  Run by hand, with an interpreter that has scikit-image 0.18.3 (python 3.9,
numpy 1.26 wrote the committed file), where a checkout of the reference exists:

    python3.9 tests/golden/make_subsegment_golden.py <path to the reference checkout>

It executes the reference's tobac_flow/label.py and tobac_flow/utils/label_utils.py from a temporary package, each with ONE
prepended line (``from __future__ import annotations`` -- python3.9 cannot evaluate their PEP-604 annotations).  Only data
is written into the repository: the masks (bit-packed), the flows of the flow-linked case and the reference's labels.

The flow-linked case.  flow_label only needs an object with `.convolve`; the reference's Flow.convolve remaps with OpenCV.
The stand-in (tests/label_glue_cases.ShiftFlow) shifts by the flows instead, which is what a nearest-neighbour remap does
when every flow vector is INTEGER-VALUED, as the stored ones are (int8): the sample position is a pixel centre, there is nothing to round, and a
position outside the frame gives the fill value.  tobac_flow_amd's Flow, built from the same vectors as float32, rounds
the same positions to themselves.

Printed per case: whether it has a peak-selection tie (subsegment_cases.has_peak_tie) and, where this interpreter can
import the restatement, whether restate() equals the reference."""
import os
import sys
import tempfile
import warnings

warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import subsegment_cases as sc  # noqa: E402
from label_glue_cases import ShiftFlow  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
tmp = tempfile.mkdtemp(prefix="tf_ref_subseg_")
os.makedirs(os.path.join(tmp, "tobac_flow", "utils"))
for parts in (("__init__.py",), ("utils", "__init__.py")):
    open(os.path.join(tmp, "tobac_flow", *parts), "w").close()
for parts in (("label.py",), ("utils", "label_utils.py")):
    with open(os.path.join(REFERENCE, "tobac_flow", *parts)) as f:
        src = f.read()
    with open(os.path.join(tmp, "tobac_flow", *parts), "w") as f:
        f.write("from __future__ import annotations\n" + src)
sys.path.insert(0, tmp)
import skimage  # noqa: E402
from tobac_flow.label import flow_label as ref_flow_label, subsegment_labels as ref_subsegment_labels  # noqa: E402

assert skimage.__version__.startswith("0.18"), skimage.__version__


try:
    restate = sc.restate
    restate(sc.make_pixel())
except Exception as e:  # noqa: BLE001
    print("restatement not available here:", repr(e))
    restate = None


def small(labels):
    assert labels.min() >= 0 and labels.max() < 2 ** 15
    return labels.astype(np.int16 if labels.max() > 255 else np.uint8)


out = {"skimage_version": np.array(skimage.__version__), "numpy_version": np.array(np.__version__),
       "flow/note": np.array("flow_label ran with a stand-in for Flow whose convolve shifts by the stored integer-valued "
                             "flows: a nearest-neighbour remap by such flows is exact")}
free, equal = {}, 0
for volume, make in sc.GENERATORS.items():
    mask = make()
    assert mask.dtype == bool and mask.ndim == 3 and not mask.all(axis=(1, 2)).any()
    out[f"mask/{volume}/bits"] = sc.pack(mask)
    out[f"mask/{volume}/shape"] = np.array(mask.shape, np.int32)
    for shrink, distance in sc.GRID:
        labels = ref_subsegment_labels(mask, shrink_factor=shrink, peak_min_distance=distance)
        out[sc.case_key(volume, shrink, distance)] = small(labels)
        tie = sc.has_peak_tie(mask, shrink, distance)
        free[volume] = free.get(volume, 0) + (not tie)
        same = None if restate is None else bool(np.array_equal(restate(mask, shrink, distance), labels))
        equal += bool(same)
        assert tie or same is not False, (volume, shrink, distance, "tie-free, yet the restatement differs")
        print(f"{volume} {mask.shape} shrink {shrink} min_distance {distance}: {int(labels.max())} labels, "
              f"{int(((labels == 0) & mask).sum())} px unlabelled, tie: {tie}, restatement equal: {same}")
print("tie-free cases per volume:", free, "of", len(sc.GRID), "each;", sum(free.values()), "of", len(sc.CASES), "in all;",
      "restatement equal in", equal)
assert all(n >= 3 for n in free.values()) and 2 * sum(free.values()) >= len(sc.CASES)

mask, forward, backward = sc.make_flow_case()
p = sc.FLOW_PARAMS
subseg = ref_subsegment_labels(mask != 0, shrink_factor=p["subsegment_shrink"], peak_min_distance=p["peak_min_distance"])
with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    linked = ref_flow_label(ShiftFlow(forward, backward), mask, overlap=p["overlap"], absolute_overlap=p["absolute_overlap"],
                            subsegment_shrink=p["subsegment_shrink"], peak_min_distance=p["peak_min_distance"])
tie = sc.has_peak_tie(mask, p["subsegment_shrink"], p["peak_min_distance"])
print(f"flow case {mask.shape}: {int(subseg.max())} subsegments -> {int(linked.max())} objects, tie: {tie}, "
      f"warnings: {[str(w.message) for w in caught]}")
assert not tie and linked.dtype == np.int32 and 1 < linked.max() < subseg.max()
if restate is not None:
    assert np.array_equal(restate(mask, p["subsegment_shrink"], p["peak_min_distance"]), subseg)
out["flow/mask/bits"], out["flow/mask/shape"] = sc.pack(mask), np.array(mask.shape, np.int32)
out["flow/forward"], out["flow/backward"] = forward, backward
out["flow/subseg"], out["flow/labels"] = small(subseg), small(linked)

path = os.path.join(HERE, "subsegment_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("wrote", path, size, "bytes")
assert size < 250_000, "the fixture must stay as small as ellipse_ref.npz"
