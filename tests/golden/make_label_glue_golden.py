"""Generate tests/golden/label_glue_ref.npz from the REFERENCE ITSELF: the label glue of tobac_flow/utils/label_utils.py
(flat_label, make_step_labels, slice_labels, relabel_objects, remap_labels, find_overlapping_labels,
get_step_labels_for_label), tobac_flow/label.py (flow_label, flow_link_overlap) and tobac_flow/linking.py (find_overlaps,
find_overlap_between_cores / _anvils, find_new_labels) on the cases of tests/label_glue_cases.py.  Run by hand where a
checkout of the reference exists (python 3.10, numpy and SciPy as recorded in the fixture wrote the committed file):

    python tests/golden/make_label_glue_golden.py <path to the reference checkout>

It executes the reference's three files from a temporary package outside this tree, each with ONE prepended line
(``from __future__ import annotations``), with empty stand-in modules for what they import and these cases never touch
(skimage -- flow_label with subsegment_shrink = 0 does not subsegment --, xarray, tobac_flow.dataset,
tobac_flow.utils.datetime_utils).  Only data is written into the repository.

flow_label and flow_link_overlap only need an object with `.convolve`; label_glue_cases.ShiftFlow shifts by the stored
INTEGER-VALUED flows, which is what a nearest-neighbour remap by such flows does exactly.  find_overlap_between_cores /
_anvils get duck-typed datasets (`.t`, `.core` / `.anvil`, `.core_label` / `.thick_anvil_label` with `.sel(t=...)`,
`.values`, `.dtype`); their atol 5 and rtol 0.5 are fixed inside.  For the other (atol, rtol) pairs find_overlaps is
called through scipy.ndimage.labeled_comprehension once per left label, as those two functions call it.

The script asserts, and fails where one does not hold: every call returned without a warning; the decisive edges
(product_edge 1 object at 0.27 and 2 at 0.28; quotient_edge linked at (5, 0.28), not at (5, 0.29) or (8, 0.28);
absolute_edge differs between 6 and 7; visit_order equals the directed model and differs from the symmetric one -- the
order of the visit itself cannot change a result, label_glue_cases' docstring says why); at least half of the seeded
flow_label cases with T >= 2 give an object count strictly between 1 and the number of step labels; the dropped first and
last common frame matters in at least one window case; oracle.np_label and oracle.np_dataset, where importable, equal the
reference on every case; the file stays under 250 000 bytes."""
import os
import sys
import tempfile
import types
import warnings
from functools import partial

import numpy as np
import scipy
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import label_glue_cases as gc  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
tmp = tempfile.mkdtemp(prefix="tf_ref_label_glue_")
os.makedirs(os.path.join(tmp, "tobac_flow", "utils"))
for parts in (("__init__.py",), ("utils", "__init__.py")):
    open(os.path.join(tmp, "tobac_flow", *parts), "w").close()
for parts in (("label.py",), ("linking.py",), ("utils", "label_utils.py")):
    with open(os.path.join(REFERENCE, "tobac_flow", *parts)) as f:
        src = f.read()
    with open(os.path.join(tmp, "tobac_flow", *parts), "w") as f:
        f.write("from __future__ import annotations\n" + src)


def stand_in(name, *attributes):
    try:
        __import__(name)
        return
    except ImportError:
        pass
    module = types.ModuleType(name)
    for a in attributes:
        setattr(module, a, None)
    sys.modules[name] = module


sys.path.insert(0, tmp)
stand_in("skimage")
stand_in("skimage.segmentation", "watershed")
stand_in("skimage.feature", "peak_local_max")
stand_in("xarray", "Dataset", "DataArray", "open_dataset")
sys.modules["tobac_flow.dataset"] = types.ModuleType("tobac_flow.dataset")
for a in ("flag_edge_labels", "flag_nan_adjacent_labels", "add_step_labels", "add_label_coords", "link_cores_and_anvils",
          "link_step_labels"):
    setattr(sys.modules["tobac_flow.dataset"], a, None)
sys.modules["tobac_flow.utils.datetime_utils"] = types.ModuleType("tobac_flow.utils.datetime_utils")
for a in ("get_dates_from_filename", "trim_file_start_and_end"):
    setattr(sys.modules["tobac_flow.utils.datetime_utils"], a, None)
import tobac_flow.label as ref_label  # noqa: E402
import tobac_flow.linking as ref_linking  # noqa: E402
import tobac_flow.utils.label_utils as ref_utils  # noqa: E402

assert ref_label.__file__.startswith(tmp) and ref_linking.__file__.startswith(tmp) and ref_utils.__file__.startswith(tmp)
warnings.simplefilter("error")                    # a warning in a recorded call ("Not all regions present" above all) ends the run

try:
    from oracle import np_dataset, np_label
    np_label.flow_label(np.zeros((2, 3, 3, 2), np.float32), np.zeros((2, 3, 3, 2), np.float32), np.ones((2, 3, 3), bool))
except Exception as e:  # noqa: BLE001
    print("oracle not available here:", repr(e))
    np_label = np_dataset = None

# the number of groups a linking call opened: every group has its own label_stack list, alive until the call returns
_stacks = set()
_find_neighbour_labels = ref_label.find_neighbour_labels


def _counting(label, label_stack, *args, **kwargs):
    _stacks.add(id(label_stack))
    return _find_neighbour_labels(label, label_stack, *args, **kwargs)


ref_label.find_neighbour_labels = _counting


def small(a):
    a = np.asarray(a)
    assert a.min(initial=0) >= 0 and a.max(initial=0) < 2 ** 15
    return a.astype(np.int16 if a.max(initial=0) > 255 else np.uint8)


def same(name, got, want):
    assert got.shape == want.shape and np.array_equal(got, want), f"the oracle differs from the reference: {name}"


out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__),
       "note": np.array("flow_label and flow_link_overlap ran with a stand-in for Flow whose convolve shifts by the stored "
                        "integer-valued (int8) flows: a nearest-neighbour remap by such flows is exact; flat_full, "
                        "flow_label and link are tables over the ids of the finer labelling (label_glue_cases.lut_of), "
                        "checked to reproduce the reference's volumes voxel for voxel")}
f32 = lambda v: v.astype(np.float32)

# ---- flat_label, flow_label --------------------------------------------------------------------------------------------
flow_cases = gc.flow_label_cases()
nontrivial = eligible = 0
for name, (mask, forward, backward, grid) in flow_cases.items():
    out[f"mask/{name}"], out[f"flows/{name}"] = gc.pack(mask), gc.pack_flows(forward, backward)
    assert forward.dtype == np.int8 and backward.dtype == np.int8 and forward.shape == mask.shape + (2,)
    flat = ref_utils.flat_label(mask)
    if name in gc.FLAT_CASES:
        flat_full = ref_utils.flat_label(mask, structure=gc.FULL.astype(int))
        assert flat.dtype == flat_full.dtype == np.int32
        out[f"flat/{name}"], out[f"flat_full/{name}"] = small(flat), small(gc.lut_of(flat, flat_full))
        if np_label is not None:
            same(f"flat_label {name}", np_label.flat_label(mask), flat)
            same(f"flat_label full {name}", np_label.flat_label(mask, gc.FULL.astype(int)), flat_full)
    counts, tables = [], []
    for overlap, absolute in grid:
        labels = ref_label.flow_label(gc.ShiftFlow(forward, backward), mask, overlap=overlap, absolute_overlap=absolute)
        assert labels.dtype == np.int32 and labels.shape == mask.shape
        tables.append(gc.lut_of(flat, labels))
        counts.append(int(labels.max()))
        if np_label is not None:
            same(f"flow_label {name} {overlap} {absolute}",
                 np_label.flow_label(f32(forward), f32(backward), mask, overlap=overlap, absolute_overlap=absolute), labels)
        if name in gc.SEEDED and mask.shape[0] >= 2:
            eligible += 1
            nontrivial += 1 < labels.max() < flat.max()
    if name not in gc.FLAT_CASES:
        out[f"flat/{name}"] = small(flat)
    out[f"flow_label/{name}"] = small(np.stack(tables))
    print(f"flow_label {name} {mask.shape}: {int(flat.max())} step labels -> objects {counts}")
print(f"non-trivial share: {nontrivial} of {eligible} seeded cases with T >= 2")
assert 2 * nontrivial >= eligible

key = lambda name, o, a: out[f"flow_label/{name}"][list(flow_cases[name][3]).index((o, a))][out[f"flat/{name}"]]
assert key("product_edge", 0.27, 0).max() == 1 and key("product_edge", 0.28, 0).max() == 2 and key("product_edge", 0.29, 0).max() == 2
assert key("absolute_edge", 0, 6).max() == 1 and key("absolute_edge", 0, 7).max() == 2
directed, symmetric = gc.check_visit_order()
visit = key("visit_order", 0, 0)
visit_flat = ref_utils.flat_label(flow_cases["visit_order"][0])
for label in range(1, int(visit_flat.max()) + 1):
    assert set(visit[visit_flat == label].tolist()) == {directed[label]}
assert any(visit[visit_flat == label][0] != symmetric[label] for label in symmetric)

# ---- find_overlapping_labels, label by label --------------------------------------------------------------------------------
for name in gc.OVERLAPPING_CASES:
    mask, forward, backward, _ = flow_cases[name]
    flat = ref_utils.flat_label(mask).astype(np.int32)
    back, fwd = gc.warped_labels(flat, forward, backward)
    bins, args = np.cumsum(np.bincount(flat.ravel())), np.argsort(flat.ravel())
    rows = []
    for i, (overlap, absolute) in enumerate(gc.overlapping_grid(name)):
        before = len(rows)
        for d, warped in enumerate((fwd, back)):
            for label in range(1, bins.size):
                locs = args[bins[label - 1]:bins[label]]
                found = ref_utils.find_overlapping_labels(warped, locs, bins, overlap=overlap, absolute_overlap=absolute)
                if np_label is not None:
                    assert list(found) == list(np_label.find_overlapping_labels(warped, locs, bins, overlap, absolute)), name
                rows += [(i, d, label, int(m)) for m in found]
        print(f"find_overlapping_labels {name} {overlap} {absolute}: {len(rows) - before} neighbours")
    out[f"overlapping/{name}"] = np.array(rows, np.int16).reshape(-1, 4)

# ---- label_utils on the tiled volumes ------------------------------------------------------------------------------------
steps = {}
for shape in gc.SHAPES:
    name = gc.shape_name(shape)
    labels = gc.tile_labels(shape)
    out[f"utils/{name}/labels"] = small(labels)
    step = ref_utils.make_step_labels(labels)
    steps[name] = step
    out[f"utils/{name}/make_step_labels"] = small(step)
    sliced = ref_utils.slice_labels(labels)
    out[f"utils/{name}/slice_labels"] = small(sliced)
    out[f"utils/{name}/relabel_objects"] = small(ref_utils.relabel_objects(gc.gappy(labels)))
    for form, (locations, new_labels) in gc.remap_arguments(labels).items():
        remapped = ref_utils.remap_labels(labels, locations, new_labels)
        out[f"utils/{name}/remap_{form}"] = small(remapped)
        if np_dataset is not None and form == "int":
            same(f"remap_labels {name}", np_dataset.remap_labels(labels, locations, new_labels), remapped)
    if np_dataset is not None:
        same(f"slice_labels {name}", np_dataset.slice_labels(labels), sliced)
    per_label = ref_utils.get_step_labels_for_label(labels, step)
    out[f"utils/{name}/steps_for_label/none"] = np.array([p is None for p in per_label])
    out[f"utils/{name}/steps_for_label/offsets"] = np.cumsum([0] + [0 if p is None else len(p) for p in per_label]).astype(np.int32)
    out[f"utils/{name}/steps_for_label/values"] = small(np.concatenate([np.zeros(0, np.int64)] + [p for p in per_label if p is not None]))
    print(f"label_utils {name}: {int(labels.max())} labels, {int(step.max())} step labels (make_step_labels), "
          f"{int(sliced.max())} (slice_labels)")

# ---- flow_link_overlap -------------------------------------------------------------------------------------------------------
for name, (flat, forward, backward, grid) in gc.link_cases(steps).items():
    if name == "gap_ids":
        out["link_input/gap_ids"], out["flows/gap_ids"] = small(flat), gc.pack_flows(forward, backward)
        assert set(np.unique(flat)) == {0, 1, 2, 4, 7}
    tables, opened = [], []
    for overlap, absolute in grid:
        _stacks.clear()
        linked = ref_label.flow_link_overlap(gc.ShiftFlow(forward, backward), flat, overlap=overlap, absolute_overlap=absolute)
        groups = len(_stacks)
        assert linked.dtype == np.int32 and groups >= linked.max()
        tables.append(gc.lut_of(flat, linked))
        opened.append(groups)
        if np_label is not None:
            same(f"flow_link_overlap {name} {overlap} {absolute}",
                 np_label.flow_link_overlap(f32(forward), f32(backward), flat, overlap=overlap, absolute_overlap=absolute), linked)
        print(f"flow_link_overlap {name} {overlap} {absolute}: {int(flat.max())} ids -> {int(linked.max())} objects, "
              f"{groups} groups opened")
    out[f"link/{name}"], out[f"link_groups/{name}"] = small(np.stack(tables)), small(opened)
assert gc.GAP_GRID == ((0, 0), (0, 12)) and out["link_groups/gap_ids"].tolist() == [6, 7] and out["link/gap_ids"].max(1).tolist() == [4, 7]


# ---- the window rule -------------------------------------------------------------------------------------------------------------
class Variable:
    def __init__(self, values, t):
        self.values, self.t, self.dtype = values, t, values.dtype

    def sel(self, t):
        at = np.searchsorted(self.t, t)
        assert np.array_equal(self.t[at], t)
        return Variable(self.values[at], self.t[at])


class Coordinate:
    def __init__(self, values):
        self.values, self.dtype = values, values.dtype

    def max(self):
        return self.values.max()


class Window:
    """a duck-typed dataset: `frames` (int32 labels) at the times t, as cores and as anvils"""

    def __init__(self, frames, t):
        ids = np.unique(frames[frames > 0]).astype(np.int32)
        self.t = t
        self.core = self.anvil = Coordinate(ids)
        self.core_label = self.thick_anvil_label = Variable(frames, t)


def reference_pairs(left, right, atol, rtol):
    """linking.py:58-86 with another (atol, rtol): find_overlaps through labeled_comprehension, once per left label"""
    index = np.unique(left[left > 0])
    max_label = int(right.max())
    label_counts = np.maximum(np.bincount(right.flatten(), minlength=max_label + 1), 1)
    comp = partial(ref_linking.find_overlaps, atol=atol, rtol=rtol, max_label=max_label, label_counts=label_counts)
    lists = ndi.labeled_comprehension(right.flatten(), left.flatten(), index, comp, list, [[]])
    x = np.repeat(index, [len(n) for n in lists])
    y = np.concatenate(lists, dtype=right.dtype, casting="unsafe")
    return np.stack([x, y], 1).astype(np.int64).reshape(-1, 2)


drop_matters = 0
for name, (left, right, grid) in gc.window_cases().items():
    assert left.dtype == right.dtype == np.int32 and left.shape == right.shape
    out[f"window/{name}/left"], out[f"window/{name}/right"] = small(left), small(right)
    n_left, n_right = int(left.max()), int(right.max())
    all_pairs, all_components = [], []
    for i, (atol, rtol) in enumerate(grid):
        if (atol, rtol) == (5, 0.5):
            # the reference's own entry points: two leading frames only the current window has, one trailing frame only
            # the next one has, and the first and last COMMON frame, which they drop
            wide_left, wide_right = gc.padded_window(left, right)
            P = wide_left.shape[0]
            zeros = lambda k: np.zeros((k,) + left.shape[1:], np.int32)
            current = Window(np.concatenate([zeros(2), wide_left]), np.arange(0, 2 + P))
            following = Window(np.concatenate([wide_right, zeros(1)]), np.arange(2, 3 + P))
            results = {}
            for kind, fn in (("cores", ref_linking.find_overlap_between_cores), ("anvils", ref_linking.find_overlap_between_anvils)):
                lo, hi, x, y = fn(current, following)
                assert (lo, hi) == (n_left, n_right) and x.dtype == np.int32
                results[kind] = np.stack([x, y], 1).astype(np.int64).reshape(-1, 2)
            assert np.array_equal(results["cores"], results["anvils"])
            pairs = results["cores"]
            assert np.array_equal(pairs, reference_pairs(left, right, atol, rtol))
            drop_matters += not np.array_equal(pairs, reference_pairs(wide_left, wide_right, atol, rtol))
        else:
            pairs = reference_pairs(left, right, atol, rtol)
        x, y = gc.node_ids(pairs[:, 0], pairs[:, 1], n_left)
        components = ref_linking.find_new_labels(x, y, n_left + n_right + 1)
        all_pairs.append(np.concatenate([np.full((len(pairs), 1), i), pairs], 1))
        all_components.append(components)
        if np_label is not None:
            ox, oy = np_label.link_overlap_pairs(left, right, atol, rtol)
            same(f"link_overlap_pairs {name} {atol} {rtol}", np.stack([ox, oy], 1).reshape(-1, 2), pairs)
            same(f"find_new_labels {name} {atol} {rtol}", np_label.find_new_labels(x, y, n_left + n_right + 1), components)
        print(f"window {name} ({atol}, {rtol}): {n_left} x {n_right} labels, {len(pairs)} pairs, "
              f"{int(components.max()) + 1} components")
    out[f"window/{name}/pairs"], out[f"window/{name}/components"] = small(np.concatenate(all_pairs)), small(np.stack(all_components))
print("cases in which the dropped first and last common frame matters:", drop_matters)
assert drop_matters >= 1
n_pairs = lambda name, grid, atol, rtol: int((out[f"window/{name}/pairs"][:, 0] == list(grid).index((atol, rtol))).sum())
linked = lambda atol, rtol: n_pairs("quotient_edge", gc.QUOTIENT_GRID, atol, rtol)
assert linked(5, 0.27) == linked(5, 0.28) == linked(7, 0.28) == linked(0, 0.28) == linked(0, 0.0) == 1
assert linked(5, 0.29) == linked(8, 0.28) == 0
assert np.array_equal(out["window/quotient_edge/pairs"][1], [1, 3, 2])
assert n_pairs("over_zero", gc.WINDOW_GRID, 5, 0.5) == 1 and n_pairs("mostly_outside", gc.WINDOW_GRID, 5, 0.5) == 0
assert n_pairs("mostly_outside", gc.WINDOW_GRID, 0, 0.3) == 1  # 12 / 40 == 0.3 over n; 12 / 80 over the right label's size

path = os.path.join(HERE, "label_glue_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("oracle compared:", np_label is not None, "| wrote", path, size, "bytes,", len(out), "arrays")
assert size < 250_000, "the fixture must stay under 250 000 bytes"
