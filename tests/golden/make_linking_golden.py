"""Generate tests/golden/linking_ref.npz: the expected values of the second stage (tobac_flow_amd/linking.py) on the cases
of tests/linking_cases.py.  Run by hand where a checkout of the reference exists (python 3.10, numpy and SciPy as recorded
in the fixture wrote the committed file):

    python tests/golden/make_linking_golden.py <path to the reference checkout>

As make_label_glue_golden.py does, it executes the reference's files (tobac_flow/linking.py, utils/label_utils.py,
utils/datetime_utils.py) from a temporary package outside this tree, each with ONE prepended line
(``from __future__ import annotations``) and empty stand-in modules for what they import and these calls never touch
(xarray, skimage, tobac_flow.dataset).  Only data is written into the repository.

What the REFERENCE itself computes here, on duck-typed datasets (`.t`, `.core` / `.anvil` with `.max().item()`, `.values`,
`.dtype`; `.core_label` / `.thick_anvil_label` with `.sel(t=...)`, `.values`, `.dtype`): find_overlaps,
find_overlap_between_cores / _anvils, find_new_labels, remap_labels(new_labels=...), get_dates_from_filename.  The
functions that need a real xarray object -- process_linking_output, get_*_label_map_for_file, the merges, process_file,
increment_step_coords -- are recorded from the line-by-line restatement of tests/linking_cases.py.  `source/<function>`
says for every function which of the two wrote its arrays.

The script asserts, and fails where one does not hold: every reference call returned without a warning; restatement and
reference agree wherever both ran; on the three-window worlds the linked, relabelled and merged partition equals the
global labelling's (label_glue_cases.canonical_partition) and the merge filled something; the frame-count edges give pairs
with 3 common frames and none with 2, 1, 0; the file stays under 250 000 bytes."""
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import label_glue_cases as gc  # noqa: E402
import linking_cases as lc  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
tmp = tempfile.mkdtemp(prefix="tf_ref_linking_")
os.makedirs(os.path.join(tmp, "tobac_flow", "utils"))
for parts in (("__init__.py",), ("utils", "__init__.py")):
    open(os.path.join(tmp, "tobac_flow", *parts), "w").close()
for parts in (("linking.py",), ("utils", "label_utils.py"), ("utils", "datetime_utils.py")):
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
import tobac_flow.linking as ref_linking  # noqa: E402
import tobac_flow.utils.datetime_utils as ref_datetime  # noqa: E402
import tobac_flow.utils.label_utils as ref_utils  # noqa: E402

assert all(m.__file__.startswith(tmp) for m in (ref_linking, ref_datetime, ref_utils))
warnings.simplefilter("error")


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


class Duck:
    """a product as the reference's find_overlap_between_cores / _anvils read it"""

    def __init__(self, product):
        self.t = product["coords"]["t"]
        self.core, self.anvil = Coordinate(product["coords"]["core"]), Coordinate(product["coords"]["anvil"])
        for name, _ in lc.VOLUMES:
            setattr(self, name, Variable(product[name], self.t))


def small(a):
    a = np.asarray(a)
    if a.dtype.kind not in "iu" or a.min(initial=0) < 0 or a.max(initial=0) >= 2 ** 15:
        return a                                              # strings, flags, times in nanoseconds
    return a.astype(np.int16 if a.max(initial=0) > 255 else np.uint8)


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), f"restatement != reference: {what}"


out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__)}
source = {name: "restatement" for name in lc.NEW_FUNCTIONS}
source.update({name: "reference" for name in ("find_overlaps", "find_overlap_between_cores", "find_overlap_between_anvils",
                                              "find_new_labels", "relabel_cores_and_anvils", "get_dates_from_filename")})
source["relabel_cores_and_anvils"] = "reference: remap_labels(values, new_labels=map) with the restatement's maps"
source["find_overlap_between_files"] = "reference: find_overlap_between_cores / _anvils; the dict is the restatement's"
for name, who in source.items():
    out[f"source/{name}"] = np.array(who)

n_pairs = {}
for case, (names, store) in lc.chains().items():
    results, links = lc.np_link_chain(names, store)
    # find_overlap_between_cores / _anvils, find_new_labels: the reference
    for i, (a, b) in enumerate(zip(names[:-1], names[1:])):
        for kind, fn in (("core", ref_linking.find_overlap_between_cores), ("anvil", ref_linking.find_overlap_between_anvils)):
            lo, hi, x, y = fn(Duck(store[a]), Duck(store[b]))
            assert (lo, hi) == results[i][kind][:2]
            same(f"{case} pair {i} {kind} x", results[i][kind][2], x)
            same(f"{case} pair {i} {kind} y", results[i][kind][3], y)
            out[f"{case}/overlap/{i}/{kind}/minmax"] = np.array([lo, hi], np.int32)
            out[f"{case}/overlap/{i}/{kind}/x"], out[f"{case}/overlap/{i}/{kind}/y"] = small(x), small(y)
            n_pairs[case, kind] = n_pairs.get((case, kind), 0) + len(x)
    for kind in ("core", "anvil"):
        start = links[kind + "_start"]
        x = np.concatenate([o[kind][2] + s for o, s in zip(results, start)])
        y = np.concatenate([o[kind][3] + s for o, s in zip(results, start[1:])])
        same(f"{case} find_new_labels {kind}", links[kind + "_labels"],
             ref_linking.find_new_labels(x, y, links[kind + "_labels"].size).astype(np.int32))
    for key, value in lc.flatten_product(f"{case}/links", links).items():
        out[key] = small(value)
    for j, name in enumerate(names):
        start, end = ref_datetime.get_dates_from_filename(name)
        assert (start, end) == lc.np_get_dates_from_filename(name)
        out[f"{case}/dates/{j}"] = np.array([np.datetime64(start, "ns"), np.datetime64(end, "ns")]).astype(np.int64)
        maps = {"core": lc.np_get_core_label_map_for_file(name, links), "anvil": lc.np_get_anvil_label_map_for_file(name, links)}
        for kind, label_map in maps.items():
            out[f"{case}/map/{j}/{kind}"] = small(label_map)
        plain = lc.np_relabel_and_merge_file(name, links, store, merge=False)
        merged = lc.np_relabel_and_merge_file(name, links, store)
        for volume, kind in lc.VOLUMES:
            same(f"{case} relabel {j} {volume}", plain[volume], ref_utils.remap_labels(store[name][volume], new_labels=maps[kind]))
            out[f"{case}/relabel/{j}/{volume}"], out[f"{case}/merge/{j}/{volume}"] = small(plain[volume]), small(merged[volume])
    print(f"{case}: {len(names)} products, pairs {n_pairs[case, 'core']} core / {n_pairs[case, 'anvil']} anvil, "
          f"{int(links['core_labels'].max())} cores, {int(links['anvil_labels'].max())} anvils")
    if case in lc.WORLDS:
        processed = [lc.np_process_file(name, links, store) for name in names]
        for j, ds in enumerate(processed):
            for key, value in lc.flatten_product(f"{case}/process/{j}", ds).items():
                out[key] = small(value)
        shifted = lc.np_increment_step_coords({"coords": {k: v.copy() for k, v in processed[1]["coords"].items()}}, processed[0])
        for key in ("core_step", "thick_anvil_step", "thin_anvil_step"):
            out[f"{case}/increment/{key}"] = small(shifted["coords"][key])
        lc.merged_partition_check(case)
        print(f"  {case}: merged partition equals the global labelling's; process_file keeps "
              f"{[int(ds['coords']['core'].size) for ds in processed]} cores, {[int(ds['coords']['anvil'].size) for ds in processed]} anvils")

assert n_pairs["time/common3", "anvil"] > 0 and n_pairs["time/gap", "anvil"] > 0
assert all(n_pairs[f"time/common{k}", kind] == 0 for k in (2, 1, 0) for kind in ("core", "anvil"))
assert n_pairs["rule/quotient_edge", "core"] == 0 and n_pairs["rule/over_zero", "core"] == 1 and n_pairs["rule/mostly_outside", "core"] == 0
# (quotient_edge: 7 / 25 = 0.28 < the fixed rtol 0.5; the (atol, rtol) grid below moves the rule across its edges)

# find_overlaps on the rule cases' regions, every (atol, rtol) of label_glue_cases' grids: the reference
for name in lc.RULE_CASES:
    left, right, grid = gc.window_cases()[name]
    max_label = int(right.max())
    label_counts = np.maximum(np.bincount(right.ravel(), minlength=max_label + 1), 1)
    rows = []
    for g, (atol, rtol) in enumerate(grid):
        for ident in np.unique(left[left > 0]):
            x = right[left == ident]
            found = ref_linking.find_overlaps(x, atol, rtol, max_label, label_counts)
            same(f"find_overlaps {name} {atol} {rtol} {ident}", lc.np_find_overlaps(x, atol, rtol, max_label, label_counts), found)
            rows += [(g, int(ident), int(m)) for m in found]
    out[f"find_overlaps/{name}"] = np.array(rows, np.int16).reshape(-1, 3)
    want = gc.fixture()[f"window/{name}/pairs"].astype(np.int16).reshape(-1, 3)
    assert np.array_equal(out[f"find_overlaps/{name}"], want), "differs from label_glue_ref.npz"

path = os.path.join(HERE, "linking_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("wrote", path, size, "bytes,", len(out), "arrays")
assert size < 250_000, "the fixture must stay under 250 000 bytes"
