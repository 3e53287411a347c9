"""Generate tests/golden/objects_ref.npz: the expected values of the third stage (utils/stats_utils.py *_groupby,
utils/filter_utils.py, utils/xarray_utils.sel_*, postprocess.process_*_properties, add_validity_flags) on the cases of
tests/objects_cases.py.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_objects_golden.py <path to the reference checkout>

As make_linking_golden.py does, it executes the reference's utils/stats_utils.py from a temporary package outside this
tree, with ONE prepended line (``from __future__ import annotations``) and an empty stand-in module for xarray, which the
calls made here never touch.  Only data is written into the repository.

What the REFERENCE itself computes here, per group on the group's values in record order (float32 columns upcast first,
as the package evaluates them): calc_combined_mean, calc_combined_std, weighted_average_uncertainty -- the values of
combined_mean_groupby, combined_std_groupby and weighted_average_uncertainty_groupby.  Everything that needs a real
xarray object (the groupby itself, argmin / argmax / idx*, differentiate, the filters, sel_*, process_*) is recorded from
the restatement of tests/objects_cases.py.  `source/<name>` says for every function which of the two wrote its arrays.

The script asserts, and fails where one does not hold: the reference's values lie within the stated bounds of the
restatement's exactly rounded ones; every criterion of filter_cores and filter_anvils removes at least one object of the
world and most objects survive neither filter alone; the file stays under 1 000 000 bytes."""
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import objects_cases as oc  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
REFERENCE = sys.argv[1]
tmp = tempfile.mkdtemp(prefix="tf_ref_objects_")
os.makedirs(os.path.join(tmp, "tobac_flow_ref"))
open(os.path.join(tmp, "tobac_flow_ref", "__init__.py"), "w").close()
with open(os.path.join(REFERENCE, "tobac_flow", "utils", "stats_utils.py")) as f:
    src = f.read()
with open(os.path.join(tmp, "tobac_flow_ref", "stats_utils.py"), "w") as f:
    f.write("from __future__ import annotations\n" + src)
try:
    import xarray  # noqa: F401
except ImportError:
    sys.modules["xarray"] = types.ModuleType("xarray")
    sys.modules["xarray"].DataArray = None
sys.path.insert(0, tmp)
import tobac_flow_ref.stats_utils as ref  # noqa: E402

assert ref.__file__.startswith(tmp)
warnings.simplefilter("error")


def ticks(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype.kind in "mM" else a


out = {"numpy_version": np.array(np.__version__)}
source = {name: "restatement" for name in oc.STATS_NAMES + oc.FILTER_NAMES + oc.SEL_NAMES + oc.PROCESS_NAMES}
for name in ("calc_combined_mean", "calc_combined_std", "combined_mean_groupby", "combined_std_groupby",
             "weighted_average_uncertainty_groupby"):
    source[name] = "reference"
for name, who in source.items():
    out[f"source/{name}"] = np.array(who)

REFERENCE_CALLS = {
    "combined_mean_groupby": lambda c, m: ref.calc_combined_mean(c["m"][m], c["w"][m]),
    "combined_std_groupby": lambda c, m: ref.calc_combined_std(c["s"][m], c["m"][m], c["w"][m]),
    "weighted_average_uncertainty_groupby": lambda c, m: ref.weighted_average_uncertainty(c["e"][m], c["w"][m]),
}
for case in oc.FIXTURE_TABLES:
    table = oc.record_table(**oc.KERNEL_TABLES[case])
    found = oc.members(table["ids"], table["coord"])
    for k, (values, _) in enumerate(oc.np_group_reduce(table["ids"], table["coord"], oc.all_ops(table), found)):
        out[f"table/{case}/op/{k}"] = values
    wide = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in table.items()}
    for name in oc.GROUPBY_NAMES:
        values, bounds = oc.np_groupby(name, table)
        if name in REFERENCE_CALLS:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")                   # the reference divides by a zero weight sum where it is one
                theirs = np.array([REFERENCE_CALLS[name](wide, m) for m in found], np.float64)
            excess = oc.close(theirs, values, bounds)
            assert excess <= 0, f"{case} {name}: the reference lies {excess} beyond the bound"
            values = theirs
        out[f"groupby/{case}/{name}"] = ticks(values)
    print(f"{case}: {table['ids'].size} records, {table['coord'].size} groups")

for world_name, kwargs in oc.WORLDS.items():
    criteria, stages = {}, {}
    ds = oc.np_remove_orphan_coords(oc.world(**kwargs))
    n_cores, n_anvils = ds.coords["core"].size, ds.coords["anvil"].size
    ds = oc.np_filter_cores(ds, criteria=criteria)
    oc.np_filter_anvils(oc.np_process(ds, "core", "core", rates=True), criteria=criteria)
    final = oc.np_chain(oc.world(**kwargs), stages)
    if world_name == "full":
        assert all(v.any() for v in criteria.values()), {k: int(v.sum()) for k, v in criteria.items()}
        assert all(v.sum() < v.size / 2 for v in criteria.values())
    for stage, table in stages.items():
        for dim, coord in table.coords.items():
            out[f"world/{world_name}/{stage}/coords/{dim}"] = coord
    for name, value in final.items():
        out[f"world/{world_name}/final/{name}"] = ticks(value)
    picked = oc.np_sel_core(stages["remove_orphan_coords"], stages["remove_orphan_coords"].coords["core"][[3, 7, 8]])
    for dim, coord in picked.coords.items():
        out[f"world/{world_name}/sel_core/coords/{dim}"] = coord
    picked = oc.np_sel_anvil(stages["remove_orphan_coords"], stages["remove_orphan_coords"].coords["anvil"][[1, 4]])
    for dim, coord in picked.coords.items():
        out[f"world/{world_name}/sel_anvil/coords/{dim}"] = coord
    print(f"{world_name}: {n_cores} cores / {n_anvils} anvils -> {final.coords['core'].size} / {final.coords['anvil'].size}, "
          f"{len(final)} variables; removed by criterion {({k: int(v.sum()) for k, v in criteria.items()})}")

path = os.path.join(HERE, "objects_ref.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print("wrote", path, size, "bytes,", len(out), "arrays")
assert size < 1_000_000, "the fixture must stay under 1 000 000 bytes"
