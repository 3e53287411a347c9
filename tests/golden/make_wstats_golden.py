"""Generate tests/golden/wstats_ref.npz from the REFERENCE ITSELF: per-label weighted statistics, their uncertainties and
flag proportions.  Run by hand where a checkout of the reference exists:

    python tests/golden/make_wstats_golden.py <path to the reference checkout>

It loads the reference's tobac_flow/utils/stats_utils.py and tobac_flow/utils/label_utils.py by path (stats_utils imports
xarray at module level and never uses it in the functions called here, so an empty module stands in for it), calls the
reference's apply_func_to_labels with weighted_stats, weighted_stats_and_uncertainties and
partial(get_weighted_proportions, flag_values=...), and stores inputs and results.  Only data is written to the repository.

Two volumes from the region recipe of tests/props_cases.volumes, each with regions across the 16-voxel and 4096-voxel
boundaries of the kernel's work layout and across row ends; (5, 33, 67) has a tail that is no multiple of 16 (6 x 40 x 50 =
12 000 is one).  Case A: float32 operands, weights as a volume.  Case B: float64 operands, weights as one (H, W) plane.
Both hold the special labels listed in `specials` below.  The script asserts that every label's minimum and maximum occur
once, which keeps the reference's undefined tie order out of the fixture, and records the largest relative difference
between the reference's float32 results and the float64 restatement of tests/wstats_cases.py as meta/max_rel_f32."""
import importlib.util
import os
import sys
import types
import warnings
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import props_cases  # noqa: E402
import wstats_cases  # noqa: E402

warnings.filterwarnings("ignore")
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.modules.setdefault("xarray", types.ModuleType("xarray"))


def load(name):
    path = os.path.join(sys.argv[1], "tobac_flow", "utils", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


ref_stats, ref_labels = load("stats_utils"), load("label_utils")
FLAG_VALUES = np.array([0, 1, 2, 4])                             # 4 never occurs; the flags also hold 5, which is not listed


def region_volume(shape, first_seed):
    """the thin-anvil volume of the first seed whose regions cross a 4096-voxel boundary, a 16-voxel boundary and a row end"""
    for seed in range(first_seed, first_seed + 50):
        labels = props_cases.volumes(seed, shape)[2]
        flat = labels.ravel()
        n = flat.size
        inside = lambda step: any(flat[i] != 0 and flat[i] == flat[i - 1] for i in range(step, n, step))  # noqa: E731
        if inside(4096) and inside(16) and inside(shape[2]) and labels.max() >= 12:
            return seed, labels.copy()
    raise RuntimeError("no seed gives the wanted region layout")


def specials(labels, x, e, w_of, rng):
    """Writes the special cases into the inputs; w_of(t, y, x) -> a view of the weights at those voxels' positions (the
    volume itself, or the plane under them).  Returns {what: label id}.  Labels are taken in ascending size so that the
    large regions keep ordinary values."""
    ids, counts = np.unique(labels[labels > 0], return_counts=True)
    by_size = [int(i) for i in ids[np.argsort(counts, kind="stable")] if counts[ids == i][0] >= 4]
    used = {}

    def take(what):
        used[what] = by_size.pop(0)
        return np.nonzero(labels == used[what])

    t, y, xx = take("all_nonfinite")
    x[t, y, xx] = np.resize([np.nan, np.inf, -np.inf], t.size)
    t, y, xx = take("zero_weight")
    w_of()[(t, y, xx) if w_of().ndim == 3 else (y, xx)] = 0
    t, y, xx = take("nan_weight")
    w_of()[(t[0], y[0], xx[0]) if w_of().ndim == 3 else (y[0], xx[0])] = np.nan
    t, y, xx = take("one_weighted_voxel")
    w_of()[(t[1:], y[1:], xx[1:]) if w_of().ndim == 3 else (y[1:], xx[1:])] = 0
    # the lone weight is a power of two: then w x / w == x exactly in every float type, the variance is 0 and std is the
    # contract's 0 / 0 = NaN; with another weight the quotient can round one ulp off x and std is a / 0 = inf instead --
    # in the reference's float32 as in any other arithmetic (the one-voxel label below has weight 1 for the same reason)
    w_of()[(t[0], y[0], xx[0]) if w_of().ndim == 3 else (y[0], xx[0])] = 2.0
    t, y, xx = take("extreme_at_zero_weight")
    x[t[0], y[0], xx[0]] = x[np.isfinite(x)].max() + 7
    w_of()[(t[0], y[0], xx[0]) if w_of().ndim == 3 else (y[0], xx[0])] = 0
    t, y, xx = take("absent")
    labels[t, y, xx] = 0
    # non-finite values and a NaN error inside the two largest regions
    big = [int(i) for i in ids[np.argsort(counts, kind="stable")][-2:]]
    t, y, xx = np.nonzero(labels == big[0])
    pick = rng.choice(t.size, 6, replace=False)
    x[t[pick], y[pick], xx[pick]] = [np.inf, -np.inf, np.nan, np.nan, np.inf, -np.inf]
    t, y, xx = np.nonzero(labels == big[1])
    e[t[5], y[5], xx[5]] = np.nan
    used["nan_error"] = big[1]
    # a one-voxel label on the background
    free = np.argwhere(labels == 0)
    t0, y0, x0 = free[len(free) // 2]
    used["one_voxel"] = int(labels.max()) + 1
    labels[t0, y0, x0] = used["one_voxel"]
    w_of()[(t0, y0, x0) if w_of().ndim == 3 else (y0, x0)] = 1.0
    # the special labels are what they are meant to be after ALL writes (plane pixels are shared between labels)
    weight_at = lambda what: np.broadcast_to(w_of(), labels.shape)[labels == used[what]]     # noqa: E731
    value_at = lambda what: x[labels == used[what]]                                           # noqa: E731
    assert not np.isfinite(value_at("all_nonfinite")).any()
    assert np.isfinite(value_at("zero_weight")).all() and (weight_at("zero_weight") == 0).all()
    assert np.isnan(weight_at("nan_weight")).sum() >= 1 and np.isfinite(value_at("nan_weight")).all()
    assert (weight_at("one_weighted_voxel") > 0).sum() == 1 and (weight_at("one_weighted_voxel") >= 0).all()
    assert np.isfinite(value_at("extreme_at_zero_weight")).all()
    assert weight_at("extreme_at_zero_weight")[np.argmax(value_at("extreme_at_zero_weight"))] == 0
    assert weight_at("extreme_at_zero_weight").sum() > 0
    return used


def make_case(shape, first_seed, dtype, plane):
    seed, labels = region_volume(shape, first_seed)
    rng = np.random.default_rng(100 + seed)
    import scipy.ndimage as ndi
    smooth = ndi.gaussian_filter(rng.normal(size=shape), (0.5, 1.5, 1.5))
    x = (220.0 + 60.0 * smooth + rng.random(shape)).astype(dtype)             # one sign, like a brightness temperature
    e = (0.5 + rng.random(shape)).astype(dtype)
    w = (1.0 + rng.random(shape[1:] if plane else shape)).astype(dtype)       # like a pixel area
    used = specials(labels, x, e, lambda: w, rng)
    top = int(labels.max())
    index = rng.permutation(np.concatenate([np.arange(1, top + 1), [top + 3, top + 9]])).astype(np.int32)
    flags = rng.choice(np.array([0, 1, 2, 5], np.int8), size=shape, p=[0.4, 0.3, 0.2, 0.1])
    flags = np.where(ndi.gaussian_filter(rng.normal(size=shape), 1.5) > 0, flags, np.int8(1)).astype(np.int8)   # runs of equal flags
    # the proportions kernel reads float32 weights (NaN and zeros kept); the reference is given the same values widened to
    # float64, so that its np.nansum of them is a float64 sum and the fixture carries no float32 summation error
    wf = w.astype(np.float32)
    case = {"labels": labels, "x": x, "e": e, "w": w, "index": index, "flags": flags, "flag_values": FLAG_VALUES, "wf": wf}
    case["special_ids"] = np.array([used[k] for k in sorted(used)], np.int32)
    case["special_names"] = np.array(sorted(used))
    # every label's extremes occur once
    for i in range(1, top + 1):
        v = x[labels == i]
        v = v[np.isfinite(v)]
        if v.size:
            assert (v == v.min()).sum() == 1 and (v == v.max()).sum() == 1, f"label {i} has a tied extreme"
    wb = np.broadcast_to(w, shape)
    case["stats8"] = np.asarray(ref_labels.apply_func_to_labels(
        labels, x, e, wb, func=ref_stats.weighted_stats_and_uncertainties, index=index, default=[np.nan] * 8)).T
    case["stats4"] = np.asarray(ref_labels.apply_func_to_labels(
        labels, x, wb, func=ref_stats.weighted_stats, index=index, default=[np.nan] * 4)).T
    case["proportions"] = np.asarray(ref_labels.apply_func_to_labels(
        labels, flags, np.broadcast_to(wf.astype(np.float64), shape), func=partial(ref_stats.get_weighted_proportions, flag_values=FLAG_VALUES),
        index=index, default=np.asarray([np.nan] * len(FLAG_VALUES)))).T
    assert case["stats8"].shape == (index.size, 8) and case["proportions"].shape == (index.size, FLAG_VALUES.size)
    return case


cases = {"A_f32_volume": make_case((6, 40, 50), 3, np.float32, False),
         "B_f64_plane": make_case((5, 33, 67), 4, np.float64, True)}
worst = {}
for name, c in cases.items():
    mine = wstats_cases.restate_stats(c["labels"], c["x"], c["e"], c["w"], c["index"])
    ref = c["stats8"].astype(np.float64)
    assert np.array_equal(np.isnan(mine), np.isnan(ref)), name
    ok = ~np.isnan(ref)
    rel = np.abs(mine - ref)[ok] / np.abs(ref[ok])
    worst[name] = float(np.where(np.isin(np.nonzero(ok)[1], wstats_cases.SUMMED), rel, 0).max())
    rows = {k: int(np.isnan(ref[:, k]).sum()) for k in (0, 1, 4)}
    print(name, "ids", c["index"].size, "largest region", int(np.bincount(c["labels"].ravel())[1:].max()),
          "NaN rows mean/std/uncertainty", rows, "max rel diff of the summed values", worst[name],
          "specials", dict(zip(c["special_names"].tolist(), c["special_ids"].tolist())))
out = {f"{name}/{k}": v for name, c in cases.items() for k, v in c.items()}
out["meta/max_rel_f32"] = np.float64(worst["A_f32_volume"])
out["meta/max_rel_f64"] = np.float64(worst["B_f64_plane"])
path = os.path.join(HERE, "wstats_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
