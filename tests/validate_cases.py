"""Cases and yardsticks of the validation stage (tobac_flow_amd.validation: validate_detection, the five validate_*
wrappers, flash_list, get_edge_filter_dev):

  * a (6, 37, 70) detection product -- cores, thick and thin anvils, anvil markers, `core_anvil_index` -- and a flash grid,
    laid out by hand so that every one of the five marker sets has a POD and a FAR strictly between 0 and 1;
  * a NumPy restatement of the five wrappers and of the script that calls them (scripts/dcc_validation.py:93-250), on the
    restatements of tests/validation_cases.py; tests/test_validate_cases_cpu.py holds it to the reference's own results
    in tests/golden/validate_ref.npz (written by tests/golden/make_validate_golden.py);
  * the footprint rule of tf_edge_filter's missing-data dilation as a small NumPy function, held to
    scipy.ndimage.binary_dilation with the reference's structure by the same CPU test."""
import os

import numpy as np

import validation_cases as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validate_ref.npz")
MARGIN, TIME_MARGIN = 4, 1
SHAPE = (6, 37, 70)
SETS = ("core", "core_with_anvil", "anvil", "anvil_with_core", "anvil_marker")
EDGE_MARGINS = (10, 7, 12, 5, 3)


# ---- the product -------------------------------------------------------------------------------------------------------
def _boxes(spec):
    v = np.zeros(SHAPE, np.int32)
    for label, (t0, t1, y0, y1, x0, x1) in spec.items():
        v[t0:t1, y0:y1, x0:x1] = label
    return v


def product():
    """{name: array}: the label volumes (int32), the coordinates `core` (1 .. 8), `anvil` (1 .. 7), `anvil_marker`
    (1 .. 6) and `core_anvil_index`.  With MARGIN, TIME_MARGIN = 4, 1 the edge filter keeps frames 1 .. 4, rows 4 .. 32,
    columns 4 .. 65.  Cores 4, 6 and 8 point at no anvil (index 0); no core points at anvils 5, 6, 7; core 8, anvil 7 and
    anvil marker 6 occur in no volume (the script cuts them from the coordinates); anvil 6 occurs in the thin volume only
    (it stays, and is absent from the thick volume the anvils are validated on); core 5, anvils 4 and 5 and anvil marker 4
    touch a border or an end frame."""
    anvils = {1: (1, 4, 6, 16, 8, 24), 2: (1, 5, 20, 30, 30, 46), 3: (2, 5, 8, 14, 50, 62), 4: (0, 3, 22, 32, 5, 15),
              5: (3, 5, 5, 12, 60, 70)}
    cores = {1: (1, 3, 9, 12, 12, 16), 2: (2, 4, 10, 13, 18, 21), 3: (2, 4, 23, 26, 35, 39), 4: (3, 5, 15, 18, 55, 58),
             5: (0, 2, 25, 28, 8, 11), 6: (1, 3, 30, 33, 40, 44), 7: (3, 5, 9, 12, 52, 56)}
    markers = {1: (1, 3, 8, 14, 10, 20), 2: (2, 4, 22, 28, 33, 42), 3: (3, 5, 9, 13, 51, 58), 4: (4, 6, 15, 20, 20, 26),
               5: (2, 3, 30, 32, 60, 64)}
    thick = _boxes(anvils)
    thin = thick.copy()
    thin[3:4, 30:33, 20:26] = 6
    return {"core_label": _boxes(cores), "thick_anvil_label": thick, "thin_anvil_label": thin,
            "anvil_marker_label": _boxes(markers), "core": np.arange(1, 9, dtype=np.int32),
            "anvil": np.arange(1, 8, dtype=np.int32), "anvil_marker": np.arange(1, 7, dtype=np.int32),
            "core_anvil_index": np.array([1, 1, 2, 0, 4, 0, 3, 0], np.int32)}


def flash_grid():
    """float64 flash counts 0 .. 3.  Inside the edge filter: two flashes in core 1, one in core 3, three in core 6 (two
    pixels below anvil 2), one two pixels above anvil 2 and away from every core, one away from everything, and one in
    frame 3 at squared distance 5 from both core 1 and core 2 in frame 2 (inside anvil 1 and anvil marker 1): there the
    closest core is a choice.  Outside it: flashes in frame 0, in a border row and in frame 5, and a NaN count in the
    border, as regrid_glm may leave one."""
    g = np.zeros(SHAPE, np.float64)
    g[1, 10, 13], g[3, 24, 36], g[2, 31, 42], g[1, 18, 45], g[4, 30, 64], g[3, 13, 16] = 2, 1, 3, 1, 1, 1
    g[0, 10, 10], g[2, 1, 30], g[5, 20, 20] = 2, 1, 3
    g[1, 0, 5] = np.nan
    return g


def flash_times():
    return vc.flash_times(SHAPE[0])


# ---- restatement of the five wrappers and of the script ----------------------------------------------------------------
def restate_subsets(p):
    """{set: (label volume, coordinate)} as the five wrappers select them (validation.py:233-234, 338-344, 456-457,
    569-574, 686-687)"""
    core, anvil, index = p["core"], p["anvil"], p["core_anvil_index"]
    with_anvil = core[index != 0]
    with_core = anvil[np.isin(anvil, np.unique(index))]
    sets = {"core": (p["core_label"], core),
            "core_with_anvil": (np.where(np.isin(p["core_label"], with_anvil), p["core_label"], 0), with_anvil),
            "anvil": (p["thick_anvil_label"], anvil),
            "anvil_with_core": (np.where(np.isin(p["thick_anvil_label"], with_core), p["thick_anvil_label"], 0), with_core)}
    if "anvil_marker" in p:
        sets["anvil_marker"] = (p["anvil_marker_label"], p["anvil_marker"])
    return sets


def restate_wrappers(p, glm_grid, glm_distance, edge_filter, n_glm_in_margin, margin, time_margin, get_closest):
    """{variable: (array of the reference's dtype, dims)} of the five validate_* wrappers"""
    out = {}
    for name, (labels, coord) in restate_subsets(p).items():
        dist, closest, marker_distance, pod, far, n_in, flag = vc.restate_validate_markers(
            labels, glm_grid, glm_distance, edge_filter, n_glm_in_margin, coord, margin, time_margin, get_closest)
        out[f"flash_{name}_distance"] = dist.astype(np.float32), ("flash",)
        if get_closest:
            out[f"flash_{name}_index"] = closest.astype(np.int32), ("flash",)
        out[f"{name}_glm_distance"] = marker_distance.astype(np.float32), (name,)
        out[f"{name}_pod"] = np.asarray(pod).astype(np.float32), ()
        out[f"{name}_far"] = np.asarray(far).astype(np.float32), ()
        out[f"{name}_count_in_margin"] = np.asarray(n_in).astype(np.int32), ()
        out[f"{name}_margin_flag"] = flag.astype(bool), (name,)
    return out


def cut_to_present(p):
    """scripts/dcc_validation.py:96-116: the three coordinates cut to the ids in their volumes, `core_anvil_index` with `core`"""
    q = dict(p)
    keep = np.isin(p["core"], np.unique(p["core_label"]))
    q["core"], q["core_anvil_index"] = p["core"][keep], p["core_anvil_index"][keep]
    q["anvil"] = p["anvil"][np.isin(p["anvil"], np.unique(p["thick_anvil_label"])) | np.isin(p["anvil"], np.unique(p["thin_anvil_label"]))]
    if "anvil_marker" in p:
        q["anvil_marker"] = p["anvil_marker"][np.isin(p["anvil_marker"], np.unique(p["anvil_marker_label"]))]
    return q


def restate_detection(p, grid, times, margin, time_margin, get_closest):
    """scripts/dcc_validation.py:93-250 without its files, for a grid without missing data"""
    grid = grid.copy()
    q = cut_to_present(p)
    glm_distance = vc.restate_cylinder(grid, time_margin)
    out = {"flash_count_total": (np.asarray(np.nansum(grid[grid > 0])).astype(np.int32), ())}
    edge = vc.restate_edge_filter(grid, times, margin, time_margin)
    grid[~edge] = 0
    n_in = np.nansum(grid)
    out["flash_count_in_margin"] = np.asarray(n_in).astype(np.int32), ()
    out.update(restate_wrappers(q, grid, glm_distance, edge, n_in, margin, time_margin, get_closest))
    return out


def script_inputs():
    """(glm_grid, glm_distance, edge_filter, n_glm_in_margin) as the script hands them to the wrappers"""
    grid = flash_grid()
    glm_distance = vc.restate_cylinder(grid, TIME_MARGIN)
    edge = vc.restate_edge_filter(grid, flash_times(), MARGIN, TIME_MARGIN)
    grid[~edge] = 0
    return grid, glm_distance, edge, np.nansum(grid)


def tie_flashes(labels, glm_grid, time_margin):
    """bool per flash: several labels lie at the minimal distance (the reported label is then a choice); with it the sets
    and values of validation_cases.brute_force gathered at the flashes, for validation_cases.in_set"""
    _, _, sets, values = vc.brute_force(labels, time_margin)
    at = np.repeat(sets.ravel(), glm_grid.astype(int).ravel())
    return (at != 0) & ~vc.single_label(at), at, values


# ---- the footprint of the missing-data dilation ------------------------------------------------------------------------
def reference_structure(margin, time_margin):
    """the structure of validation.py:197-213, in its own words"""
    return np.stack([np.sum([(arr - 10) ** 2 for arr in np.meshgrid(np.arange(margin * 2 + 1), np.arange(margin * 2 + 1))], 0) ** 0.5
                     < margin] * (time_margin * 2 + 1), 0)


def footprint_dilation(missing, margin, time_margin):
    """tf_edge_filter's rule: output (t, y, x) is set exactly when some voxel (k, y - dy, x - dx) of `missing` is, with
    |k - t| <= time_margin, |dy|, |dx| <= margin and (dx + margin - 10)^2 + (dy + margin - 10)^2 < margin^2"""
    T, H, W = missing.shape
    m = margin
    window = np.zeros_like(missing)
    for t in range(T):
        window[t] = missing[max(t - time_margin, 0):t + time_margin + 1].any(0)
    out = np.zeros_like(missing)
    for dy in range(-m, m + 1):
        for dx in range(-m, m + 1):
            if (dx + m - 10) ** 2 + (dy + m - 10) ** 2 >= m * m:
                continue
            # out[:, y, x] |= window[:, y - dy, x - dx]
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yr, xr = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            if ys.start < ys.stop and xs.start < xs.stop:
                out[:, ys, xs] |= window[:, yr, xr]
    return out


def missing_cases(shape=(5, 37, 70)):
    """{name: float64 grid}: -1 at a corner, on a border, in the interior, as one whole frame, absent, and a NaN that is
    not -1"""
    def grid(**at):
        g = np.zeros(shape, np.float64)
        g[1, 20, 30] = 2
        for where in at.values():
            g[where] = -1
        return g
    cases = {"corner": grid(a=(2, 0, 0)), "border": grid(a=(1, shape[1] - 1, 33)), "interior": grid(a=(3, 18, 35)),
             "frame": grid(a=(2, slice(None), slice(None))), "absent": grid()}
    cases["nan"] = grid()
    cases["nan"][2, 15, 15] = np.nan
    return cases


_GOLDEN = None


def golden():
    """{case: {name: array}} of tests/golden/validate_ref.npz"""
    global _GOLDEN
    if _GOLDEN is None:
        z = np.load(GOLDEN)
        _GOLDEN = {}
        for k in z.files:
            case, name = k.split("/")
            _GOLDEN.setdefault(case, {})[name] = z[k]
    return _GOLDEN
