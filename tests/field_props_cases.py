"""Cases and expected values for the fifth stage (tobac_flow_amd.postprocess: get_cre, add_cre_to_dataset,
cloud_quality_weights, add_weighted_stats_of_fields, add_cloud_properties, add_flux_properties; tf_label_wstats_multi).

tests/golden/cre_ref.npz holds seeded float32 and float64 inputs and the results of the reference's OWN add_cre_to_dataset
on them, written by tests/golden/make_cre_golden.py.  What the reference's functions and the two script sections
(scripts/postprocess_seviri_nat_dcc.py:180-215 and :271-298) compute is restated here line by line with NumPy; the
statistics are restated in float64 by wstats_cases.restate_stats.  test_field_props_cases_cpu.py holds the restatement
against the fixture; the GPU tests compare the package with the restatement and with its own composed calls.

Every value of every case is a float32 number, so a case as float64 holds the same reals (the derived fluxes still differ
between the two types: they are rounded in the field type)."""
import functools
import os

import numpy as np

import wstats_cases as wc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cre_ref.npz")
DIMS = ("core_step", "thick_anvil_step", "thin_anvil_step")
TOA_PLANES = ("toa_swdn", "toa_swup", "toa_swup_clr", "toa_lwup", "toa_lwup_clr")
BOA_PLANES = ("boa_swdn", "boa_swup", "boa_lwdn", "boa_lwup", "boa_swdn_clr", "boa_swup_clr", "boa_lwdn_clr", "boa_lwup_clr")
RAW = TOA_PLANES + BOA_PLANES
CRE_NAMES = ("toa_swup_cre", "toa_lwup_cre", "boa_swdn_cre", "boa_swup_cre", "boa_lwdn_cre", "boa_lwup_cre",
             "toa_net", "toa_net_cre", "boa_net", "boa_net_cre")
TOA_FIELDS = ("toa_swdn", "toa_swup", "toa_swup_cre", "toa_lwup", "toa_lwup_cre", "toa_net", "toa_net_cre")
BOA_FIELDS = ("boa_swdn", "boa_swdn_cre", "boa_swup", "boa_swup_cre", "boa_lwdn", "boa_lwdn_cre", "boa_lwup", "boa_lwup_cre",
              "boa_net", "boa_net_cre")
FLUX_VARIABLES = TOA_FIELDS + BOA_FIELDS + ("lts", "fth", "cbh")                 # postprocess_seviri_nat_dcc.py:274-295
CLOUD_VARIABLES = ("cot", "cer", "cwp", "ctp", "ctp_corrected", "cth", "cth_corrected", "ctt", "ctt_corrected", "stemp", "dem")
CLOUD_FLAGS = {"lsflag": (0, 1), "lusflag": (0, 1, 2), "illum": (1, 2, 3), "cldtype": (0, 1, 2, 3, 4), "phase": (0, 1, 2)}
WITH_UNCERTAINTY = ("cot", "cer", "ctp", "cth", "ctt", "stemp", "fth")
# the shapes at which the walk can go wrong: a workgroup takes 4096 voxels, a lane 4 x 4 voxels 256 apart
SHAPES = ((1, 1, 1), (2, 32, 64), (3, 37, 41), (5, 64, 96))
EXACT, SUMMED = (2, 3, 6, 7), (0, 1, 4, 5)                        # columns of restate_stats: min, max, their errors / the sums


def bits_equal(a, b):
    """equal element by element as IEEE values with the sign of a zero told apart and NaN equal to NaN.  The sign and
    payload of a NaN are NOT compared: IEEE 754 leaves them open and the hardware differs (inf - inf is the NaN with the
    sign bit set on x86 and the one without on the GPU); every other value has one bit pattern only."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])
                and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


# ---- add_cre_to_dataset -------------------------------------------------------------------------------------------------------
def cre_inputs(dtype):
    """the thirteen raw planes, seeded: random fluxes (a regrouped expression tree rounds about a third of them
    differently), and planted NaN, inf - inf, inf + inf, -0.0 and exact cancellation"""
    rng = np.random.default_rng(20240613)
    shape = (3, 6, 9)
    out = {}
    for k, name in enumerate(RAW):
        a = rng.normal(150.0, 220.0, shape).astype(np.float32)
        flat = a.reshape(-1)
        flat[(7 * k + 3) % flat.size] = np.nan
        out[name] = a
    for name in ("toa_swup", "toa_swup_clr", "boa_lwdn", "boa_lwdn_clr"):
        out[name][1, 2, 3] = np.inf                               # inf - inf in two cre fields; inf + inf in the nets
    out["boa_swup"][2, 0, 0] = -np.inf
    for name in ("boa_swdn", "boa_swdn_clr"):
        out[name][0, 0, 1] = 812.25                               # exact cancellation: +0.0
    out["toa_lwup"][0, 1, 1], out["toa_lwup_clr"][0, 1, 1] = -0.0, 0.0
    return {name: a.astype(dtype) for name, a in out.items()}


def restate_cre(ds):
    """get_cre and add_cre_to_dataset (tobac_flow/postprocess.py:29-99) line by line on a name -> ndarray mapping: the ten
    new variables in the order the reference adds them"""
    new = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for var in ("toa_swup", "toa_lwup", "boa_swdn", "boa_swup", "boa_lwdn", "boa_lwup"):
            new[f"{var}_cre"] = ds[var] - ds[f"{var}_clr"]
        new["toa_net"] = ds["toa_swdn"] - (ds["toa_swup"] + ds["toa_lwup"])
        new["toa_net_cre"] = -(new["toa_swup_cre"] + new["toa_lwup_cre"])
        new["boa_net"] = ds["boa_swdn"] + ds["boa_lwdn"] - (ds["boa_swup"] + ds["boa_lwup"])
        new["boa_net_cre"] = new["boa_swdn_cre"] + new["boa_lwdn_cre"] - (new["boa_swup_cre"] + new["boa_lwup_cre"])
    return new


@functools.lru_cache(maxsize=None)
def golden():
    """{"float32" / "float64": {"in": {name: array}, "out": {name: array}}}, the names in the reference's order and the
    provenance line; the arrays are shared and must not be written to"""
    z = np.load(GOLDEN)
    names = [str(n) for n in z["meta/names"]]
    cases = {}
    for dtype in ("float32", "float64"):
        cases[dtype] = {"in": {n: z[f"{dtype}/in/{n}"] for n in RAW}, "out": {n: z[f"{dtype}/out/{n}"] for n in names}}
    return cases, names, str(z["meta/provenance"])


# ---- the quality weights ---------------------------------------------------------------------------------------------------------
def restate_quality_weights(weights, qcflag, cth, cot):
    """postprocess_seviri_nat_dcc.py:181-186 on NumPy arrays"""
    with np.errstate(invalid="ignore"):
        return weights * (qcflag == 0).astype(np.float32) * (cth < 30).astype(np.float32) * np.isfinite(cot).astype(np.float32)


def quality_case(shape, dtype, plane):
    """weights (a plane or a volume) with NaN, inf and 0 among them, qcflag, cth with NaN and the threshold itself, cot with
    NaN and inf: every combination of a special weight with a zero factor occurs where the volume is large enough"""
    rng = np.random.default_rng(99 + int(np.prod(shape)))
    n = int(np.prod(shape))
    w = rng.integers(1, 40, shape[1:] if plane else shape).astype(dtype) / 8
    wf = w.reshape(-1)
    wf[::7], wf[3::11], wf[5::13] = np.nan, np.inf, 0
    qcflag = np.where(rng.random(shape) < 0.3, rng.integers(1, 4, shape), 0).astype(np.int16)
    cth = rng.integers(0, 45, shape).astype(np.float32)
    cth.reshape(-1)[::5], cth.reshape(-1)[1::9] = np.nan, 30
    cot = rng.integers(0, 100, shape).astype(np.float32) / 8
    cot.reshape(-1)[2::6], cot.reshape(-1)[4::17] = np.nan, np.inf
    want = restate_quality_weights(w, qcflag, cth, cot)
    if n >= 4096:
        full = np.broadcast_to(w, shape)
        zero = (qcflag != 0) | ~(cth < 30) | ~np.isfinite(cot)
        assert (np.isnan(full) & zero).any() and (np.isinf(full) & zero).any() and (np.isinf(full) & ~zero).any()
        assert np.isnan(want[np.isinf(full) & zero]).all() and (want[np.isfinite(full) & zero] == 0).all()
        assert (np.isnan(cth) & (qcflag == 0) & np.isfinite(cot) & np.isfinite(full)).any()
    assert want.shape == tuple(shape) and want.dtype == (np.float32 if dtype == np.float32 else np.float64)
    return {"weights": w, "qcflag": qcflag, "cth": cth, "cot": cot, "want": want}


# ---- the statistics ------------------------------------------------------------------------------------------------------------
# planted labels (volumes of >= 4096 voxels)
L_MASK, L_ALLNAN, L_INFINF, L_NANW, L_W0, L_TIES, L_CONST, L_SINGLE, L_ABSENT = 5, 6, 7, 8, 9, 10, 38, 39, 40
ID_ABOVE, ID_NEGATIVE = 45, -3


def _labels(shape, variant):
    """About 40 ids as rectangles a quarter of the rows high and a fifth of the columns wide, ids 1 .. 20 in even frames and
    21 .. 40 in odd ones: runs along rows that continue 256 voxels (some rows) further down.  Background stripes, one id
    above the largest requested one, one negative id, id 40 absent, id 39 a single voxel.  `variant` 1 and 2 shift the
    pattern (the three step-label volumes of a dataset)."""
    T, H, W = shape
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    y, x = (y + 3 * variant) % H, (x + 5 * variant) % W
    lab = (1 + (t % 2) * 20 + (y * 4 // H) * 5 + (x * 5 // W)).astype(np.int32)
    lab[(x % 11 == 10) | (y % 13 == 12)] = 0
    lab[lab == L_ABSENT] = 0
    single = np.flatnonzero(lab.reshape(-1) == L_SINGLE)
    if single.size > 1:
        lab.reshape(-1)[single[1:]] = 0
    if lab.size >= 4096:
        flat = lab.reshape(-1)
        flat[np.flatnonzero(flat == 0)[[2, 9]]] = ID_ABOVE, ID_NEGATIVE
    return lab


def _voxels(labels, label):
    return np.flatnonzero(labels.reshape(-1) == label)


@functools.lru_cache(maxsize=None)
def stats_case(shape, plane):
    """One seeded case as float32 arrays: three label volumes with their scrambled indices, the thirteen raw flux planes,
    lts / fth / cbh, the eleven cloud variables (dem as int16), uncertainties for WITH_UNCERTAINTY, five flags, and the
    weights as a float32 plane or volume.  Shared: the arrays must not be written to.  For volumes of >= 4096 voxels
    every plant is asserted here."""
    rng = np.random.default_rng(7 + int(np.prod(shape)) + int(plane))
    big = int(np.prod(shape)) >= 4096
    labels = {dim: _labels(shape, k) for k, dim in enumerate(DIMS)}
    index = {dim: rng.permutation(np.arange(1, L_ABSENT + 1)) for dim in DIMS} if big else {dim: np.array([2, 1]) for dim in DIMS}
    lab = labels[DIMS[0]]
    fields = {}
    for name in RAW + ("lts", "fth", "cbh") + CLOUD_VARIABLES:
        fields[name] = np.round(rng.normal(0.0, 200.0, shape) * 8).astype(np.float32) / 8      # signed
    for name in WITH_UNCERTAINTY:
        fields[f"{name}_uncertainty"] = rng.integers(1, 64, shape).astype(np.float32) / 16
    fields["dem"] = rng.integers(-50, 3000, shape).astype(np.int16)
    for name, values in CLOUD_FLAGS.items():
        fields[name] = rng.integers(0, max(values) + 2, shape).astype(np.int8)
    w = rng.integers(1, 16, shape[1:] if plane else shape).astype(np.float32) / 4
    if big:
        flat = {name: a.reshape(-1) for name, a in fields.items()}
        every = [n for n in fields if fields[n].dtype == np.float32]
        at = lambda label, k: int(_voxels(lab, label)[k])                                       # noqa: E731
        wflat = w.reshape(-1)
        hw = shape[1] * shape[2]
        windex = (lambda v: v % hw) if plane else (lambda v: v)
        # the per-field mask: a NaN in one _clr plane where every other plane is finite
        flat["toa_swup_clr"][at(L_MASK, 3)] = np.nan
        flat["boa_swup_clr"][at(L_MASK, 4)] = np.nan
        # a label all-NaN in one plane, finite in the others
        for name in ("toa_lwup_clr", "boa_lwup_clr", "cbh", "cwp"):
            flat[name][_voxels(lab, L_ALLNAN)] = np.nan
        # inf - inf in a derived field
        for name in ("toa_swup", "toa_swup_clr", "boa_lwdn", "boa_lwdn_clr"):
            flat[name][at(L_INFINF, 2)] = np.inf
        # a NaN weight under one label
        wflat[windex(at(L_NANW, 1))] = np.nan
        # a weight-0 voxel holding the extreme of every field
        v = at(L_W0, 5)
        wflat[windex(v)] = 0
        for name in every:
            flat[name][v] = 6000.0 if "clr" not in name else -6000.0
        # tied extremes: the largest and the smallest value twice, raw and (through swup - swup_clr) derived
        ties = _voxels(lab, L_TIES)
        for name in every:
            if "uncertainty" not in name:
                flat[name][ties[[1, 6]]], flat[name][ties[[2, 4]]] = 5000.0, -5000.0
        flat["toa_swup_clr"][ties[[1, 6]]] = flat["boa_swup_clr"][ties[[1, 6]]] = -4000.0
        # one label whose fields are constant (raw and therefore derived)
        for k, name in enumerate(every):
            if "uncertainty" not in name:
                flat[name][_voxels(lab, L_CONST)] = 12.5 + k
        flat["dem"][_voxels(lab, L_CONST)] = 777
        _assert_plants(lab, fields, np.broadcast_to(w, shape))
    return {"shape": shape, "plane": plane, "labels": labels, "index": index, "fields": fields, "weights": w}


def _assert_plants(lab, fields, w):
    derived = restate_cre(fields)
    get = lambda name: (derived[name] if name in derived else fields[name]).reshape(-1)        # noqa: E731
    wf = w.reshape(-1)
    v = _voxels(lab, L_MASK)
    assert np.isnan(get("toa_swup_clr")[v]).sum() == 1 and np.isfinite(get("toa_swup")[v]).all()
    assert np.isnan(get("toa_swup_cre")[v]).sum() == 1 and np.isnan(get("toa_net_cre")[v]).sum() == 1
    assert np.isfinite(get("toa_net")[v]).all() and np.isnan(get("boa_net_cre")[v]).sum() == 1
    v = _voxels(lab, L_ALLNAN)
    assert v.size > 1 and np.isnan(get("toa_lwup_cre")[v]).all() and np.isnan(get("boa_net_cre")[v]).all() and np.isnan(get("cbh")[v]).all()
    assert np.isfinite(get("toa_lwup")[v]).all() and np.isfinite(get("toa_net")[v]).all() and np.isfinite(get("lts")[v]).all()
    v = _voxels(lab, L_INFINF)
    assert (np.isinf(get("toa_swup")[v]) & np.isinf(get("toa_swup_clr")[v]) & np.isnan(get("toa_swup_cre")[v])).sum() == 1
    assert (np.isinf(get("boa_lwdn")[v]) & np.isnan(get("boa_lwdn_cre")[v])).sum() == 1
    assert np.isnan(wf[_voxels(lab, L_NANW)]).any() and np.isfinite(get("toa_swdn")[_voxels(lab, L_NANW)]).all()
    v = _voxels(lab, L_W0)
    for name in ("toa_swdn", "toa_swup_cre", "boa_lwup_cre", "lts", "cot"):
        assert wf[v[np.nanargmax(get(name)[v])]] == 0, name
    v = _voxels(lab, L_TIES)
    for name in ("toa_swdn", "toa_swup_cre", "boa_swup_cre", "fth", "cer"):
        x = get(name)[v]
        assert (x == np.nanmax(x)).sum() >= 2, name
    assert (get("toa_swdn")[v] == np.nanmin(get("toa_swdn")[v])).sum() >= 2
    v = _voxels(lab, L_CONST)
    assert v.size > 2 and all(np.ptp(get(name)[v]) == 0 for name in ("toa_swdn", "toa_net_cre", "boa_net", "cbh", "dem"))
    assert _voxels(lab, L_SINGLE).size == 1 and _voxels(lab, L_ABSENT).size == 0
    assert _voxels(lab, ID_ABOVE).size == 1 and _voxels(lab, ID_NEGATIVE).size == 1
    assert (get("toa_swup_cre") < 0).any() and (get("toa_swup_cre") > 0).any()                # signed


def case_fields(case, dtype):
    """name -> array of the case with its float32 arrays as `dtype` (exact), everything else as it is"""
    return {n: (a.astype(dtype) if a.dtype == np.float32 else a) for n, a in case["fields"].items()}


def set_fields(fields, names):
    """the named variables as arrays: raw ones as they are, derived ones by the restated reference, in the fields' type"""
    derived = restate_cre(fields)
    return [derived[n] if n in derived else fields[n] for n in names]


def restate_with_bounds(labels, x, e, w, index):
    """(stats, bounds): wstats_cases.restate_stats in float64, and per id what the bounds of the summed columns need, all
    from this side: n, scale = sum |w x| / sum w, xmax = max |x| and the Bessel factor c over the finite values"""
    stats = wc.restate_stats(labels, x, e, w, index)
    lab, X = np.asarray(labels).ravel(), np.asarray(x, np.float64).ravel()
    W = np.broadcast_to(np.asarray(w, np.float64), np.shape(labels)).ravel()
    bounds = np.full((len(index), 4), np.nan)
    for k, i in enumerate(index):
        at = np.flatnonzero(lab == i)
        at = at[np.isfinite(X[at])]
        if at.size == 0:
            continue
        sw = W[at].sum()
        if not sw > 0:
            continue
        bounds[k] = at.size, np.abs(W[at] * X[at]).sum() / sw, np.abs(X[at]).max(), 1 - (W[at] ** 2).sum() / sw ** 2
    return stats, bounds


def check_stats(got, want, bounds, constant=None, what="", rounding=0.0):
    """`got` (len(index), 4 or 8) against the float64 restatement: the NaN pattern of every column and the exact columns
    (min, max, the errors at them) equal; the mean within 8 n 2^-53 sum|w x| / sum w (both sides sum n products in double
    in some order: (4 n + 1) 2^-53 to first order; signed terms need this absolute form); std, mean uncertainty and
    combined error within rtol 1e-9 (non-negative terms; the mean's perturbation enters the squared deviations in second
    order), on the condition asserted here that std >= 1e-6 max|x| for every label of n >= 2 but the constant one, which
    is held on both sides by std <= 8 n 2^-53 |x| / sqrt(c).
    `rounding`: the relative rounding error of the type the values were stored in -- 2^-24 for the float32 columns a stage
    function writes for a float32 field, where `got` is a double within the bounds above rounded once to float32: the
    bound b on a summed value then becomes b + rounding (|want| + b).  The exact columns are field values and unaffected."""
    n_out = got.shape[1]
    want = want[:, :n_out]
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN pattern"
    exact = [k for k in EXACT if k < n_out]
    assert np.array_equal(got[:, exact], want[:, exact], equal_nan=True), what + ": min / max / errors at them"
    n, scale, xmax, c = bounds.T
    ok = ~np.isnan(want[:, 0])
    b = 8 * n[ok] * 2.0 ** -53 * scale[ok]
    assert np.all(np.abs(got[ok, 0] - want[ok, 0]) <= b + rounding * (np.abs(want[ok, 0]) + b)), what + ": mean"
    rows = np.ones(len(want), bool)
    if constant is not None:
        rows[constant] = False
        for side in (got, want):
            if not np.isnan(want[constant, 1]):
                b = 8 * n[constant] * 2.0 ** -53 * xmax[constant] / np.sqrt(c[constant])
                assert side[constant, 1] <= b * (1 + rounding), what + ": constant label"
    spread = rows & ok & (n >= 2) & ~np.isnan(want[:, 1])
    assert np.all(want[spread, 1] >= 1e-6 * xmax[spread]), what + ": the case's condition std >= 1e-6 max|x|"
    for k in (1, 4, 5):
        if k < n_out:
            sel = rows if k == 1 else np.ones(len(want), bool)
            np.testing.assert_allclose(got[sel, k], want[sel, k], rtol=1e-9 + rounding * (1 + 1e-9), atol=0, equal_nan=True,
                                       err_msg=f"{what}: column {k}")


def check_pair(got, other, want, bounds, constant=None, what="", rounding=0.0):
    """two evaluations by the package (fused and composed) against each other: the exact columns and the NaN pattern equal,
    the summed ones within the bounds of check_stats, which hold between any two orders of summation"""
    assert got.shape == other.shape, what
    check_stats(got, want, bounds, constant, what, rounding)
    check_stats(other, want, bounds, constant, what + " (composed)", rounding)
    exact = [k for k in EXACT if k < got.shape[1]]
    assert np.array_equal(got[:, exact], other[:, exact], equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(other)), what


# ---- the two script sections ------------------------------------------------------------------------------------------------------
def restate_stage(labels, index, fields, weights, variables, dims=DIMS):
    """The loop of postprocess_seviri_nat_dcc.py:190-205 / :274-298 in float64:
    {f"{dim}_{var}": (restate_stats columns, bounds)} in the order of insertion, and the names the loop adds in its order.
    `fields` holds every variable (the derived fluxes too: restate_cre first, as the script does)."""
    out, names = {}, []
    for var in variables:
        e = fields.get(f"{var}_uncertainty")
        for dim in dims:
            out[f"{dim}_{var}"] = restate_with_bounds(labels[dim], fields[var], e, weights, index[dim])
            names += [f"{dim}_{var}_{s}" for s in ("mean", "std", "min", "max")]
            if e is not None:
                names += [f"{dim}_{var}_{s}" for s in ("mean_uncertainty", "mean_combined_error", "min_error", "max_error")]
    return out, names


def restate_flux_section(labels, index, fields, weights, variables=FLUX_VARIABLES, dims=DIMS):
    """postprocess_seviri_nat_dcc.py:271-298: add_cre_to_dataset, then the loop over the twenty variables"""
    return restate_stage(labels, index, dict(fields, **restate_cre(fields)), weights, variables, dims)


def restate_cloud_section(labels, index, fields, weights, variables=CLOUD_VARIABLES, flags=CLOUD_FLAGS, dims=DIMS):
    """postprocess_seviri_nat_dcc.py:190-215: the statistics of the eleven variables, then the proportions of the five
    flags: (statistics as restate_stage, {f"{dim}_{flag}_proportion": array}, names in the order of insertion)"""
    stats, names = restate_stage(labels, index, fields, weights, variables, dims)
    proportions = {}
    for flag, values in flags.items():
        for dim in dims:
            proportions[f"{dim}_{flag}_proportion"] = wc.restate_proportions(labels[dim], fields[flag], weights, values, index[dim])
            names.append(f"{dim}_{flag}_proportion")
    return stats, proportions, names


def stat_columns(ds, prefix, n_out):
    """the columns a stage function wrote for f"{dim}_{var}" as a (len(index), n_out) float64 array"""
    names = ("mean", "std", "min", "max", "mean_uncertainty", "mean_combined_error", "min_error", "max_error")[:n_out]
    return np.stack([np.asarray(ds[f"{prefix}_{s}"], np.float64) for s in names], 1)
