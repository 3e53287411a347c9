"""Cases and expected values for the per-label weighted statistics and flag proportions (tobac_flow_amd.postprocess).

tests/golden/wstats_ref.npz holds inputs and the results of the reference's own functions (apply_func_to_labels with
weighted_stats, weighted_stats_and_uncertainties and get_weighted_proportions), written by tests/golden/make_wstats_golden.py.
What those functions compute is restated here in float64 with one plain loop per label; where an extreme occurs more than
once the restatement takes the smallest raveled index (the reference's unstable argsort leaves that open, so the fixture's
cases have no such ties and `tie_case` is held against the restatement only).  test_wstats_cases_cpu.py holds the
restatement against the fixture, the GPU tests compare the package with the restatement."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wstats_ref.npz")
CASES = ("A_f32_volume", "B_f64_plane")
SUMMED, SELECTED = (0, 1, 4, 5), (2, 3, 6, 7)                    # columns: mean, std, uncertainty, combined / min, max, their errors


@functools.lru_cache(maxsize=None)
def golden():
    """{case: {field: array}} and the metadata of the fixture; the arrays are shared and must not be written to"""
    z = np.load(GOLDEN)
    cases, meta = {}, {}
    for key in z.files:
        group, field = key.split("/")
        (meta if group == "meta" else cases.setdefault(group, {}))[field] = z[key]
    return cases, meta


def restate_stats(labels, x, e, w, index):
    """(len(index), 8) float64: mean, std, min, max, uncertainty of the mean, combined error, error at the minimum and at
    the maximum of every id, from the formulas of the contract; columns 4 .. 7 are NaN with e=None"""
    labels = np.asarray(labels)
    lab = labels.ravel()
    X = np.asarray(x, np.float64).ravel()
    W = np.broadcast_to(np.asarray(w, np.float64), labels.shape).ravel()
    E = None if e is None else np.asarray(e, np.float64).ravel()
    out = np.full((len(index), 8), np.nan)
    for k, i in enumerate(index):
        at = np.flatnonzero(lab == i)                             # ascending raveled index
        at = at[np.isfinite(X[at])]
        n = at.size
        if n == 0:
            continue
        xs, ws = X[at], W[at]
        sw = ws.sum()
        if not sw > 0:                                            # also a NaN sum
            continue
        mean = (ws * xs).sum() / sw
        var = (ws * (xs - mean) ** 2).sum() / sw
        c = 1 - (ws * ws).sum() / (sw * sw)
        with np.errstate(divide="ignore", invalid="ignore"):
            std = np.sqrt(np.float64(var) / np.float64(c)) if c >= 0 else np.nan
        lo, hi = np.argmin(xs), np.argmax(xs)                     # first occurrence = smallest raveled index; -0.0 == 0.0
        out[k, :4] = mean, std, xs[lo], xs[hi]
        if E is not None:
            es = E[at]
            unc = np.sqrt((ws * ws * (es * es)).sum()) / sw
            out[k, 4:] = unc, np.sqrt((std / np.sqrt(n)) ** 2 + unc ** 2), es[lo], es[hi]
    return out


def restate_proportions(labels, flags, w, flag_values, index):
    """(len(index), K) float64: the share of every id's non-NaN weight on each flag value; NaN rows without weight"""
    labels = np.asarray(labels)
    lab, F = labels.ravel(), np.asarray(flags).ravel()
    W = np.broadcast_to(np.asarray(w, np.float64), labels.shape).ravel()
    out = np.full((len(index), len(flag_values)), np.nan)
    for k, i in enumerate(index):
        at = np.flatnonzero(lab == i)
        at = at[~np.isnan(W[at])]
        total = W[at].sum()
        if not total > 0:
            continue
        for j, f in enumerate(flag_values):
            out[k, j] = W[at][F[at] == f].sum() / total
    return out


def tie_case():
    """A small volume in which every label's minimum and maximum occur several times, with a distinct error at every
    voxel: what is returned shows which voxel was chosen.  Label 2 has its minimum as +0.0 and then as -0.0 (one value
    for the ordering; the first of them is chosen).  Labels cross row ends, the 16-voxel and 256-voxel pieces of the
    kernel's work layout and the volume has a tail that is no multiple of 4."""
    shape = (3, 9, 23)
    n = int(np.prod(shape))
    i = np.arange(n)
    labels = np.where((i // 40) % 4 == 3, 0, 1 + (i // 150) % 4).astype(np.int32).reshape(shape)
    x = (10.0 + (i * 7) % 5).reshape(shape)                       # five values, each many times per label
    flat = x.ravel()
    two = np.flatnonzero(labels.ravel() == 2)
    flat[two] -= 10.0                                             # label 2: values 0 .. 4, so the minimum is a zero
    zeros = two[flat[two] == 0]
    flat[zeros[1::2]] = -0.0
    assert zeros.size >= 4 and np.signbit(flat[zeros[1]]) and not np.signbit(flat[zeros[0]])
    e = (1.0 + i / 1024.0).reshape(shape)                         # exact in float32 as well
    w = (0.5 + (i % 7) / 8.0).reshape(shape)
    return {"labels": labels, "x": x, "e": e, "w": w, "index": np.arange(1, 5)}


def with_dtype(case, dtype):
    """the field, errors and weights of a case as another float type (float32 values widen exactly)"""
    return dict(case, x=case["x"].astype(dtype), e=case["e"].astype(dtype), w=case["w"].astype(dtype))
