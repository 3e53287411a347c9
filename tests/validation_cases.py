"""Cases and yardsticks of the GLM validation (tobac_flow_amd.validation, ndimage_dev.distance_transform_edt_frames):

  * the volumes: the smallest shapes at which the kernels can still go wrong (see each function);
  * a NumPy / SciPy restatement of the five functions, held to the reference's own results in
    tests/golden/validation_ref.npz by tests/test_validation_cases_cpu.py;
  * brute force: per voxel the exact integer squared distance to the nearest feature, how many features lie at exactly
    that distance, and which labels they carry -- the sets the tie contract is checked against.

The contract on ties: distances are unique, the nearest feature is not.  A result must be a feature at
exactly the minimal distance, must equal the reference wherever only one label lies at that distance, and must be the
same in every run; which of several equally near features SciPy reports follows its Voronoi sweep and is not reproduced."""
import os
import warnings
from types import SimpleNamespace

import numpy as np
import scipy.ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validation_ref.npz")
MARGIN, TIME_MARGIN = 4, 1                                        # of the validate_markers / get_edge_filter cases


# ---- volumes -----------------------------------------------------------------------------------------------------------
def boxes():
    """(6, 37, 70) int32: labelled boxes, several per frame, ids that persist over frames; frames 2 and 5 are empty.
    Label 9 lives in frame 4 only (where the flash grid below is empty: it lies over an inf distance)."""
    rng = np.random.default_rng(11)
    v = np.zeros((6, 37, 70), np.int32)
    for t in (0, 1, 3, 4):
        for k in range(4):
            label = 1 + (2 * t + k) % 8
            y0, x0 = int(rng.integers(0, 33)), int(rng.integers(0, 62))
            v[t, y0:y0 + int(rng.integers(1, 7)), x0:x0 + int(rng.integers(1, 10))] = label
    v[4, 20:23, 30:34] = 9
    return v


def borders():
    """(4, 33, 300) int32: a row longer than one workgroup; features in the four corners and along the borders only"""
    v = np.zeros((4, 33, 300), np.int32)
    v[:, 0, 0], v[:, 0, -1], v[:, -1, 0], v[:, -1, -1] = 1, 2, 3, 4
    v[1, 0, ::7] = 5
    v[2, ::5, -1] = 6
    v[3, -1, 3::11] = 7
    v[3, 1::4, 0] = 8
    return v


def single():
    """(3, 70, 37) int32: ONE feature in a corner of frame 0 (full-row scans, the largest distance); frame 1 is all
    features (every distance 0); frame 2 is empty"""
    v = np.zeros((3, 70, 37), np.int32)
    v[0, -1, -1] = 3
    v[1] = -1
    return v


def degenerate():
    """(2, 1, 130) and (2, 65, 1) float32 with a NaN feature: one row, one column"""
    rng = np.random.default_rng(5)
    a = (rng.random((2, 1, 130)) < 0.05).astype(np.float32)
    b = (rng.random((2, 65, 1)) < 0.08).astype(np.float32)
    a[0, 0, 77], b[1, 40, 0] = np.nan, np.nan
    return a, b


def wide():
    """(1, 64, 5424) bool: sparse features on the product's row length (the row pass holds it in LDS)"""
    rng = np.random.default_rng(9)
    return rng.random((1, 64, 5424)) < 2e-4


def very_wide():
    """(1, 2, 16500) uint8: a row beyond the 16384 columns the row pass holds in LDS (it then scans the workspace)"""
    rng = np.random.default_rng(10)
    return (rng.random((1, 2, 16500)) < 1e-3).astype(np.uint8)


def regions():
    """(4, 64, 512) int32 labels and a float64 field for the per-label minimum: regions that span whole waves of the
    kernel's work layout (1024 consecutive voxels), so that the wave-wide combine of equal labels runs, beside stripes one
    voxel wide, a region that ends inside a wave, small boxes and background.  Label 4's values are all NaN, label 6 lies
    over inf, -0.0 and +0.0 both occur, and id 11 is absent."""
    rng = np.random.default_rng(17)
    v = np.zeros((4, 64, 512), np.int32)
    v[0], v[1, :40] = 1, 1
    v[1, 40:, :300] = 2
    v[2, :, :256], v[2, :, 256:] = 3, 4
    v[2, ::2, 100:101] = 5
    v[3, 10:30, 17:401] = 6
    v[3, 40:44, 5:9], v[3, 50:51, 500:512] = 7, 8
    field = np.round(rng.normal(size=v.shape) * 64) / 8
    field[rng.random(v.shape) < 0.05] = np.nan
    field[v == 4] = np.nan
    field[v == 6] = np.inf
    field[0, 0, :2] = [0.0, -0.0]
    return v, field, np.array([3, 11, 1, 8, 4, 2, 7, 6, 5], np.int64)


def flash_grid(shape=(6, 37, 70)):
    """float64 flash counts 0 .. 3, sparse, frame 4 without a flash; one NaN voxel in the border that the edge filter
    clears (scripts/dcc_validation.py:149-155 computes the distance first and zeroes the filtered voxels afterwards)"""
    rng = np.random.default_rng(21)
    g = np.where(rng.random(shape) < 0.006, rng.integers(1, 4, shape), 0).astype(np.float64)
    g[4] = 0
    g[1, 0, 5] = np.nan
    return g


def flash_times(n, gap_after=None):
    """datetime64[ns] times 300 s apart, with a gap of 1200 s after frame `gap_after`"""
    seconds = 300 * np.arange(n)
    if gap_after is not None:
        seconds[gap_after + 1:] += 900
    return np.datetime64("2018-06-19T17:00:00", "ns") + seconds.astype("timedelta64[s]").astype("timedelta64[ns]")


def label_index(labels):
    """every id of the volume in a shuffled order, with one that is absent from it"""
    ids = np.unique(labels[labels > 0])
    return np.random.default_rng(3).permutation(np.concatenate([ids, [int(ids.max()) + 2]])).astype(np.int64)


def distance_field_with_specials(labels, flashes):
    """(field, {what: id}): the per-frame flash distance under `labels`, NaN under every voxel of label 2; label 9 lies over
    the inf distance of the flash-free frame 4; the id beyond the largest label is absent"""
    field = restate_cylinder(flashes, 0)
    field[labels == 2] = np.nan
    assert np.isinf(field[labels == 9]).all() and (labels == 2).any()
    return field, {"all_nan": 2, "over_inf": 9, "absent": int(labels.max()) + 2}


# ---- restatement in NumPy / SciPy --------------------------------------------------------------------------------------
def _frames(markers, indices=False):
    """per frame: SciPy's distance to the nearest voxel != 0 (inf in a frame without one) and the value there (0)"""
    markers = np.asarray(markers)
    dist = np.full(markers.shape, np.inf)
    value = np.zeros(markers.shape, np.int64)
    for t, frame in enumerate(markers):
        if not np.any(frame):
            continue
        if indices:
            dist[t], (iy, ix) = ndi.distance_transform_edt(frame == 0, return_indices=True)
            value[t] = frame[iy, ix]
        else:
            dist[t] = ndi.distance_transform_edt(frame == 0)
    return dist, value


def restate_marker_distance(labels, time_range=1):
    d = _frames(labels)[0]
    for i in range(1, time_range + 1):
        d[i:] = np.fmin(d[:-i], d[i:])
        d[:-i] = np.fmin(d[:-i], d[i:])
    return d


def restate_cylinder(markers, time_margin, get_closest=False):
    dist, value = _frames(markers, get_closest)
    T = dist.shape[0]
    out_d, out_v = np.empty_like(dist), np.empty_like(value)
    for t in range(T):
        lo, hi = max(t - time_margin, 0), min(t + time_margin + 1, T)
        first = np.argmin(dist[lo:hi], 0)[None]                  # the earliest frame of the minimum; there is no NaN
        out_d[t] = np.take_along_axis(dist[lo:hi], first, 0)[0]
        out_v[t] = np.take_along_axis(value[lo:hi], first, 0)[0]
    return (out_d, out_v) if get_closest else out_d


def restate_label_nanmin(labels, field, index, default):
    flat, values = np.asarray(labels).ravel(), np.asarray(field).ravel()
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # np.nanmin of an all-NaN region is NaN, with a warning
        for i in index:
            region = values[flat == i]
            out.append(np.nanmin(region) if region.size else default)
    return np.asarray(out)


def restate_validate_markers(labels, glm_grid, glm_distance, edge_filter, n_glm_in_margin, coord, margin, time_margin,
                             get_closest=False):
    counts = glm_grid.astype(int).ravel()
    if get_closest:
        dist, closest = restate_cylinder(labels, time_margin, True)
        flash_closest = np.repeat(closest.ravel(), counts)
    else:
        dist, flash_closest = restate_cylinder(labels, time_margin), None
    flash_distance = np.repeat(dist.ravel(), counts)
    pod = np.sum(flash_distance <= margin) / n_glm_in_margin if n_glm_in_margin > 0 else np.nan
    flag = restate_label_nanmin(labels, edge_filter, coord, False).astype(bool)
    n_in = np.sum(flag)
    marker_distance = restate_label_nanmin(labels, glm_distance, coord, np.nan).astype(np.float64)
    far = np.sum(marker_distance[flag] > margin) / n_in if n_in > 0 else np.nan
    return flash_distance, flash_closest, marker_distance, pod, far, n_in, flag


def restate_edge_filter(flashes, times, margin, time_margin):
    """without the missing-data branch, which tobac_flow_amd.validation keeps as SciPy's binary_dilation"""
    T = flashes.shape[0]
    keep = np.zeros(flashes.shape, bool)
    keep[time_margin:T - time_margin, margin:flashes.shape[1] - margin, margin:flashes.shape[2] - margin] = True
    seconds = np.diff(np.asarray(times).astype("datetime64[ns]").astype(np.int64)) // 10 ** 9
    for i in np.flatnonzero(seconds > 900):
        keep[max(i - time_margin + 1, 0):min(i + time_margin + 2, T)] = False
    return keep


def script_inputs(labels, gap_after=None):
    """the sequence of scripts/dcc_validation.py:145-155 on the restatement: (glm_grid, glm_distance, edge_filter,
    n_glm_in_margin, dataset) for `labels`' shape"""
    grid = flash_grid(labels.shape)
    ds = SimpleNamespace(glm_flashes=grid.copy(), t=flash_times(labels.shape[0], gap_after))
    glm_distance = restate_cylinder(grid, TIME_MARGIN)
    edge = restate_edge_filter(grid, ds.t, MARGIN, TIME_MARGIN)
    grid[~edge] = 0
    return grid, glm_distance, edge, np.nansum(grid), ds


# ---- brute force -------------------------------------------------------------------------------------------------------
def brute_force(markers, time_margin=0):
    """(d2, count, label_sets, values) over the window t - time_margin .. t + time_margin of every voxel: the exact
    int64 squared in-plane distance to the nearest voxel != 0 (-1 where the window holds none), how many such voxels
    lie at exactly that distance, and a bit mask over `values` (the distinct non-zero marker values) of those they carry"""
    markers = np.asarray(markers)
    T, H, W = markers.shape
    values = [v for v in np.unique(markers[~np.isnan(markers)] if markers.dtype.kind == "f" else markers) if v != 0]
    yy, xx = np.mgrid[:H, :W]
    py, px = yy.ravel()[:, None], xx.ravel()[:, None]
    per_frame = []
    for t in range(T):
        fy, fx = np.nonzero(markers[t] != 0)
        if fy.size == 0:
            per_frame.append(None)
            continue
        d = (py - fy[None]) ** 2 + (px - fx[None]) ** 2          # (H W, features)
        bits = np.array([1 << values.index(v) if v == v else 0 for v in markers[t][fy, fx]], np.int64)
        per_frame.append((d, bits))
    d2 = np.full((T, H * W), -1, np.int64)
    count = np.zeros((T, H * W), np.int64)
    sets = np.zeros((T, H * W), np.int64)
    for t in range(T):
        window = [per_frame[k] for k in range(max(t - time_margin, 0), min(t + time_margin + 1, T)) if per_frame[k] is not None]
        if not window:
            continue
        best = np.min([d.min(1) for d, _ in window], 0)
        d2[t] = best
        for d, bits in window:
            at = d == best[:, None]
            count[t] += at.sum(1)
            sets[t] |= np.bitwise_or.reduce(np.where(at, bits[None], 0), 1)
    shape = (T, H, W)
    return d2.reshape(shape), count.reshape(shape), sets.reshape(shape), values


def single_label(sets):
    """where exactly one label lies at the minimal distance"""
    return (sets != 0) & (sets & (sets - 1) == 0)


def in_set(result, sets, values):
    """the voxels whose `result` value is one of the labels at the minimal distance (0 where there is none)"""
    bit = np.zeros(result.shape, np.int64)
    for k, v in enumerate(values):
        bit[result == v] = 1 << k
    return np.where(sets == 0, result == 0, (bit & sets) != 0)


_GOLDEN = None


def golden():
    """{case: {name: array}} of tests/golden/validation_ref.npz (written by tests/golden/make_validation_golden.py)"""
    global _GOLDEN
    if _GOLDEN is None:
        z = np.load(GOLDEN)
        _GOLDEN = {}
        for k in z.files:
            case, name = k.split("/")
            _GOLDEN.setdefault(case, {})[name] = z[k]
    return _GOLDEN
