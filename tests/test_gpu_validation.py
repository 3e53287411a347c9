"""GLM validation on the GPU (tobac_flow_amd.validation, ndimage_dev.distance_transform_edt_frames, and the C ABI of
tf_edt2d_frames / tf_edt_cylinder / tf_label_nanmin) against the reference's own results (tests/golden/validation_ref.npz),
SciPy and brute force (tests/validation_cases.py).

Everything computed is an integer squared distance followed by one correctly rounded square root, so the bound is
equality: (a) distances are bit-equal everywhere; (b) a returned feature or label is one of those at exactly the minimal
distance, found by brute force; (c) it equals the reference wherever only one label (SciPy: one feature) lies there;
(d) two runs give identical output.  No share of pixels is exempted."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import validation_cases as vc

pytestmark = pytest.mark.gpu
M, TM = vc.MARGIN, vc.TIME_MARGIN


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


_BRUTE = {}


def brute(name, markers, tm):
    if (name, tm) not in _BRUTE:
        _BRUTE[name, tm] = vc.brute_force(markers, tm)
    return _BRUTE[name, tm]


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def host(x):
    return x.cpu().numpy()


# ---- distance_transform_edt_frames against SciPy and brute force ---------------------------------------------------------
VOLUMES = {"boxes": vc.boxes, "borders": vc.borders, "single": vc.single, "one_row": lambda: vc.degenerate()[0],
           "one_column": lambda: vc.degenerate()[1], "wide": vc.wide, "lds_limit": lambda: vc.very_wide()[:, :, :16384],
           "very_wide": vc.very_wide}


@pytest.mark.parametrize("name", list(VOLUMES))
def test_edt_frames_equal_scipy_and_indices_point_at_a_nearest_zero(lib, name):
    from tobac_flow_amd import ndimage_dev
    markers = VOLUMES[name]()
    x = markers == 0                                              # SciPy measures the distance to the nearest ZERO of its input
    T, H, W = x.shape
    xd = lib.to_dev(x)
    dist_t, idx_t = ndimage_dev.distance_transform_edt_frames(xd, return_indices=True)
    dist, idx = host(dist_t), host(idx_t)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and idx.shape == (2, T, H, W)
    yy, xx = np.mgrid[:H, :W]
    for t in range(T):
        if x[t].all():                                            # no zero voxel: inf and -1 by contract
            assert np.isposinf(dist[t]).all() and (idx[:, t] == -1).all()
            continue
        want, (wy, wx) = ndi.distance_transform_edt(x[t], return_indices=True)
        assert np.array_equal(dist[t], want)                                                         # (a) bit for bit
        iy, ix = idx[0, t], idx[1, t]
        assert (iy >= 0).all() and (iy < H).all() and (ix >= 0).all() and (ix < W).all()
        assert not x[t][iy, ix].any()                                                                # (b) a zero voxel ...
        assert np.array_equal(np.sqrt(((iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2).astype(np.float64)), want)   # ... at the distance
        if name not in ("wide", "lds_limit", "very_wide"):                                                        # (c) SciPy's wherever it is unique
            d2, count, _, _ = brute(name, markers, 0)
            assert np.array_equal(np.sqrt(d2[t].astype(np.float64)), want)
            one = count[t] == 1
            assert np.array_equal(iy[one], wy[one]) and np.array_equal(ix[one], wx[one])
            if name in ("boxes", "borders"):
                assert (~one).any()
    again = ndimage_dev.distance_transform_edt_frames(xd, return_indices=True)                       # (d)
    assert np.array_equal(host(again[0]), dist) and np.array_equal(host(again[1]), idx)
    same(host(ndimage_dev.distance_transform_edt_frames(xd)), dist)
    same(host(ndimage_dev.distance_transform_edt_frames(xd, return_distances=False, return_indices=True)), idx)
    if name == "single":
        assert dist[0, 0, 0] == np.sqrt(69.0 ** 2 + 36.0 ** 2) and (dist[1] == 0).all()


def test_the_square_root_is_numpys_for_every_integer_it_can_meet(lib):
    """tf_edt_cylinder on squared distances given directly: 0 .. 2^17, the largest admissible ones and random ones"""
    from tobac_flow_amd import ndimage_dev
    t = lib.torch()
    rng = np.random.default_rng(2)
    d2 = np.concatenate([np.arange(1 << 17), 2 ** 31 - 2 - np.arange(1 << 12), rng.integers(0, 2 ** 31 - 1, 1 << 17),
                         np.arange(1, 46341) ** 2, np.arange(1, 46341) ** 2 - 1, np.arange(1, 46341) ** 2 + 1]).astype(np.int32)
    d2[7] = 2 ** 31 - 1                                           # the "no feature" value
    dist, src = ndimage_dev.edt_cylinder(lib.to_dev(d2.reshape(1, 1, -1)), None, 0)
    want = np.sqrt(d2.astype(np.float64))
    want[7] = np.inf
    assert src is None
    same(host(dist).ravel(), want)


# ---- the five functions against the reference's results ---------------------------------------------------------------
def check_closest(name, labels, tm, closest, reference):
    _, _, sets, values = brute(name, labels, tm)
    closest = np.asarray(closest)
    assert closest.dtype == np.int64
    assert vc.in_set(closest, sets, values).all()                                                    # (b)
    one = vc.single_label(sets) | (sets == 0)
    assert np.array_equal(closest[one], reference[one])                                              # (c)
    return int((closest != reference).sum())


@pytest.mark.parametrize("device_inputs", [False, True])
def test_marker_distances_equal_the_reference(lib, device_inputs):
    from tobac_flow_amd import validation as v
    g = vc.golden()
    give = (lambda a: lib.to_dev(a)) if device_inputs else (lambda a: a)
    take = host if device_inputs else (lambda a: a)
    differing = 0
    for name, cases in (("boxes", (0, 2, 7)), ("borders", (1,))):
        c = g[name]
        labels = give(c["labels"])
        for time_range in (1, 2):
            if f"marker_distance_{time_range}" in c:
                same(take(v.get_marker_distance(labels, time_range)), c[f"marker_distance_{time_range}"])    # (a)
        for tm in cases:
            want = c[f"cylinder_{tm}_closest_distance"]
            got = v.get_marker_distance_cylinder(labels, tm)
            assert lib.is_tensor(got) == device_inputs
            same(take(got), want)                                                                    # (a)
            dist, closest = v.get_marker_distance_cylinder(labels, tm, get_closest=True)
            same(take(dist), want)
            differing += check_closest(name, c["labels"], tm, take(closest), c[f"cylinder_{tm}_closest"])
            dist2, closest2 = v.get_marker_distance_cylinder(labels, tm, get_closest=True)           # (d)
            assert np.array_equal(take(closest2), take(closest)) and np.array_equal(take(dist2), take(dist))
    print("closest markers that differ from the reference's choice (all at tie pixels):", differing)


@pytest.mark.parametrize("dtype", [np.bool_, np.uint8, np.int64, np.int16, np.float32, np.float64])
def test_every_marker_dtype_gives_the_same_distances(lib, dtype):
    from tobac_flow_amd import validation as v
    c = vc.golden()["boxes"]
    markers = c["labels"].astype(dtype)
    same(v.get_marker_distance_cylinder(markers, 2), c["cylinder_2"])
    if dtype != np.bool_:
        closest = v.get_marker_distance_cylinder(markers, 2, get_closest=True)[1]
        check_closest("boxes", c["labels"], 2, closest, c["cylinder_2_closest"])


def test_flash_grid_distance_counts_nan_as_a_flash(lib):
    from tobac_flow_amd import validation as v
    c = vc.golden()["boxes"]
    same(v.get_marker_distance_cylinder(c["glm_grid_raw"], TM), c["glm_distance"])
    at = np.argwhere(np.isnan(c["glm_grid_raw"]))[0]
    assert c["glm_distance"][tuple(at)] == 0


@pytest.mark.parametrize("device_inputs", [False, True])
@pytest.mark.parametrize("get_closest", [False, True])
def test_validate_markers_equals_the_reference(lib, device_inputs, get_closest):
    from tobac_flow_amd import validation as v
    c = vc.golden()["boxes"]
    give = (lambda a: lib.to_dev(a)) if device_inputs else (lambda a: a)
    take = host if device_inputs else (lambda a: a)
    run = lambda: v.validate_markers(give(c["labels"]), give(c["glm_grid"]), give(c["glm_distance"]), give(c["edge_filter"]),   # noqa: E731
                                     c["n_glm_in_margin"], coord=c["index"], margin=M, time_margin=TM, get_closest=get_closest)
    got = run()
    key = f"validate_{int(get_closest)}_"
    same(take(got[0]), c[key + "flash_distance"])
    same(take(got[2]), c[key + "marker_distance"])
    same(take(got[6]), c[key + "margin_flag"])
    assert got[3] == c[key + "pod"] and got[4] == c[key + "far"] and got[5] == c[key + "n_marker_in_margin"]
    assert 0 < got[3] < 1 and 0 < got[4] < 1
    if not get_closest:
        assert got[1] is None
    else:
        _, _, sets, values = brute("boxes", c["labels"], TM)
        counts = c["glm_grid"].astype(int).ravel()
        flash_sets = np.repeat(sets.ravel(), counts)
        closest, reference = take(got[1]), c[key + "flash_closest"]
        assert closest.dtype == np.int64 and closest.shape == reference.shape
        assert vc.in_set(closest, flash_sets, values).all()                                          # (b)
        one = vc.single_label(flash_sets) | (flash_sets == 0)
        assert np.array_equal(closest[one], reference[one])                                          # (c)
    plain = lambda r: [None if a is None else np.asarray(host(a) if lib.is_tensor(a) else a) for a in r]    # noqa: E731
    for a, b in zip(plain(got), plain(run())):                                                       # (d)
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_default_coord_is_every_label_and_a_nan_count_is_refused(lib):
    from tobac_flow_amd import validation as v
    c = vc.golden()["boxes"]
    labels = c["labels"]
    ids = np.arange(1, labels.max() + 1)
    got = v.validate_markers(labels, c["glm_grid"], c["glm_distance"], c["edge_filter"], c["n_glm_in_margin"], margin=M, time_margin=TM)
    want = vc.restate_validate_markers(labels, c["glm_grid"], c["glm_distance"], c["edge_filter"], c["n_glm_in_margin"], ids, M, TM)
    for a, b in zip(got, want):
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    with pytest.raises(ValueError, match="negative"):
        v.validate_markers(lib.to_dev(labels), lib.to_dev(c["glm_grid_raw"]), lib.to_dev(c["glm_distance"]),
                           lib.to_dev(c["edge_filter"]), 1.0)


@pytest.mark.parametrize("device_inputs", [False, True])
def test_min_dist_for_objects_with_an_absent_an_all_nan_and_an_inf_label(lib, device_inputs):
    from tobac_flow_amd import validation as v
    c = vc.golden()["boxes"]
    give = (lambda a: lib.to_dev(a)) if device_inputs else (lambda a: a)
    take = host if device_inputs else (lambda a: a)
    same(take(v.get_min_dist_for_objects(give(c["special_field"]), give(c["labels"]), index=c["index"])), c["special_min"])
    same(take(v.get_min_dist_for_objects(give(c["special_field"].astype(np.float32)), give(c["labels"]), index=c["index"])),
         c["special_min"].astype(np.float32).astype(np.float64))
    ids = np.arange(1, c["labels"].max() + 1)
    same(take(v.get_min_dist_for_objects(give(c["glm_distance"]), give(c["labels"]))),
         vc.restate_label_nanmin(c["labels"], c["glm_distance"], ids, np.nan).astype(np.float64))


@pytest.mark.parametrize("name,tm", [("single", 0), ("single", 1), ("single", 5), ("one_row", 1), ("one_column", 1)])
def test_cylinder_on_the_single_feature_all_feature_and_degenerate_volumes(lib, name, tm):
    from tobac_flow_amd import validation as v
    markers = VOLUMES[name]()
    same(v.get_marker_distance_cylinder(markers, tm), vc.restate_cylinder(markers, tm))               # (a)
    same(host(v.get_marker_distance(lib.to_dev(markers), 1)), vc.restate_marker_distance(markers, 1))
    if name == "single":                                          # the degenerate volumes hold NaN markers: no label to report
        dist, closest = v.get_marker_distance_cylinder(markers, tm, get_closest=True)
        want_dist, want_closest = vc.restate_cylinder(markers, tm, get_closest=True)
        same(dist, want_dist)
        check_closest(name, markers, tm, closest, want_closest)                                       # (b), (c)
        assert np.array_equal(v.get_marker_distance_cylinder(markers, tm, get_closest=True)[1], closest)   # (d)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
def test_label_minimum_over_regions_that_span_whole_waves(lib, dtype):
    """regions of thousands of consecutive voxels: the lanes of a wave agree on the label and combine their runs"""
    from tobac_flow_amd import ndimage_dev, validation as v
    labels, field, index = vc.regions()
    if dtype == np.uint8:
        field = (np.nan_to_num(field, nan=1.0, posinf=1.0) > 0).astype(np.uint8)
    field = field.astype(dtype)
    want = vc.restate_label_nanmin(labels, field, index, np.nan).astype(np.float64)
    same(v.get_min_dist_for_objects(field, labels, index=index), want)
    mins, counts = ndimage_dev.label_nanmin(lib.to_dev(labels), lib.to_dev(field), index)
    flat_labels, flat_field = labels.ravel(), field.ravel()
    want_counts = [int(np.sum(~np.isnan(flat_field[flat_labels == i].astype(np.float64)))) if (flat_labels == i).any() else -1 for i in index]
    assert host(counts).tolist() == want_counts and max(want_counts) > 4096 and -1 in want_counts
    same(host(mins), want)
    again = ndimage_dev.label_nanmin(lib.to_dev(labels), lib.to_dev(field), index)                   # (d)
    assert np.array_equal(host(again[0]), host(mins), equal_nan=True) and np.array_equal(host(again[1]), host(counts))
    if dtype != np.uint8:
        row = {int(i): k for k, i in enumerate(index)}
        assert np.isnan(want[row[4]]) and want_counts[row[4]] == 0 and np.isposinf(want[row[6]]) and np.isnan(want[row[11]])


# ---- the C ABI directly ----------------------------------------------------------------------------------------------
def test_c_abi_takes_a_misaligned_view_and_a_null_nearest(lib):
    t, L = lib.torch(), lib.lib()
    markers = vc.boxes()
    T, H, W = markers.shape
    d2_want = brute("boxes", markers, 0)[0]
    d2_want = np.where(d2_want < 0, 2 ** 31 - 1, d2_want).astype(np.int32)
    flat = t.zeros(markers.size + 1, dtype=t.int32, device=lib.device())
    view = flat[1:]                                               # one element past the allocation's alignment
    view.copy_(lib.to_dev(markers).reshape(-1))
    assert view.data_ptr() % 16 == 4
    ws = lib.workspace(L.tf_edt2d_frames_workspace_bytes(T, H, W), "edt")
    d2 = t.full((T, H, W), -7, dtype=t.int32, device=flat.device)
    lib.check(L.tf_edt2d_frames(lib.ptr(view), lib.TF_I32, T, H, W, lib.ptr(d2), None, lib.ptr(ws), ws.numel(), lib.stream_ptr()),
              "tf_edt2d_frames")
    same(host(d2), d2_want)
    nearest = t.empty_like(d2)
    lib.check(L.tf_edt2d_frames(lib.ptr(view), lib.TF_I32, T, H, W, lib.ptr(d2), lib.ptr(nearest), lib.ptr(ws), ws.numel(), lib.stream_ptr()),
              "tf_edt2d_frames")
    same(host(d2), d2_want)
    near = host(nearest)
    assert (near[[2, 5]] == -1).all() and (near[[0, 1, 3, 4]] >= 0).all()
    # the per-label minimum on misaligned views of labels and field, float32 / float64 / uint8
    c = vc.golden()["boxes"]
    ids = lib.to_dev(c["index"])
    n = markers.size
    n_labels = int(c["index"].max())
    lws = lib.workspace(L.tf_label_nanmin_workspace_bytes(n_labels), "label_nanmin")
    for field, code in ((c["special_field"].astype(np.float32), lib.TF_F32), (c["special_field"], lib.TF_F64),
                        (c["edge_filter"].view(np.uint8), lib.TF_U8)):
        shifted = t.zeros(n + 1, dtype=lib.to_dev(field).dtype, device=flat.device)
        shifted[1:].copy_(lib.to_dev(field).reshape(-1))
        mins = t.empty(ids.numel(), dtype=t.float64, device=flat.device)
        counts = t.empty(ids.numel(), dtype=t.int64, device=flat.device)
        lib.check(L.tf_label_nanmin(lib.ptr(view), lib.ptr(shifted[1:]), code, n, n_labels, lib.ptr(ids), ids.numel(), lib.ptr(mins),
                                    lib.ptr(counts), lib.ptr(lws), lws.numel(), lib.stream_ptr()), "tf_label_nanmin")
        want = vc.restate_label_nanmin(markers, field, c["index"], np.nan).astype(np.float64)
        same(host(mins), want)
        flat_labels, flat_field = markers.ravel(), field.ravel()
        want_counts = [int(np.sum(flat_field[flat_labels == i] == flat_field[flat_labels == i])) if (flat_labels == i).any() else -1 for i in c["index"]]
        assert host(counts).tolist() == want_counts and -1 in want_counts
        assert code == lib.TF_U8 or 0 in want_counts             # the all-NaN label has voxels and none that counts


def test_c_abi_reports_what_it_requires(lib):
    t, L = lib.torch(), lib.lib()
    x = t.zeros(8, dtype=t.int32, device=lib.device())
    ws = lib.workspace(1024, "edt")
    args = (lib.ptr(x), None, lib.ptr(ws), ws.numel(), lib.stream_ptr())
    assert L.tf_edt2d_frames(lib.ptr(x), lib.TF_I32, 1, 32769, 32769, *args) == -1                  # (H - 1)^2 + (W - 1)^2 = 2^31
    assert b"2^31" in L.tf_last_error()
    assert L.tf_edt2d_frames(lib.ptr(x), 9, 1, 2, 4, *args) == -1 and b"uint8" in L.tf_last_error()
    assert L.tf_edt2d_frames(lib.ptr(x), lib.TF_I32, 1, 2, 4, lib.ptr(x), None, lib.ptr(ws), 8, lib.stream_ptr()) == -2
    d = t.zeros(8, dtype=t.float64, device=x.device)
    s = t.zeros(8, dtype=t.int64, device=x.device)
    assert L.tf_edt_cylinder(lib.ptr(x), None, 1, 8, 0, lib.ptr(d), lib.ptr(s), lib.stream_ptr()) == -1     # src needs nearest
    assert L.tf_edt_cylinder(lib.ptr(x), None, 1, 8, -1, lib.ptr(d), None, lib.stream_ptr()) == -1
    assert L.tf_label_nanmin(lib.ptr(x), lib.ptr(x), lib.TF_I32, 8, 1, lib.ptr(s), 1, lib.ptr(d), lib.ptr(s), lib.ptr(ws), ws.numel(),
                             lib.stream_ptr()) == -1
    with pytest.raises(ValueError, match="2\\^31"):
        from tobac_flow_amd import ndimage_dev
        ndimage_dev.edt_squared_frames(t.zeros((1, 46342, 1), dtype=t.uint8, device=x.device))
