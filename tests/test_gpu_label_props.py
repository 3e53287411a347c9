"""calculate_label_properties, get_label_stats and n_unique_along_axis (tf_label_props, tf_unique_along_t,
tf_unique_per_frame) against the restatement of the reference in tests/props_cases.py, which test_props_cases_cpu.py holds
against the reference's own primitives.

Bounds.  With float64 operands the kernel's double sums of N <= 12 000 terms are off by at most N * 2^-53 relative (areas:
non-negative terms) resp. N * 2^-53 * max|v| (a weighted mean of signed values v), far inside half a float32 spacing, so
only a rounding boundary can move the float32 cast: areas are held to ONE float32 spacing of the float64 result cast to
float32, locations to one float32 spacing at max|plane|.  Counts and everything about time are exact.  With float32
operands the comparison is with numpy's own float32 sums at the tolerance of those sums (rtol 2e-5, atol 1e-6, as
test_label_statistics_match_numpy_within_float32_summation_error)."""
import numpy as np
import pytest

import props_cases as pc

pytestmark = pytest.mark.gpu

CASES = [(3, pc.SHAPES[0]), (4, pc.SHAPES[1])]
IDS = ["x".join(map(str, c[1])) for c in CASES]


def _dataset(case, device=False):
    """a LabelDataset holding the arrays of a linked case (label volumes copied; as device tensors with device=True)"""
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords=dict(case["coords"]))
    for name, value in case.items():
        if name == "coords":
            continue
        if name.endswith("_label"):
            value = value.copy()
            if device:
                import torch
                value = torch.as_tensor(value).cuda()
            ds.add(name, value, ("t", "y", "x"))
        else:
            ds[name] = value
    return ds


def _scale(name, case):
    """max |plane| of the operand a location variable averages"""
    c = name.rsplit("_", 1)[1]
    plane = case["coords"][c] if c in ("x", "y") else case[c]
    return float(np.max(np.abs(np.asarray(plane, np.float64))))


def _compare(ds, before, case, summing=np.float64):
    want = pc.expected_properties(case, summing)
    assert set(ds) - before == set(want)
    for name, (dims, value) in want.items():
        got = np.asarray(ds[name])
        assert ds.dims[name] == dims, name
        assert got.dtype == value.dtype and got.shape == value.shape, (name, got.dtype, value.dtype)
        if value.dtype.kind in "mM":
            assert pc.same_times(got, value), name
        elif value.dtype.kind == "i":
            assert np.array_equal(got, value), name
        else:
            assert np.array_equal(np.isnan(got), np.isnan(value)), name
            ok = ~np.isnan(value)
            err = np.abs(got[ok].astype(np.float64) - value[ok].astype(np.float64))
            if summing == np.float32:
                bound = 1e-6 + 2e-5 * np.abs(value[ok].astype(np.float64))
            elif name.endswith("_area"):
                bound = np.spacing(np.abs(value[ok])).astype(np.float64)
            else:
                bound = np.full(err.shape, float(np.spacing(np.float32(_scale(name, case)))))
            print(name, "max error / bound:", float((err / bound).max()) if err.size else 0.0)
            assert np.all(err <= bound), (name, float((err / bound).max()))
    return want


@pytest.mark.parametrize("seed,shape", CASES, ids=IDS)
def test_properties_after_the_scripts_order_match_the_restatement(seed, shape):
    from tobac_flow_amd import dataset as D
    core, thick, thin = pc.raw_volumes(seed, shape)
    case = pc.linked_case(seed, shape)
    ds = D.LabelDataset(coords={c: case["coords"][c] for c in ("t", "x", "y")})
    for name, v in (("core_label", core), ("thick_anvil_label", thick), ("thin_anvil_label", thin)):
        ds.add(name, v, ("t", "y", "x"))
    for name in ("area", "lat", "lon"):
        ds.add(name, case[name], ("y", "x"))
    # the script's order: scripts/dcc_detect_goes.py:316-330
    D.add_label_coords(ds)
    D.link_cores_and_anvils(ds)
    D.add_step_labels(ds)
    D.add_label_coords(ds)
    D.link_step_labels(ds)
    for c in ("core", "anvil", "core_step", "thick_anvil_step", "thin_anvil_step"):
        assert np.array_equal(ds.coords[c], case["coords"][c]), c
    assert np.array_equal(ds["core_step_core_index"], case["core_step_core_index"])
    before = set(ds)
    D.calculate_label_properties(ds)
    want = _compare(ds, before, case)
    # the case has something to choose from: a core with two or more steps of different area, and a link
    parent, area = case["core_step_core_index"], want["core_step_area"][1]
    assert any(np.unique(area[parent == i]).size >= 2 for i in case["coords"]["core"])
    assert np.asarray(ds["core_anvil_index"]).max() > 0


@pytest.mark.parametrize("seed,shape", CASES, ids=IDS)
def test_float32_operands_match_numpys_float32_sums(seed, shape):
    from tobac_flow_amd.dataset import calculate_label_properties
    case = pc.linked_case(seed, shape, dtype=np.float32)
    assert case["area"].dtype == np.float32 and case["coords"]["x"].dtype == np.float32
    ds = _dataset(case)
    before = set(ds)
    calculate_label_properties(ds)
    _compare(ds, before, case, np.float32)


# ---- tf_label_props on hand-made volumes ---------------------------------------------------------------------------------
def _operands(shape, seed=5):
    g = pc.grid(shape, seed)
    T = shape[0]
    rank = np.random.default_rng(seed).permutation(T).astype(np.int32)
    return dict(area=g["area"], x=g["x"], y=g["y"], lat=g["lat"], lon=g["lon"], t_rank=rank)


def _expect_records(labels, n_labels, area=None, x=None, y=None, lat=None, lon=None, t_rank=None):
    """the accumulators of include/tobac_flow_hip.h, one numpy pass per id"""
    out = {k: np.zeros(n_labels + 1) for k in ("area_nansum", "w", "wx", "wy", "wlat", "wlon")}
    out["count"] = np.zeros(n_labels + 1, np.int64)
    out["tmin"] = np.full(n_labels + 1, 0x7fffffff, np.int32)
    out["tmax"] = np.full(n_labels + 1, -1, np.int32)
    for i in range(1, n_labels + 1):
        tt, yy, xx = np.nonzero(labels == i)
        out["count"][i] = tt.size
        if tt.size and t_rank is not None:
            out["tmin"][i], out["tmax"][i] = t_rank[tt].min(), t_rank[tt].max()
        if tt.size and area is not None:
            a = area[yy, xx]
            out["area_nansum"][i], out["w"][i] = np.nansum(a), a.sum()
            for key, v in (("wx", None if x is None else x[xx]), ("wy", None if y is None else y[yy]),
                           ("wlat", None if lat is None else lat[yy, xx]), ("wlon", None if lon is None else lon[yy, xx])):
                if v is not None:
                    out[key][i] = (a * v).sum()
    return out


def _check_records(labels, n_labels, **ops):
    from tobac_flow_amd.label import label_props
    got = label_props(labels, n_labels, **ops)
    want = _expect_records(np.asarray(labels), n_labels, **ops)
    assert got.shape == (n_labels + 1,)
    for key in ("count", "tmin", "tmax"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("area_nansum", "w", "wx", "wy", "wlat", "wlon"):
        n = max(int(want["count"].max()), 1)
        # double sums of n terms in another order: n * 2^-53 of the sum of the terms' magnitudes (<= n * max|term|)
        scale = {"area_nansum": 1.0, "w": 1.0, "wx": 0.11, "wy": 0.09, "wlat": 40.0, "wlon": 140.0}[key] * 10.0 * n
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
        assert np.allclose(got[key], want[key], rtol=0, atol=n * 2.0 ** -53 * scale, equal_nan=True), key
    return got


def test_label_props_one_voxel_and_one_long_run():
    one = np.ones((1, 1, 1), np.int32)
    got = _check_records(one, 1, **_operands(one.shape))
    assert got["count"][1] == 1 and got["count"][0] == 0
    run = np.full((1, 1, 300), 2, np.int32)                       # no background, every lane adds to the same record
    got = _check_records(run, 2, **_operands(run.shape))
    assert list(got["count"]) == [0, 0, 300]


def test_label_props_alternating_labels_and_all_zero():
    alt = (1 + (np.arange(3 * 2 * 130) % 2)).reshape(3, 2, 130).astype(np.int32)     # no run longer than one voxel
    got = _check_records(alt, 2, **_operands(alt.shape))
    assert list(got["count"]) == [0, 390, 390]
    zero = np.zeros((3, 2, 130), np.int32)
    got = _check_records(zero, 4, **_operands(zero.shape))
    assert not got["count"].any() and np.all(got["tmax"] == -1) and np.all(got["tmin"] == 0x7fffffff)


def test_label_props_gaps_and_ids_beyond_n_labels():
    rng = np.random.default_rng(8)
    lab = rng.choice(np.array([0, 0, 0, 3, 4, 9, 11], np.int32), (3, 5, 68)).astype(np.int32)
    lab = np.repeat(lab, 2, axis=2)[:, :, :68].copy()             # runs of two; a width that takes the wide loads
    ops = _operands(lab.shape)
    full = _check_records(lab, 20, **ops)                         # n_labels above the largest id: the gaps stay empty
    assert full["count"][[1, 2, 5, 12, 20]].sum() == 0 and full["count"][11] > 0
    cut = _check_records(lab, 9, **ops)                           # two below the largest id: its voxels are skipped
    for key in cut.dtype.names:
        assert np.array_equal(cut[key], full[key][:10], equal_nan=True) or np.allclose(cut[key], full[key][:10], rtol=1e-13, atol=0)
    negative = lab.copy()
    negative[0, 0, :5] = -3
    _check_records(negative, 11, **ops)


def test_label_props_runs_do_not_straddle_rows():
    lab = np.zeros((2, 3, 37), np.int32)
    lab[0, 0, 30:] = 5                                            # ends at the last voxel of a row ...
    lab[0, 1, :4] = 5                                             # ... and begins the next one
    lab[1, 2, 36] = 6
    ops = _operands(lab.shape)
    got = _check_records(lab, 6, **ops)
    a, y = ops["area"], ops["y"]
    assert np.isclose(got["wy"][5], a[0, 30:].sum() * y[0] + a[1, :4].sum() * y[1], rtol=1e-14, atol=0)
    assert got["tmin"][5] == got["tmax"][5] == ops["t_rank"][0] and got["tmin"][6] == ops["t_rank"][1]


def test_label_props_null_operands_switch_their_sums_off():
    core, thick, thin = pc.raw_volumes(*CASES[1])
    ops = _operands(thin.shape)
    n = int(thin.max())
    got = _check_records(thin, n)
    assert not got["w"].any() and np.all(got["tmax"] == -1) and got["count"].sum() == np.count_nonzero(thin)
    _check_records(thin, n, area=ops["area"], t_rank=ops["t_rank"])
    _check_records(thin, n, area=ops["area"], lat=ops["lat"], y=ops["y"])
    _check_records(thin, n, **ops)
    with pytest.raises(ValueError):
        _check_records(thin, n, x=ops["x"])                       # a location without the area that weights it


# ---- semantics of calculate_label_properties ------------------------------------------------------------------------------
def _run(case, device=False):
    from tobac_flow_amd.dataset import calculate_label_properties
    ds = _dataset(case, device)
    before = set(ds)
    calculate_label_properties(ds)
    return ds, before


def test_nan_area_inside_and_outside_a_region():
    case = pc.with_nan_area(pc.linked_case(*CASES[0]))
    ds, before = _run(case)
    want = _compare(ds, before, case)
    nan = np.isnan(want["core_step_lat"][1])
    assert nan.any() and not nan.all() and not np.isnan(ds["core_step_area"]).any()


def test_a_region_of_zero_area_raises_like_np_average():
    case = pc.linked_case(*CASES[0])
    area = case["area"].copy()
    area[np.any(case["core_step_label"] == case["coords"]["core_step"][-1], axis=0)] = 0.0
    with pytest.raises(ZeroDivisionError, match="Weights sum to zero"):
        _run(dict(case, area=area))
    with pytest.raises(ZeroDivisionError):
        pc.expected_properties(dict(case, area=area))


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_t_need_not_be_sorted(order):
    seed, shape = CASES[1]
    t = pc.grid(shape)["t"]
    t = t[::-1].copy() if order == "descending" else t[np.random.default_rng(2).permutation(t.size)]
    case = pc.linked_case(seed, shape, t=t)
    ds, before = _run(case)
    want = _compare(ds, before, case)
    assert (want["thin_anvil_lifetime"][1] > np.timedelta64(0, "ns")).any()


def test_one_dimensional_lat_lon_are_meshed():
    seed, shape = CASES[1]
    g = pc.grid(shape)
    case = pc.linked_case(seed, shape, lat=g["lat"][:, 0].copy(), lon=g["lon"][0, :].copy())
    ds, before = _run(case)
    _compare(ds, before, dict(case, lat=np.repeat(case["lat"][:, None], shape[2], 1), lon=np.repeat(case["lon"][None], shape[1], 0)))


def test_a_coordinate_id_absent_from_its_volume():
    case = pc.linked_case(*CASES[0])
    coords = dict(case["coords"])
    coords["thin_anvil_step"] = np.append(coords["thin_anvil_step"], coords["thin_anvil_step"][-1] + 3).astype(np.int32)
    case = dict(case, coords=coords)
    ds, before = _run(case)
    _compare(ds, before, case)
    assert ds["thin_anvil_step_pixel_count"][-1] == 0 and np.isnan(ds["thin_anvil_step_area"][-1])
    assert np.isnat(ds["thin_anvil_step_t"][-1]) and np.isnan(ds["thin_anvil_step_lon"][-1])
    # the anvil coordinate is shared: thin-only anvils are absent from the thick volume
    assert np.isnan(ds["thick_anvil_total_area"]).any() and np.isnat(ds["thick_anvil_lifetime"]).any()


def test_device_tensor_volumes_give_the_same_variables():
    case = pc.linked_case(*CASES[1])
    host, before = _run(case)
    dev, _ = _run(case, device=True)
    assert dev["core_label"].is_cuda and dev["thin_anvil_step_label"].is_cuda
    for name in set(host) - before:
        a, b = np.asarray(host[name]), np.asarray(dev[name])
        assert a.dtype == b.dtype and host.dims[name] == dev.dims[name]
        if a.dtype.kind == "f":                                   # double atomics: the last bits of a sum may differ
            assert np.allclose(a, b, rtol=2.0 ** -22, atol=0, equal_nan=True), name
        else:
            assert pc.same_times(a, b) if a.dtype.kind in "mM" else np.array_equal(a, b), name


# ---- unique counts ------------------------------------------------------------------------------------------------------
def _lanes_for(T):
    return 256 if T <= 160 else 128 if T <= 320 else 64 if T <= 640 else 0


def test_unique_along_t_on_hand_made_columns_in_both_forms():
    """(T, 3, 70) volumes (at most 147 k voxels) at T = 1, 2, 40, on both sides of every T at which the workgroup of the
    LDS form shrinks (160, 320), on both sides of the switch to the HBM scratch (640), and at 700"""
    from tobac_flow_amd.label import unique_along_t
    forms_seen = set()
    for T in (1, 2, 40, 160, 161, 320, 321, 640, 641, 700):
        v = pc.column_volume(T)
        uniq, nz, lanes = unique_along_t(v)
        assert uniq.dtype == np.int32 and nz.dtype == np.int32 and uniq.shape == (3, 70), T
        assert np.array_equal(uniq, pc.distinct_nonzero(v, 0)) and np.array_equal(nz, np.count_nonzero(v, 0)), T
        assert uniq[0, 3] == T and uniq[0, 4] == 0, T
        assert lanes == _lanes_for(T), T                          # 0: the sets lived in the HBM scratch
        forms_seen.add(lanes)
    assert forms_seen == {0, 64, 128, 256}                        # both forms, and every workgroup size of the LDS one


@pytest.mark.parametrize("seed,shape", CASES, ids=IDS)
def test_unique_counts_on_label_volumes(seed, shape):
    import torch
    from tobac_flow_amd.label import unique_along_t, unique_per_frame
    for v in pc.raw_volumes(seed, shape):
        uniq, nz, lanes = unique_along_t(v)
        assert lanes == 256
        assert np.array_equal(uniq, pc.distinct_nonzero(v, 0)) and np.array_equal(nz, np.count_nonzero(v, 0))
        per, count = unique_per_frame(torch.as_tensor(v).cuda())
        assert per.dtype == np.int32 and count.dtype == np.int64
        assert np.array_equal(per, pc.distinct_nonzero(v.reshape(shape[0], -1), 1))
        assert np.array_equal(count, np.count_nonzero(v, (1, 2)))


@pytest.mark.parametrize("T", [1, 2, 40, 700])
def test_unique_per_frame_on_hand_made_volumes(T):
    from tobac_flow_amd.label import unique_per_frame
    v = pc.column_volume(T, negatives=False)
    if T > 2:
        v[1] = 0                                                  # an empty frame between two occupied ones
    per, count = unique_per_frame(v)
    assert np.array_equal(per, pc.distinct_nonzero(v.reshape(T, -1), 1)) and np.array_equal(count, np.count_nonzero(v, (1, 2)))
    assert T <= 2 or (per[1] == 0 and per[0] > 0 and per[2] > 0)
    # ids above n_labels are not counted as labels, but are non-zero voxels
    per_cut, count_cut = unique_per_frame(v, 8)
    assert np.array_equal(per_cut, pc.distinct_nonzero(np.where(v > 8, 0, v).reshape(T, -1), 1)) and np.array_equal(count_cut, count)


def test_n_unique_along_axis_on_every_axis():
    import torch
    from tobac_flow_amd.utils import n_unique_along_axis
    v = pc.column_volume(40)                                      # holds negative ids
    labels = pc.raw_volumes(*CASES[1])[2]
    for a in (v, labels, labels.astype(np.int64), np.abs(v).astype(np.uint8)):
        for axis in (0, 1, 2, -1):
            got = n_unique_along_axis(a, axis)
            assert got.dtype == np.int32 and np.array_equal(got, pc.distinct_nonzero(a, axis)), axis
            assert np.array_equal(n_unique_along_axis(torch.as_tensor(a).cuda(), axis), got)
        flat = a.reshape(a.shape[0], -1)
        for axis in (0, 1):
            assert np.array_equal(n_unique_along_axis(flat, axis), pc.distinct_nonzero(flat, axis)), axis
    # what the kernels do not take goes through the formula itself
    f = np.where(v == 0, 0.0, v + 0.5)
    assert np.array_equal(n_unique_along_axis(f, 0), pc.distinct_nonzero(f, 0)) and n_unique_along_axis(f, 0).dtype == np.int32
    big = labels.astype(np.int64) * (1 << 33)
    assert np.array_equal(n_unique_along_axis(big, 2), pc.distinct_nonzero(big, 2))
    assert np.array_equal(n_unique_along_axis(labels[0, 0], 0), pc.distinct_nonzero(labels[0, 0], 0))


def test_get_label_stats_variables():
    from tobac_flow_amd.analysis import get_label_stats
    seed, shape = CASES[0]
    case = pc.linked_case(seed, shape)
    T, Y, X = shape
    for device in (False, True):
        ds = _dataset(case, device)
        before = set(ds)
        get_label_stats("thick_anvil_label", ds)
        get_label_stats(ds["core_step_label"], ds, name="core_step")
        assert set(ds) - before == {p + s for p in ("thick_anvil_label", "core_step")
                                    for s in ("_fraction", "_unique_count", "_temporal_fraction", "_temporal_unique_count")}
        for prefix, v in (("thick_anvil_label", case["thick_anvil_label"]), ("core_step", case["core_step_label"])):
            want = {"_fraction": (("y", "x"), (np.count_nonzero(v, 0) / T).astype(np.float32)),
                    "_unique_count": (("y", "x"), pc.distinct_nonzero(v, 0).astype(np.int32)),
                    "_temporal_fraction": (("t",), (np.count_nonzero(v, (1, 2)) / (X * Y)).astype(np.float32)),
                    "_temporal_unique_count": (("t",), pc.distinct_nonzero(v.reshape([T, -1]), 1).astype(np.int32))}
            for suffix, (dims, value) in want.items():
                got = ds[prefix + suffix]
                assert isinstance(got, np.ndarray) and ds.dims[prefix + suffix] == dims
                assert got.dtype == value.dtype and np.array_equal(got, value), prefix + suffix
    with pytest.raises(ValueError):
        get_label_stats(case["core_label"], _dataset(case))       # an array needs name=
