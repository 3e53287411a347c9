"""The yardstick of the label-property tests (tests/props_cases.py) against the reference's own primitives, the pure host
reductions of calculate_label_properties, and its input validation.  No GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import props_cases as pc

CASES = [(3, pc.SHAPES[0]), (4, pc.SHAPES[1])]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "x".join(map(str, c[1])))
def case(request):
    seed, shape = request.param
    return pc.linked_case(seed, shape)


def _check_against_primitives(case):
    """dataset.py:705-1595 with its calls made directly: np.bincount, labeled_comprehension(np.nansum / np.nanmin /
    np.nanmax) on broadcast operands, np.average(..., weights=) on np.repeat stacks"""
    want = pc.expected_properties(case)
    T = case["coords"]["t"].size
    t3 = case["coords"]["t"][:, None, None]
    area_stack = np.repeat(case["area"][None], T, 0)
    xx, yy = np.meshgrid(case["coords"]["x"], case["coords"]["y"])
    stacks = {"x": np.repeat(xx[None], T, 0), "y": np.repeat(yy[None], T, 0),
              "lat": np.repeat(case["lat"][None], T, 0), "lon": np.repeat(case["lon"][None], T, 0)}
    for kind, dim in pc.KINDS:
        for vol, ids, prefix, d in ((case[kind + "_label"], case["coords"][dim], kind, dim),
                                    (case[kind + "_step_label"], case["coords"][kind + "_step"], kind + "_step", kind + "_step")):
            step = prefix.endswith("_step")
            if step or kind == "core":
                got = want[prefix + "_pixel_count"]
                assert got[0] == (d,) and got[1].dtype == np.int32
                assert np.array_equal(got[1], np.bincount(vol.ravel())[ids])
            if step or kind != "thin_anvil":
                name = prefix + ("_area" if step else "_total_area")
                ref = ndi.labeled_comprehension(case["area"][None], vol, ids, np.nansum, np.float32, np.nan)
                assert want[name][1].dtype == np.float32
                # float64 pairwise sums in two orders, cast to float32: equal up to a rounding boundary
                assert np.allclose(want[name][1], ref, rtol=2.0 ** -23, atol=0, equal_nan=True), name
            tmin = ndi.labeled_comprehension(t3, vol, ids, np.nanmin, "datetime64[ns]", None)
            tmax = ndi.labeled_comprehension(t3, vol, ids, np.nanmax, "datetime64[ns]", None)
            if step:
                assert pc.same_times(want[prefix + "_t"][1], tmin)
            else:
                assert pc.same_times(want[prefix + "_start_t"][1], tmin) and pc.same_times(want[prefix + "_end_t"][1], tmax)
                assert pc.same_times(want[prefix + "_lifetime"][1], (tmax - tmin).astype("timedelta64[ns]"))
            if step:
                for c, stack in stacks.items():
                    ref = np.array([np.average(stack[vol == i], weights=area_stack[vol == i]) for i in ids])
                    got = want[f"{prefix}_{c}"][1]
                    assert got.dtype == np.float32
                    assert np.allclose(got, ref.astype(np.float32), rtol=2.0 ** -23, atol=0, equal_nan=True), (prefix, c)
    # the per-core choices, as the reference writes them
    core, core_step, parent = case["coords"]["core"], case["coords"]["core_step"], case["core_step_core_index"]
    step_area = want["core_step_area"][1]
    widest = np.asarray([core_step[parent == i][np.argmax(step_area[parent == i])] for i in core])
    first = np.asarray([np.nanmin(core_step[parent == i]) for i in core])
    loc = lambda ids: np.searchsorted(core_step, ids)             # noqa: E731  (`.loc[...]` on the ascending coordinate)
    assert np.array_equal(want["core_max_area"][1], step_area[loc(widest)], equal_nan=True)
    assert pc.same_times(want["core_max_area_t"][1], want["core_step_t"][1][loc(widest)])
    for c in ("x", "y", "lat", "lon"):
        assert np.array_equal(want[f"core_start_{c}"][1], want[f"core_step_{c}"][1][loc(first)], equal_nan=True)
    return want


def test_restatement_equals_the_references_primitives(case):
    want = _check_against_primitives(case)
    assert len(want) == 39                                      # 11 core, 4 thick, 3 thin, 3 x 7 step variables
    # the case has something to choose from: a core with steps of different area, and a core linked to an anvil
    parent, area = case["core_step_core_index"], want["core_step_area"][1]
    assert any(np.unique(area[parent == i]).size >= 2 for i in case["coords"]["core"])
    assert case["core_anvil_index"].max() > 0


def test_restatement_with_nan_areas_equals_the_primitives(case):
    want = _check_against_primitives(pc.with_nan_area(case))
    nan = np.isnan(want["core_step_x"][1])                        # the steps that cover the pixel, in every frame they do
    assert nan.any() and not nan.all() and not np.isnan(want["core_step_area"][1]).any()


@pytest.mark.parametrize("T", [1, 2, 5, 40])
def test_sorted_form_counts_distinct_nonzero_values(T):
    """the package's host form (sort, then count the non-zero entries that differ from their predecessor) against a Python
    set per line, negative ids included"""
    from tobac_flow_amd.utils.stats_utils import _sorted_form
    v = pc.column_volume(T)
    for axis in (0, 1, 2):
        got = _sorted_form(v, axis)
        assert got.dtype == np.int32 and np.array_equal(got, pc.distinct_nonzero(v, axis)), axis
    assert np.array_equal(_sorted_form(v.reshape(T, -1), 1), pc.distinct_nonzero(v.reshape(T, -1), 1))
    # the hand-made columns: a,0,a / a,b,a / a,a,b,b,5 (no zero) / all distinct / all zero / -2,0,-2,-5
    by_hand = {1: [1, 1, 1, 1, 0, 1], 2: [1, 2, 1, 2, 0, 1], 5: [1, 2, 3, 5, 0, 2], 40: [1, 2, 3, 40, 0, 2]}
    assert list(pc.distinct_nonzero(v, 0)[0, :6]) == by_hand[T]
    assert list(_sorted_form(v, 0)[0, :6]) == by_hand[T]


def test_sorted_form_on_the_label_volumes_and_floats(case):
    from tobac_flow_amd.utils.stats_utils import _sorted_form
    for name in ("core_label", "thin_anvil_label", "core_step_label"):
        for axis in (0, 1, 2):
            assert np.array_equal(_sorted_form(case[name], axis), pc.distinct_nonzero(case[name], axis))
    f = np.where(case["core_label"] == 0, 0.0, case["core_label"] + 0.5)
    assert np.array_equal(_sorted_form(f, 0), pc.distinct_nonzero(f, 0))


# ---- the host reductions ------------------------------------------------------------------------------------------------
def test_first_max_step_ties_nan_and_order():
    from tobac_flow_amd.dataset import _first_max_step, _first_step
    ids = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.int32)
    parent = np.array([1, 1, 1, 2, 2, 3, 3, 0], np.int32)
    area = np.array([2.0, 5.0, 5.0, np.nan, 9.0, 1.0, np.nan, 50.0], np.float32)
    parents = np.array([1, 2, 3], np.int32)
    # core 1: a tie between steps 2 and 3 -> step 2; core 2: the NaN wins although 9 is larger; core 3: the NaN comes last
    assert list(ids[_first_max_step(ids, parent, area, parents)]) == [2, 4, 7]
    assert list(ids[_first_step(ids, parent, parents)]) == [1, 4, 6]
    assert np.array_equal(_first_max_step(ids, parent, area, parents), pc.first_max_step(ids, parent, area, parents))
    # two NaNs: the first one
    assert list(ids[_first_max_step(ids, np.ones(8, np.int32), np.where(ids % 3 == 0, np.nan, 1.0), [1])]) == [3]
    # the steps listed out of order: the choice goes by step id, the result is a position in the arrays as listed
    rng = np.random.default_rng(0)
    for _ in range(5):
        p = rng.permutation(ids.size)
        got = _first_max_step(ids[p], parent[p], area[p], parents)
        assert list(ids[p][got]) == [2, 4, 7]
        assert np.array_equal(got, pc.first_max_step(ids[p], parent[p], area[p], parents))
        assert list(ids[p][_first_step(ids[p], parent[p], parents)]) == [1, 4, 6]
        assert np.array_equal(_first_step(ids[p], parent[p], parents), pc.first_step(ids[p], parent[p], parents))
    # parents asked for in another order, and only some of them
    assert list(ids[_first_max_step(ids, parent, area, [3, 1])]) == [7, 2]


def test_a_core_without_steps_raises():
    from tobac_flow_amd.dataset import _first_max_step, _first_step
    ids, parent, area = np.array([1, 2]), np.array([1, 1]), np.array([1.0, 2.0])
    for parents in ([1, 2], [0], [5]):
        with pytest.raises(ValueError):
            _first_max_step(ids, parent, area, parents)
        with pytest.raises(ValueError):
            _first_step(ids, parent, parents)
        with pytest.raises(ValueError):
            pc.first_max_step(ids, parent, area, parents)
        with pytest.raises(ValueError):
            pc.first_step(ids, parent, parents)
    with pytest.raises(ValueError):
        _first_max_step(np.zeros(0, int), np.zeros(0, int), np.zeros(0), [1])
    assert _first_max_step(np.zeros(0, int), np.zeros(0, int), np.zeros(0), []).size == 0


def test_host_reductions_agree_with_the_restatement_on_the_cases(case):
    from tobac_flow_amd.dataset import _first_max_step, _first_step
    want = pc.expected_properties(case)
    core, core_step, parent = case["coords"]["core"], case["coords"]["core_step"], case["core_step_core_index"]
    area = want["core_step_area"][1]
    assert np.array_equal(_first_max_step(core_step, parent, area, core), pc.first_max_step(core_step, parent, area, core))
    assert np.array_equal(_first_step(core_step, parent, core), pc.first_step(core_step, parent, core))


# ---- input validation: everything below raises before the library or a device is touched --------------------------------
def _dataset(case):
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords=case["coords"])
    for name, value in case.items():
        if name != "coords":
            ds[name] = value
    return ds


def test_missing_inputs_raise_keyerror_naming_them(case):
    from tobac_flow_amd.dataset import calculate_label_properties
    for name in ("area", "lat", "lon", "core_label", "thin_anvil_step_label", "core_step_core_index"):
        ds = _dataset(case)
        del ds[name]
        with pytest.raises(KeyError, match=name):
            calculate_label_properties(ds)
    for name in ("x", "y", "t", "core", "anvil", "thick_anvil_step"):
        ds = _dataset(case)
        ds.coords = {k: v for k, v in ds.coords.items() if k != name}
        with pytest.raises(KeyError, match=f"'{name}'"):
            calculate_label_properties(ds)


def test_mismatched_lat_lon_and_nat_raise_valueerror(case):
    from tobac_flow_amd.dataset import calculate_label_properties
    ds = _dataset(case)
    ds["lat"] = case["lat"][:, 0]                                 # lat 1-D with lon 2-D
    with pytest.raises(ValueError, match="lat and lon"):
        calculate_label_properties(ds)
    ds = _dataset(case)
    ds["area"] = case["area"][:, :-1]
    with pytest.raises(ValueError, match="area"):
        calculate_label_properties(ds)
    ds = _dataset(case)
    t = case["coords"]["t"].copy()
    t[1] = np.datetime64("NaT")
    ds.coords = dict(ds.coords, t=t)
    with pytest.raises(ValueError, match="NaT"):
        calculate_label_properties(ds)
