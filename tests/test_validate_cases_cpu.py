"""The yardsticks of the validation stage without a device: the NumPy restatement of tests/validate_cases.py against the
reference's own five wrappers in tests/golden/validate_ref.npz, name for name and dtype for dtype; the footprint rule of
tf_edge_filter's missing-data dilation against scipy.ndimage.binary_dilation with the reference's structure; the argument
checks of the new entry points, which run before the library is touched; the ABI."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import validate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, TM = cases.MARGIN, cases.TIME_MARGIN


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def _same_variables(got, golden):
    """`got` {name: (array, dims)} against one case of the fixture: the same names, dims, dtypes and values"""
    dims = dict(entry.split("=") for entry in golden["dims"])
    assert set(got) == set(dims) == set(golden) - {"dims"}
    for name, (value, value_dims) in got.items():
        assert ",".join(value_dims) == dims[name], name
        _same(value, golden[name])


def test_fixture_inputs_are_the_cases_of_this_module():
    g = cases.golden()["inputs"]
    for name, value in cases.product().items():
        _same(value, g[name])
    _same(cases.flash_grid(), g["glm_grid_raw"])
    _same(cases.flash_times().astype(np.int64), g["times"])
    grid, glm_distance, edge, n_in = cases.script_inputs()
    _same(grid, g["glm_grid"])
    _same(glm_distance, g["glm_distance"])
    _same(edge, g["edge_filter"])
    assert n_in == g["n_glm_in_margin"] == 9 and (grid[edge] > 1).any()


def test_the_product_has_what_the_subsets_and_the_cut_need():
    p = cases.product()
    index, core, anvil = p["core_anvil_index"], p["core"], p["anvil"]
    assert (index == 0).any() and not np.isin(anvil, index).all()                 # a core without an anvil, an anvil without a core
    cut = cases.cut_to_present(p)
    for name in ("core", "anvil", "anvil_marker"):
        assert cut[name].size == p[name].size - 1                                 # one id of each coordinate is in no volume
    assert 6 in cut["anvil"] and 6 not in p["thick_anvil_label"] and cut["core_anvil_index"].size == cut["core"].size
    sets = cases.restate_subsets(p)
    assert list(sets) == list(cases.SETS)
    assert 0 < sets["core_with_anvil"][1].size < core.size and 0 < sets["anvil_with_core"][1].size < anvil.size


@pytest.mark.parametrize("get_closest", [0, 1])
def test_restatement_of_the_wrappers_equals_the_reference(get_closest):
    grid, glm_distance, edge, n_in = cases.script_inputs()
    got = cases.restate_wrappers(cases.product(), grid, glm_distance, edge, n_in, M, TM, bool(get_closest))
    _same_variables(got, cases.golden()[f"wrappers{get_closest}"])


@pytest.mark.parametrize("get_closest", [0, 1])
def test_restatement_of_the_script_equals_the_reference(get_closest):
    raw = cases.flash_grid()
    got = cases.restate_detection(cases.product(), raw, cases.flash_times(), M, TM, bool(get_closest))
    golden = cases.golden()[f"stage{get_closest}"]
    _same_variables(got, golden)
    _same(raw, cases.flash_grid())
    assert golden["flash_count_total"] == 15 and golden["flash_count_in_margin"] == 9
    for name in cases.SETS:                                                       # nothing trivially 0, 1 or NaN
        assert 0 < golden[f"{name}_pod"] < 1 and 0 < golden[f"{name}_far"] < 1 and golden[f"{name}_count_in_margin"] >= 2
        assert golden[f"{name}_pod"].dtype == golden[f"{name}_far"].dtype == np.float32
        assert golden[f"{name}_count_in_margin"].dtype == np.int32 and golden[f"{name}_margin_flag"].dtype == np.bool_
    # an id that is in no volume: present in the wrappers' case (NaN, False), cut from the stage's
    wrappers = cases.golden()[f"wrappers{get_closest}"]
    assert np.isnan(wrappers["core_glm_distance"][-1]) and not wrappers["core_margin_flag"][-1]
    assert wrappers["core_glm_distance"].size == golden["core_glm_distance"].size + 1


def test_the_flashes_where_a_label_is_a_choice_are_a_minority():
    grid = cases.script_inputs()[0]
    for name, (labels, _) in cases.restate_subsets(cases.product()).items():
        ties = cases.tie_flashes(labels, grid, TM)[0]
        assert ties.size == 9 and 2 * ties.sum() < ties.size, name
        assert ties.sum() == (1 if name.startswith("core") else 0), name         # the allowance for a choice is used, once


@pytest.mark.parametrize("margin", cases.EDGE_MARGINS)
@pytest.mark.parametrize("time_margin", [0, 1, 2])
def test_footprint_rule_equals_scipy_with_the_reference_structure(margin, time_margin):
    structure = cases.reference_structure(margin, time_margin)
    assert structure.shape == (2 * time_margin + 1, 2 * margin + 1, 2 * margin + 1) and structure.any() == (margin != 3)
    for name, grid in cases.missing_cases().items():
        missing = grid == -1
        assert missing.any() == (name not in ("absent", "nan")), name
        want = ndi.binary_dilation(missing, structure=structure)
        got = cases.footprint_dilation(missing, margin, time_margin)
        assert np.array_equal(got, want), (name, margin, time_margin)
    if margin == 10:                                                              # the centred open disc
        dy, dx = np.mgrid[-10:11, -10:11]
        assert np.array_equal(structure[0], dy * dy + dx * dx < 100)


# ---- input validation: before the library is touched ---------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    from tobac_flow_amd import _lib

    def refuse(*args, **kwargs):
        raise AssertionError("the library was touched before the inputs were validated")
    for name in ("lib", "device", "to_dev", "torch"):
        monkeypatch.setattr(_lib, name, refuse)


def test_bad_inputs_raise_before_the_library_is_touched(no_library):
    from tobac_flow_amd import validation as v
    from tobac_flow_amd.dataset import LabelDataset
    labels = cases.product()["core_label"]
    grid = np.zeros(labels.shape)
    edge = np.ones(labels.shape, bool)
    for value in (-1.0, -0.5, np.nan):
        counts = grid.copy()
        counts[3, 4, 5] = value
        with pytest.raises(ValueError, match="negative"):
            v.flash_list(counts)
        with pytest.raises(ValueError, match="negative"):
            v.validate_markers(labels, counts, grid, edge, 1)
    with pytest.raises(ValueError, match="time_margin"):
        v.validate_markers(labels, grid, grid, edge, 1, time_margin=-1)
    with pytest.raises(ValueError, match="id < 1"):                               # the last check, still in front of the flash list
        v.validate_markers(labels, grid, grid, edge, 1, coord=[0, 1])
    for coord in ([[1, 2]], [1.5]):
        with pytest.raises(ValueError, match="one-dimensional sequence of integer"):
            v.validate_markers(labels, grid, grid, edge, 1, coord=coord)
    counts = grid.copy()
    counts[3, 4, 5] = -1
    with pytest.raises(ValueError, match="negative"):                             # of two bad arguments the counts are named, as ever
        v.validate_markers(labels, counts, grid, edge, 1, coord=[0, 1])
    product, ds = cases.product(), LabelDataset()
    for wrapper in (v.validate_cores_with_anvils, v.validate_anvils_with_cores):  # the subset remap is device work: checks first
        with pytest.raises(ValueError, match="same shape"):
            wrapper(product, ds, grid[:, :-1], grid, edge, 1, M, TM)
        with pytest.raises(ValueError, match="time_margin"):
            wrapper(product, ds, grid, grid, edge, 1, M, -1)
    with pytest.raises(ValueError, match="same shape"):
        v.validate_detection(product, {"glm_flashes": grid[:5], "t": cases.flash_times()[:5]}, M, TM)
    with pytest.raises(ValueError, match="not listed"):
        v.validate_markers(labels, grid, grid, edge, 1, flashes=v.FlashList(np.zeros(0, np.int64), (1, 2, 3)))
    with pytest.raises(ValueError, match="volume"):
        v.get_edge_filter_dev({"glm_flashes": grid[0], "t": cases.flash_times()}, M, TM)
    with pytest.raises(ValueError, match="negative"):
        v.get_edge_filter_dev({"glm_flashes": grid, "t": cases.flash_times()}, -1, TM)
    with pytest.raises(ValueError, match="volume"):
        v.validate_detection(cases.product(), {"glm_flashes": grid[0], "t": cases.flash_times()}, M, TM)


def test_abi_version_and_entry_points():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    assert L.tf_version() >= 118
    for name in ("tf_flash_tile", "tf_flash_workspace_bytes", "tf_flash_count", "tf_flash_list", "tf_edt_cylinder_at",
                 "tf_grid_has_missing", "tf_edge_filter_workspace_bytes", "tf_edge_filter"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS and hasattr(L, name)
    tile = L.tf_flash_tile()
    assert tile > 0 and tile % 256 == 0
    # two head words and one offset per tile and one more; nothing for a shape the entry points reject
    assert L.tf_flash_workspace_bytes(0) == 0 and L.tf_flash_workspace_bytes(3 * tile + 5) >= 8 * (2 + 4 + 1)
    assert L.tf_flash_workspace_bytes(16 * 5424 * 5424) < 4 << 20
    # the dilation's row counts: none without missing data, bounded by the chunk of frames with it
    assert L.tf_edge_filter_workspace_bytes(16, 5424, 5424, 0) == 0
    assert 4 * 5424 * 5425 <= L.tf_edge_filter_workspace_bytes(16, 5424, 5424, 1) <= (1 << 30) + 1024


def test_the_stage_is_exported_under_the_reference_names():
    from tobac_flow_amd import validation as v
    for name in ("validate_cores", "validate_cores_with_anvils", "validate_anvils", "validate_anvils_with_cores",
                 "validate_anvil_markers", "validate_detection", "get_edge_filter_dev", "flash_list"):
        assert name in v.__all__ and callable(getattr(v, name))
    import inspect
    order = ["detection_ds", "validation_ds", "glm_grid", "glm_distance", "edge_filter_array", "n_glm_in_margin", "margin",
             "time_margin", "get_closest"]
    for name in v.__all__:
        if name.startswith("validate_") and name not in ("validate_markers", "validate_detection"):
            assert list(inspect.signature(getattr(v, name)).parameters)[:9] == order
