"""The yardsticks of the GLM validation without a device: the NumPy / SciPy restatement of tests/validation_cases.py
against the reference's own results in tests/golden/validation_ref.npz (exactly: everything is an integer squared
distance and one square root), the brute-force tie sets against both, the input validation of
tobac_flow_amd.validation, and the kernel bodies compiled for the host (tools/edt_host_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import validation_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, TM = vc.MARGIN, vc.TIME_MARGIN


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def test_fixture_inputs_are_the_cases_of_this_module():
    g = vc.golden()
    _same(vc.boxes(), g["boxes"]["labels"])
    _same(vc.borders(), g["borders"]["labels"])
    _same(vc.flash_grid(), g["boxes"]["glm_grid_raw"])
    _same(vc.label_index(vc.boxes()), g["boxes"]["index"])
    _same(vc.flash_times(6).astype(np.int64), g["boxes"]["times"])
    _same(vc.flash_times(6, gap_after=2).astype(np.int64), g["boxes"]["times_gap"])


def test_restatement_of_the_distances_equals_the_reference():
    a, b = vc.golden()["boxes"], vc.golden()["borders"]
    for time_range in (1, 2):
        _same(vc.restate_marker_distance(a["labels"], time_range), a[f"marker_distance_{time_range}"])
    for tm in (0, 2, 7):
        _same(vc.restate_cylinder(a["labels"], tm), a[f"cylinder_{tm}"])
        dist, closest = vc.restate_cylinder(a["labels"], tm, get_closest=True)
        _same(dist, a[f"cylinder_{tm}_closest_distance"])
        _same(closest, a[f"cylinder_{tm}_closest"])
    _same(vc.restate_marker_distance(b["labels"], 1), b["marker_distance_1"])
    dist, closest = vc.restate_cylinder(b["labels"], 1, get_closest=True)
    _same(dist, b["cylinder_1_closest_distance"])
    _same(closest, b["cylinder_1_closest"])
    assert np.isinf(a["cylinder_0"][2]).all() and np.isinf(a["cylinder_0"][5]).all() and not np.isinf(a["cylinder_7"]).any()
    # the two fmin statements per step are not a plain +- time_range window
    assert not np.array_equal(a["marker_distance_2"], a["cylinder_2"])


def test_restatement_of_the_script_sequence_equals_the_reference():
    a = vc.golden()["boxes"]
    grid, glm_distance, edge, n_in, _ = vc.script_inputs(a["labels"])
    _same(glm_distance, a["glm_distance"])
    _same(edge, a["edge_filter"])
    _same(grid, a["glm_grid"])
    assert n_in == a["n_glm_in_margin"] and not np.isnan(grid).any() and np.isnan(a["glm_grid_raw"]).sum() == 1
    _same(vc.restate_edge_filter(grid, a["times_gap"], M, TM), a["edge_filter_gap"])
    for get_closest in (False, True):
        got = vc.restate_validate_markers(a["labels"], grid, glm_distance, edge, n_in, a["index"], M, TM, get_closest)
        names = ("flash_distance", "flash_closest", "marker_distance", "pod", "far", "n_marker_in_margin", "margin_flag")
        for name, value in zip(names, got):
            key = f"validate_{int(get_closest)}_{name}"
            if value is None:
                assert key not in a
            elif name in ("pod", "far", "n_marker_in_margin"):
                assert value == a[key] and 0 < value
            else:
                _same(value, a[key])
        assert 0 < got[3] < 1 and 0 < got[4] < 1 and got[0].size == n_in
    field, special = vc.distance_field_with_specials(a["labels"], a["glm_grid_raw"])
    _same(field, a["special_field"])
    got = vc.restate_label_nanmin(a["labels"], field, a["index"], np.nan)
    _same(got, a["special_min"])
    row = {int(i): k for k, i in enumerate(a["index"])}
    assert np.isnan(got[row[special["all_nan"]]]) and np.isnan(got[row[special["absent"]]]) and np.isposinf(got[row[special["over_inf"]]])


@pytest.mark.parametrize("case,tm", [("boxes", 0), ("boxes", 2), ("boxes", 7), ("borders", 1)])
def test_brute_force_agrees_with_the_reference_and_every_difference_of_a_choice_is_a_tie(case, tm):
    c = vc.golden()[case]
    d2, count, sets, values = vc.brute_force(c["labels"], tm)
    dist, closest = c[f"cylinder_{tm}_closest_distance"], c[f"cylinder_{tm}_closest"]
    assert np.array_equal(np.where(d2 < 0, np.inf, np.sqrt(np.maximum(d2, 0).astype(np.float64))), dist)      # bit for bit
    assert vc.in_set(closest, sets, values).all()
    assert (count > 1).any() and (count == 1).any() and ((sets != 0) & ~vc.single_label(sets)).any()
    assert (closest[sets == 0] == 0).all()


def test_edge_filter_of_the_module_equals_the_reference_in_all_three_branches():
    from tobac_flow_amd import validation as v
    from types import SimpleNamespace
    a = vc.golden()["boxes"]
    raw = a["glm_grid_raw"]
    _same(v.get_edge_filter(SimpleNamespace(glm_flashes=raw, t=vc.flash_times(6)), M, TM), a["edge_filter"])
    _same(v.get_edge_filter({"glm_flashes": raw, "t": a["times_gap"]}, M, TM), a["edge_filter_gap"])
    _same(v.get_edge_filter({"glm_flashes": a["glm_grid_missing"], "t": a["times"]}, M, TM), a["edge_filter_missing"])
    assert a["edge_filter_missing"].sum() < a["edge_filter"].sum() and a["edge_filter_gap"].sum() < a["edge_filter"].sum()


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
    labels = vc.boxes()
    grid = np.zeros(labels.shape)
    edge = np.ones(labels.shape, bool)
    for bad in (labels[0], labels[None], labels[:0]):
        with pytest.raises(ValueError, match="volume"):
            v.get_marker_distance_cylinder(bad, 1)
        with pytest.raises(ValueError, match="volume"):
            v.get_marker_distance(bad)
        with pytest.raises(ValueError, match="volume"):
            v.validate_markers(bad, grid, grid, edge, 1)
    with pytest.raises(ValueError, match="time_margin"):
        v.get_marker_distance_cylinder(labels, -1)
    with pytest.raises(ValueError, match="same shape"):
        v.get_min_dist_for_objects(grid[:, :, :5], labels)
    for k in range(3):
        operands = [grid, grid, edge]
        operands[k] = operands[k][:, :-1]
        with pytest.raises(ValueError, match="same shape"):
            v.validate_markers(labels, *operands, 1)
    with pytest.raises(ValueError, match="id < 1"):
        v.get_min_dist_for_objects(grid, labels, index=[1, 0])
    for value in (-1.0, np.nan):
        counts = grid.copy()
        counts[3, 4, 5] = value
        with pytest.raises(ValueError, match="negative"):
            v.validate_markers(labels, counts, grid, edge, 1)
    with pytest.raises(ValueError, match="negative"):
        v.validate_markers(labels, vc.flash_grid(), grid, edge, 1)           # the unfiltered grid holds a NaN count
    with pytest.raises(NotImplementedError, match="integer-exact"):
        v.get_marker_distance_ellipse(labels, 3, 10)


def test_abi_version_and_entry_points():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 103
    for name in ("tf_edt2d_frames", "tf_edt2d_frames_workspace_bytes", "tf_edt_cylinder", "tf_label_nanmin", "tf_label_nanmin_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    # shapes the entry point rejects need no workspace; the chunk of frames keeps the workspace bounded
    assert L.tf_edt2d_frames_workspace_bytes(1, 46342, 2) == 0 and L.tf_edt2d_frames_workspace_bytes(1, 32769, 32769) == 0
    one, many = L.tf_edt2d_frames_workspace_bytes(1, 5424, 5424), L.tf_edt2d_frames_workspace_bytes(10000, 5424, 5424)
    assert one >= 4 * 5424 * 5424 and many <= (1 << 30) + 1024
    assert L.tf_edt2d_frames_workspace_bytes(1, 2, 16500) >= 2 * 4 * 2 * 16500


def test_kernel_bodies_on_the_host_against_brute_force(tmp_path):
    """tools/edt_host_check.cpp: the bodies of csrc/edt_kernels.h compiled for the CPU and run lane after lane on
    exactly-sized buffers (its first lines give the AddressSanitizer / UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "edt_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "edt_host_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout + out.stderr
