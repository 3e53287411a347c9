"""subsegment_labels without a GPU: the NumPy restatement of tests/subsegment_cases.py against the reference's own results
(tests/golden/subsegment_ref.npz, scikit-image 0.18.3) on every case without a peak-selection tie, the share of such cases,
the error paths, and the host side of the new entry points."""
import ctypes
import inspect

import numpy as np
import pytest

import subsegment_cases as sc


def test_fixture_covers_the_grid_and_says_how_the_flow_case_was_made():
    z = sc.golden()
    assert str(z["skimage_version"]).startswith("0.18")
    for volume, shrink, distance in sc.CASES:
        assert sc.reference(volume, shrink, distance).shape == sc.masks(volume).shape
    assert {v: sc.masks(v).shape for v in sc.VOLUMES} == {"blobs": (3, 48, 64), "noise": (2, 40, 50), "wide": (2, 33, 300),
                                                          "dumbbell": (3, 40, 90), "pixel": (1, 9, 11), "block": (1, 12, 13),
                                                          "border": (2, 30, 40)}
    dumbbell = sc.masks("dumbbell")
    assert np.array_equal(dumbbell[1], dumbbell[0][:, ::-1]) and not dumbbell[2].any()
    assert sc.masks("pixel").sum() == 1 and sc.masks("block").sum() == 4
    border = sc.masks("border")
    assert border[:, 0].any() and border[:, -1].any() and border[:, :, 0].any() and border[:, :, -1].any()
    assert "integer-valued" in str(z["flow/note"]) and "exact" in str(z["flow/note"])
    f = sc.flow_case()
    assert np.array_equal(f["forward"], np.round(f["forward"])) and np.array_equal(f["backward"], np.round(f["backward"]))
    assert len(np.unique(f["forward"].reshape(-1, 2), axis=0)) > 1


def test_at_least_half_of_the_cases_are_tie_free_and_three_of_every_volume():
    free = {v: sum(sc.tie_free(v, s, d) for s, d in sc.GRID) for v in sc.VOLUMES}
    print("tie-free cases per volume:", free)
    assert all(n >= 3 for n in free.values())
    assert 2 * sum(free.values()) >= len(sc.CASES)
    assert sum(free.values()) < len(sc.CASES)                      # ... and some cases do have a tie: the GPU test runs those too


@pytest.mark.parametrize("volume", sc.VOLUMES)
def test_restatement_equals_the_reference_where_no_peak_tie_exists(volume):
    checked = 0
    for shrink, distance in sc.GRID:
        got = sc.restated(volume, shrink, distance)
        assert got.dtype == np.int32
        if sc.tie_free(volume, shrink, distance):
            want = sc.reference(volume, shrink, distance)
            assert np.array_equal(got, want), (volume, shrink, distance, int((got != want).sum()))
            checked += 1
        assert not got[~sc.masks(volume)].any()
    assert checked >= 3


def test_restatement_equals_the_reference_on_the_flow_case():
    f, p = sc.flow_case(), sc.FLOW_PARAMS
    assert not sc.has_peak_tie(f["mask"], p["subsegment_shrink"], p["peak_min_distance"])
    assert np.array_equal(sc.restate(f["mask"], p["subsegment_shrink"], p["peak_min_distance"]), f["subseg"])
    assert 1 < f["labels"].max() < f["subseg"].max()               # the linking joins subsegments
    assert np.array_equal(f["labels"] != 0, f["subseg"] != 0)


def test_the_rank_key_keeps_the_float64_order_where_float32_does_not():
    a = np.array([[1.0, 1.0 + 2.0 ** -40, 0.25, 1.0 + 2.0 ** -40]])
    assert np.float32(a[0, 0]) == np.float32(a[0, 1])
    assert sc.rank_key(a).tolist() == [[1.0, 2.0, 0.0, 2.0]] and sc.rank_key(a).dtype == np.float32
    assert sc.rank_key(-a).tolist() == [[1.0, 0.0, 2.0, 0.0]]


def test_error_paths_of_the_restatement():
    full = np.zeros((3, 5, 6), bool)
    full[1] = True
    full[0, 2, 2] = True
    with pytest.raises(ValueError, match="frame 1 has no background"):
        sc.restate(full)
    with pytest.raises(ValueError, match="volume is required"):
        sc.restate(np.zeros((5, 6), bool))


def test_entry_points_reject_bad_arguments_before_any_launch():
    """host side of tf_subseg_prepare / tf_subseg_rank: the argument checks return before a kernel is launched, so they
    need no device; the rank overflow (more than 2^24 distinct keys in one frame) is TF_EINVAL -> ValueError"""
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 106
    for name in ("tf_subseg_prepare", "tf_subseg_rank"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = L.tf_subseg_rank(p, 8, p, 2 ** 24 + 1, p, None)
    assert rc == -1
    with pytest.raises(ValueError, match="distinct keys"):
        _lib.check(rc, "tf_subseg_rank")
    assert L.tf_subseg_rank(None, 8, p, 4, p, None) == -1
    assert L.tf_subseg_rank(p, 8, p, 0, p, None) == -1
    assert L.tf_subseg_prepare(p, p, None, 1, 8, 0.1, p, p, None) == -1
    assert L.tf_subseg_prepare(p, p, p, 1, 0, 0.1, p, p, None) == -1
    assert L.tf_subseg_prepare(p, p, p, 1, 8, float("nan"), p, p, None) == -1


def test_public_interface_mirrors_the_reference():
    import tobac_flow_amd.label as label
    from tobac_flow_amd import ndimage_dev
    sig = inspect.signature(label.subsegment_labels)
    assert list(sig.parameters) == ["input_mask", "shrink_factor", "peak_min_distance"]
    assert sig.parameters["shrink_factor"].default == 0.1 and sig.parameters["peak_min_distance"].default == 5
    assert "subsegment_labels" in label.__all__
    assert inspect.signature(ndimage_dev.peak_local_max_2d).parameters["threshold_abs"].default is None
