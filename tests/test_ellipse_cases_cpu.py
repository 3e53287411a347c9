"""The yardsticks of the 3-D distance transform with a time sampling without a device: the NumPy restatement of
tests/ellipse_cases.py (SciPy per frame, then the envelope along t) against the reference's own results in
tests/golden/ellipse_ref.npz under the contract of ellipse_cases.check, the entry point's presence in the C ABI, and the
argument errors of the Python layer, raised before the library is touched."""
import numpy as np
import pytest

import ellipse_cases as ec


def test_fixture_inputs_are_the_volumes_of_this_module():
    results, inputs = ec.golden()
    assert set(inputs) == set(ec.VOLUMES)
    for name, make in ec.VOLUMES.items():
        assert np.array_equal(inputs[name], make()) and inputs[name].dtype == make().dtype
    assert set(results) == {(v, s) for v, s in ec.CASES if v != "none"}
    assert ec.sampling("10_3") == 10 / 3 and ec.sampling("0.3") == 0.3 and ec.sampling("1") == 1 and ec.sampling("3") == 3
    assert not ec.gap()[3].any() and ec.gap()[2].any() and ec.tiny().shape == (1, 5, 7)
    assert [t for t in range(40) if ec.ends()[t].any()] == [0, 39]


@pytest.mark.parametrize("name,sname", ec.CASES)
def test_restatement_keeps_the_contract_against_the_reference(name, sname):
    markers, s = ec.VOLUMES[name](), ec.sampling(sname)
    dist, indices, closest = ec.restate(markers, s)
    exempt, differing = ec.check(name, sname, dist, indices, closest)                                # points 1 - 6
    assert differing <= exempt <= ec.TIE_SHARE_CAP * markers.size
    print(f"{name} at {sname}: {exempt} voxels with several features within 4 eps, {differing} of them differ from SciPy")


def test_the_fixture_holds_the_reference_on_its_own_terms():
    """the stored distances are E at the stored indices, the stored closest markers the values there"""
    results, inputs = ec.golden()
    for (name, sname), r in results.items():
        assert r["distances"].dtype == np.float64 and r["closest"].dtype == inputs[name].dtype
        assert np.array_equal(r["distances"], ec.at_indices(r["indices"], ec.sampling(sname)))
        assert np.array_equal(r["closest"], ec.closest_at(inputs[name], r["indices"]))
    assert any((ec.brute_force(v, s)["count"] > 1).any() for v, s in ec.CASES if s not in ec.INTEGER_SAMPLINGS)


def test_abi_version_and_entry_point():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert "tf_edt_time_envelope" in _lib.EXPORTS and hasattr(L, "tf_edt_time_envelope")
    assert L.tf_version() >= 105


# ---- argument errors: before the library is touched ----------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    from tobac_flow_amd import _lib

    def refuse(*args, **kwargs):
        raise AssertionError("the library was touched before the inputs were validated")
    for name in ("lib", "device", "to_dev"):
        monkeypatch.setattr(_lib, name, refuse)


def test_bad_arguments_of_the_validation_function(no_library):
    from tobac_flow_amd import validation as v
    assert "get_marker_distance_ellipse_dev" in v.__all__
    markers = ec.tiny()
    with pytest.raises(ZeroDivisionError):
        v.get_marker_distance_ellipse_dev(markers, 0, 10)
    for time_margin, margin in ((3, 0), (3, -10), (-3, 10), (3, np.inf), (3, np.nan), (np.float64(0), 10.0), (np.inf, 10)):
        with np.errstate(all="ignore"), pytest.raises(ValueError, match="finite and > 0"):
            v.get_marker_distance_ellipse_dev(markers, time_margin, margin)
    for bad in (markers[0], markers[None], markers[:0]):
        with pytest.raises(ValueError, match="volume"):
            v.get_marker_distance_ellipse_dev(bad, 3, 10)
    with pytest.raises(NotImplementedError, match="integer-exact"):                                  # the old name keeps refusing
        v.get_marker_distance_ellipse(markers, 3, 10)


def test_bad_arguments_of_distance_transform_edt(no_library):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    x = torch.zeros((2, 5, 7), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="at least one"):
        nd.distance_transform_edt(x, return_distances=False, return_indices=False)
    for sampling in ((1, 2, 1), (1, 1, 0.5), (2, 2, 2), 2, 0.5):
        with pytest.raises(ValueError, match="in-plane"):
            nd.distance_transform_edt(x, sampling=sampling)
    with pytest.raises(ValueError, match="in-plane"):
        nd.distance_transform_edt(x[0], sampling=(2, 1))
    for sampling in ((0, 1, 1), (-1, 1, 1), (np.inf, 1, 1), (np.nan, 1, 1)):
        with pytest.raises(ValueError, match="finite and > 0"):
            nd.distance_transform_edt(x, sampling=sampling)
    for sampling in ((1, 1), (1, 1, 1, 1)):
        with pytest.raises(ValueError, match="per axis"):
            nd.distance_transform_edt(x, sampling=sampling)
    for bad in (x[0, 0], x[None], x[:0]):
        with pytest.raises(ValueError, match="tensor is required"):
            nd.distance_transform_edt(bad)
    d2 = torch.zeros((2, 5, 7), dtype=torch.int32)
    for s in (0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="finite and > 0"):
            nd.edt_time_envelope(d2, None, s)
    with pytest.raises(ValueError, match="int32"):
        nd.edt_time_envelope(d2.to(torch.int64), None, 1.0)
    with pytest.raises(ValueError, match="nearest"):
        nd.edt_time_envelope(d2, d2[:1], 1.0)
