"""The label filters without a GPU: the NumPy restatement of tf_label_filter (tests/label_filter_cases.py) against the
reference's own results (tests/golden/label_filter_ref.npz), the host side of the new entry point, and the public interface."""
import ctypes
import inspect

import numpy as np
import pytest

import label_filter_cases as lc

# the ten functions and detect_growth_markers_multichannel: parameter lists of the reference (tobac_flow/analysis.py:15-201,
# tobac_flow/detection.py:203-214)
SIGNATURES = {
    "find_object_lengths": ["labels", "axis"],
    "mask_labels": ["labels", "mask"],
    "filter_labels_by_length": ["labels", "min_length"],
    "filter_labels_by_mask": ["labels", "mask"],
    "filter_labels_by_length_and_mask": ["labels", "mask", "min_length"],
    "filter_labels_by_multimask": ["labels", "masks"],
    "filter_labels_by_length_and_multimask": ["labels", "masks", "min_length"],
    "filter_labels_by_length_legacy": ["labels", "min_length"],
    "filter_labels_by_length_and_mask_legacy": ["labels", "mask", "min_length"],
    "filter_labels_by_length_and_multimask_legacy": ["labels", "masks", "min_length"],
}


def test_fixture_holds_the_volumes_the_kernel_can_go_wrong_on():
    assert {v: lc.case(v)["labels"].shape for v in lc.VOLUMES} == {"odd": (3, 33, 67), "aligned": (2, 40, 64), "one": (1, 1, 1),
                                                                   "zero": (2, 5, 7), "gap": (2, 6, 20)}
    for v in lc.VOLUMES:                                           # the stored inputs are the generators' (this NumPy agrees)
        made, stored = lc.GENERATORS[v](), lc.case(v)
        assert np.array_equal(made["labels"], stored["labels"])
        for name, a in made["fields"].items():
            assert np.array_equal(a, stored["fields"][name], equal_nan=a.dtype != bool) and a.dtype == stored["fields"][name].dtype
    odd = lc.case("odd")
    labels, f = odd["labels"], odd["fields"]["f"]
    assert 67 % 16 and 67 % 4 and 64 % 16 == 0
    assert labels[0, 0, 0] == 3 and labels[-1, -1, -1] == 4 and (labels == 3).sum() == (labels == 4).sum() == 1
    assert len(set(np.flatnonzero(labels[0, 5] == 1) // 16)) == 4  # spans several 16-voxel chunks
    assert labels[1, 10, -1] == 2 and labels[1, 11, 0] == 2        # ends at a row's last voxel, goes on at the next row's first
    assert not odd["fields"]["background_only"][labels != 0].any() and odd["fields"]["background_only"].any()
    assert odd["fields"]["one_voxel"].sum() == 1 and labels[odd["fields"]["one_voxel"]] == 1
    assert np.isnan(f[labels != 0]).sum() == 1 and odd["fields"]["g"].dtype == np.float64
    at = (labels != 0) & (f == lc.F32_07)
    assert at.sum() == 1 and f.dtype == np.float32
    assert (f[at] >= 0.7).all() and not (f[at].astype(np.float64) >= 0.7).any()   # passes in float32, would fail in float64
    assert lc.reference("odd", "lengths").tolist() == [2, 2, 1, 1]
    gap = lc.case("gap")["labels"]
    assert set(np.unique(gap)) == {0, 1, 3}


def test_restated_records_of_the_first_volume():
    rec = lc.records("odd")
    assert rec.dtype == np.int32 and rec.shape == (5, 4)
    assert rec[0].tolist() == [lc.INT_MAX, -1, 0, 0]
    assert rec[1:, :2].tolist() == [[0, 1], [1, 2], [0, 0], [2, 2]]
    # bit 0 background only; 1 one voxel of region 1; 2 f >= 0.7 (float32); 3 g < -1; 4 f < 0.5
    assert rec[1:, 2].tolist() == [0b11010, 0b10100, 0b11000, 0b10000]
    beyond = lc.restate(lc.case("odd")["labels"], 2, [])          # ids beyond n_labels are ignored
    assert beyond.shape == (3, 4) and beyond[1:, :2].tolist() == [[0, 1], [1, 2]]
    signed = lc.case("odd")["labels"].copy()
    signed[signed == 3] = -7                                       # negative labels are ignored
    assert lc.restate(signed, 4, [])[3].tolist() == [lc.INT_MAX, -1, 0, 0]


@pytest.mark.parametrize("volume", lc.VOLUMES)
def test_restatement_reproduces_every_result_of_the_reference(volume):
    """tf_label_filter's records, restated in NumPy, give what the reference's ten functions return or raise.  One
    deliberate difference: filter_labels_by_mask on a volume with a missing id, where the reference casts
    labeled_comprehension's None to an integer (garbage) and the device branch raises ValueError."""
    c, rec = lc.case(volume), lc.records(volume)
    checked = 0
    for key, name, which, min_length in lc.calls(c):
        want = lc.reference(volume, key)
        got = lc.from_records(c["labels"], rec, name, which, min_length)
        if volume == "gap" and name == "filter_labels_by_mask":
            assert got == "ValueError" and not isinstance(want, str)
            continue
        if isinstance(want, str):
            assert got == want, (volume, key, got)
        else:
            assert not isinstance(got, str), (volume, key, got)
            assert np.array_equal(got, want), (volume, key)
        checked += 1
    assert checked >= 20


def test_masks_the_reference_saw_are_the_criteria_as_the_kernel_evaluates_them():
    for volume in lc.VOLUMES:
        c = lc.case(volume)
        for q in c["criteria"] + c["extra"]:
            assert np.array_equal(lc.as_mask(c, q), lc.satisfied(c, q)), (volume, q)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """host side of tf_label_filter: the argument checks return TF_EINVAL before a kernel is launched, so they need no device"""
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 107
    assert "tf_label_filter" in _lib.EXPORTS and hasattr(L, "tf_label_filter")
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def crit(*entries):
        a = (_lib.LabelCriterion * max(len(entries), 1))()
        for k, e in enumerate(entries):
            a[k] = _lib.LabelCriterion(*e)
        return a
    ok = (p.value, _lib.TF_F32, _lib.CMP_OPS[">="], 0.5)
    call = lambda labels, n_labels, c, k, rec, shape=(1, 2, 2): L.tf_label_filter(labels, *shape, n_labels, c, k, rec, None)  # noqa: E731
    assert call(None, 1, crit(ok), 1, p) == -1
    assert call(p, 1, crit(ok), 1, None) == -1
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(call(p, 1, crit(ok), 1, None), "tf_label_filter")
    assert call(p, 1, None, 1, p) == -1
    assert call(p, 1, crit(ok), -1, p) == -1
    assert call(p, 1, crit(*[ok] * 9), 9, p) == -1
    assert call(p, -1, crit(ok), 1, p) == -1
    assert call(p, 1, crit((None, _lib.TF_F32, 0, 0.5)), 1, p) == -1
    assert call(p, 1, crit((p.value, _lib.TF_I32, 0, 0.5)), 1, p) == -1
    assert call(p, 1, crit((p.value, 7, 0, 0.5)), 1, p) == -1
    assert call(p, 1, crit((p.value, _lib.TF_F64, 4, 0.5)), 1, p) == -1
    assert call(p, 1, crit((p.value, _lib.TF_F64, -1, 0.5)), 1, p) == -1
    assert call(p, 1, crit((p.value, _lib.TF_F32, 0, float("nan"))), 1, p) == -1
    assert call(p, 1, crit(ok, (p.value, _lib.TF_F64, 1, float("nan"))), 2, p) == -1
    assert call(p, 1, crit(ok), 1, p, (65536, 2, 2)) == -1
    assert call(p, 1, crit(ok), 1, p, (1, 0, 2)) == -1
    assert ctypes.sizeof(_lib.LabelCriterion) == 24


def test_public_interface_mirrors_the_reference():
    from tobac_flow_amd import analysis, detection, ndimage_dev
    for name, params in SIGNATURES.items():
        assert list(inspect.signature(getattr(analysis, name)).parameters) == params, name
    assert inspect.signature(analysis.find_object_lengths).parameters["axis"].default == 0
    sig = inspect.signature(detection.detect_growth_markers_multichannel)
    assert list(sig.parameters) == ["flow", "wvd", "bt", "t_sigma", "overlap", "subsegment_shrink", "min_length",
                                    "lower_threshold", "upper_threshold"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [1, 0.5, 0, 4, 0.25, 0.5]
    assert inspect.signature(detection._detect_growth_markers_multichannel_host) == sig
    assert list(inspect.signature(ndimage_dev.label_filter).parameters) == ["labels", "criteria"]


def test_numpy_inputs_keep_the_host_code_path():
    """the analysis functions on NumPy arrays give the reference's results without touching a device"""
    from tobac_flow_amd import analysis
    for volume in ("odd", "aligned", "one"):
        c = lc.case(volume)
        masks = [lc.as_mask(c, q) for q in c["criteria"]]
        for key, name, which, min_length in lc.calls(c):
            got = lc.call(analysis, name, c["labels"].copy(), None if which is None else [masks[k] for k in which], min_length)
            assert np.array_equal(got, lc.reference(volume, key)), (volume, key)
    for fn in (analysis.filter_labels_by_multimask, analysis.filter_labels_by_length_and_multimask,
               analysis.filter_labels_by_length_and_multimask_legacy):
        with pytest.raises(ValueError, match="must be a list"):
            fn(lc.case("one")["labels"].copy(), lc.case("one")["fields"]["none"], *([1] if "length" in fn.__name__ else []))
