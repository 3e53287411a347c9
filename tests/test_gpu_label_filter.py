"""tf_label_filter, ndimage_dev.label_filter, the device branch of the ten analysis label filters and the device-resident
detect_growth_markers_multichannel on the GPU, against the NumPy restatement and the reference's own results
(tests/label_filter_cases.py, tests/golden/label_filter_ref.npz) and against the host forms."""
import itertools
import warnings

import numpy as np
import pytest

import label_filter_cases as lc
from helpers import blob_sequence

pytestmark = pytest.mark.gpu


def _eight(case):
    """eight criteria of a volume: its own, its extra ones, then the same again"""
    return list(itertools.islice(itertools.cycle(case["criteria"] + case["extra"]), 8))


def _offset_by_one_element(t_, array):
    """the array on the device in a contiguous tensor whose base is one element past a 16-byte aligned address"""
    src = t_.from_numpy(np.array(array))
    nbytes, size = src.numel() * src.element_size(), src.element_size()
    raw = t_.zeros(nbytes + 16, dtype=t_.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    out = raw[size:size + nbytes].view(src.dtype).view(src.shape)
    out.copy_(src)
    assert out.is_contiguous() and out.data_ptr() % 16 == size
    return out


def _records(labels, n_labels, case, criteria, misaligned=False):
    """tf_label_filter itself: int32[n_labels + 1, 4] as a NumPy array"""
    import torch
    from tobac_flow_amd import _lib
    put = (lambda a: _offset_by_one_element(torch, a)) if misaligned else (lambda a: torch.from_numpy(np.array(a)).cuda())
    lab = put(labels)
    crit = (_lib.LabelCriterion * max(len(criteria), 1))()
    keep = []
    for k, q in enumerate(criteria):
        if q[0] == "mask":
            d = put(case["fields"][q[1]].view(np.uint8))
            crit[k] = _lib.LabelCriterion(d.data_ptr(), _lib.TF_U8, 0, 0.0)
        else:
            d = put(case["fields"][q[0]])
            crit[k] = _lib.LabelCriterion(d.data_ptr(), _lib.TF_F32 if d.dtype == torch.float32 else _lib.TF_F64, _lib.CMP_OPS[q[1]], q[2])
        keep.append(d)
    rec = torch.full((n_labels + 1, 4), 12345, dtype=torch.int32, device="cuda")
    T, H, W = labels.shape
    _lib.check(_lib.lib().tf_label_filter(_lib.ptr(lab), T, H, W, n_labels, crit, len(criteria), _lib.ptr(rec), _lib.stream_ptr()),
               "tf_label_filter")
    return rec.cpu().numpy()


@pytest.mark.parametrize("volume", lc.VOLUMES)
def test_records_equal_the_restatement(volume):
    """0, 1, 3 and 8 criteria; every volume also from tensors whose base is NOT 16-byte aligned (the aligned volume then has
    to take the scalar path)"""
    c = lc.case(volume)
    labels = c["labels"]
    n = max(int(labels.max()), 0)
    for K in (0, 1, 3, 8):
        criteria = _eight(c)[:K]
        want = lc.restate(labels, n, [lc.satisfied(c, q) for q in criteria])
        for misaligned in (False, True):
            got = _records(labels, n, c, criteria, misaligned)
            assert np.array_equal(got, want), (volume, K, misaligned)
    if K == 8 and volume in ("odd", "aligned"):
        assert len(set(want[1:, 2].tolist())) > 2                  # the eight bits tell labels apart


def test_records_ignore_ids_beyond_n_labels_and_negative_labels():
    c = lc.case("odd")
    criteria = c["criteria"]
    truths = [lc.satisfied(c, q) for q in criteria]
    got = _records(c["labels"], 2, c, criteria)
    assert got.shape == (3, 4) and np.array_equal(got, lc.restate(c["labels"], 2, truths))
    signed = c["labels"].copy()
    signed[signed == 3] = -7
    signed[signed == 2] = -2 ** 31
    got = _records(signed, 4, c, criteria)
    assert np.array_equal(got, lc.restate(signed, 4, truths))
    assert got[2].tolist() == got[3].tolist() == [lc.INT_MAX, -1, 0, 0] and got[1, 1] == 1 and got[4, 1] == 2


@pytest.mark.parametrize("volume", lc.VOLUMES)
def test_label_filter_of_ndimage_dev(volume):
    """masks as bool tensors, fields as (tensor, op, threshold); a non-contiguous view of a wider tensor gives the same"""
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    c = lc.case(volume)
    rec = lc.records(volume)[1:].astype(np.int64)
    K = len(c["criteria"])
    dev = {name: torch.from_numpy(np.array(a)).cuda() for name, a in c["fields"].items()}
    labels = torch.from_numpy(c["labels"].copy()).cuda()
    criteria = [dev[q[1]] if q[0] == "mask" else (dev[q[0]], q[1], q[2]) for q in c["criteria"]]

    def check(lengths, hits, present):
        assert lengths.dtype == np.int64 and hits.dtype == bool and present.dtype == bool and hits.shape == (len(rec), K)
        assert np.array_equal(present, rec[:, 1] >= 0)
        assert np.array_equal(lengths, np.where(rec[:, 1] >= 0, rec[:, 1] - rec[:, 0] + 1, 0))
        assert np.array_equal(hits, ((rec[:, 2:3] >> np.arange(K)) & 1).astype(bool))
    check(*nd.label_filter(labels, criteria))
    T, H, W = labels.shape
    wide = torch.zeros((T, H, W + 3), dtype=torch.int32, device="cuda")
    wide[:, :, 1:W + 1] = labels
    view = wide[:, :, 1:W + 1]
    assert not view.is_contiguous() or W == 1
    check(*nd.label_filter(view, criteria))
    check(*nd.label_filter(view.contiguous(), criteria))
    assert nd.label_filter(labels)[1].shape == (len(rec), 0)
    if volume == "odd":                                            # an integer field is compared as float64
        as_int = (dev["g"].nan_to_num() * 3).to(torch.int16)
        assert nd.label_filter(labels, [(as_int, "<=", -5.5)])[1][:, 0].tolist() == [True, False, True, False]
        with pytest.raises(ValueError, match="comparison"):
            nd.label_filter(labels, [(dev["f"], "==", 0.0)])
        with pytest.raises(ValueError, match="shape"):
            nd.label_filter(labels, [dev["f"][:, :, :-1]])
        with pytest.raises(ValueError, match="at most 8"):
            nd.label_filter(labels, [dev["one_voxel"]] * 9)


def _outcome(fn):
    """the result of fn(), or the name of the exception it raises"""
    try:
        return fn()
    except Exception as e:  # noqa: BLE001
        return type(e).__name__


@pytest.mark.parametrize("volume", lc.VOLUMES)
def test_analysis_functions_on_device_tensors_equal_the_host_functions_and_the_reference(volume):
    """every recorded call of the ten functions: device tensors in (masks alternately tensors and host arrays, which are
    uploaded), against the same function on the NumPy copies and against the reference's result.  filter_* return device
    tensors, the legacy forms the very tensor they were given, find_object_lengths / mask_labels NumPy arrays.  The one
    deliberate difference: filter_labels_by_mask with a missing id raises ValueError where the reference returns garbage."""
    import torch
    from tobac_flow_amd import analysis
    c = lc.case(volume)
    masks = [np.array(lc.as_mask(c, q)) for q in c["criteria"]]
    dev_masks = [torch.from_numpy(m).cuda() if k % 2 == 0 else m for k, m in enumerate(masks)]
    for key, name, which, min_length in lc.calls(c):
        want = lc.reference(volume, key)
        given = torch.from_numpy(c["labels"].copy()).cuda()
        got = _outcome(lambda: lc.call(analysis, name, given, None if which is None else [dev_masks[k] for k in which], min_length))
        if volume == "gap" and name == "filter_labels_by_mask":
            assert got == "ValueError"
            with pytest.raises(ValueError, match="label 2 does not occur"):
                analysis.filter_labels_by_mask(given, dev_masks[0])
            continue
        host = _outcome(lambda: lc.call(analysis, name, c["labels"].copy(), None if which is None else [masks[k] for k in which],
                                        min_length))
        if isinstance(want, str):
            assert got == want and host == want, (volume, key, got, host)
            assert np.array_equal(given.cpu().numpy(), c["labels"])                 # nothing was written before the error
            continue
        if name in ("find_object_lengths", "mask_labels"):
            assert isinstance(got, np.ndarray), (volume, key, got)
        else:
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32, (volume, key, got)
            assert (got is given) == ("legacy" in name), (volume, key)
            if "legacy" not in name:
                assert np.array_equal(given.cpu().numpy(), c["labels"])
            got = got.cpu().numpy()
        assert np.array_equal(got, want), (volume, key)
        assert np.array_equal(got, host), (volume, key)


def test_analysis_error_paths_and_axis_on_device_tensors():
    import torch
    from tobac_flow_amd import analysis
    c = lc.case("odd")
    labels = torch.from_numpy(c["labels"].copy()).cuda()
    mask = torch.from_numpy(np.array(c["fields"]["one_voxel"])).cuda()
    for fn in (analysis.filter_labels_by_multimask, analysis.filter_labels_by_length_and_multimask,
               analysis.filter_labels_by_length_and_multimask_legacy):
        with pytest.raises(ValueError, match="must be a list"):
            fn(labels, mask, *([1] if "length" in fn.__name__ else []))
    with pytest.raises(AssertionError, match="same shape"):
        analysis.mask_labels(labels, mask[:, :, :-1])
    for axis in (1, 2):
        assert np.array_equal(analysis.find_object_lengths(labels, axis), analysis.find_object_lengths(c["labels"], axis))
    gap = torch.from_numpy(lc.case("gap")["labels"].copy()).cuda()
    with pytest.raises(TypeError, match="label 2 does not occur"):
        analysis.find_object_lengths(gap)
    zero = torch.zeros((2, 5, 7), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        analysis.filter_labels_by_mask(zero, torch.ones((2, 5, 7), dtype=torch.bool, device="cuda"))
    assert analysis.find_object_lengths(zero).size == 0 and analysis.mask_labels(zero, zero != 0).size == 0
    assert analysis.filter_labels_by_length_legacy(zero, 1) is zero and not zero.any()


# ---- detect_growth_markers_multichannel ---------------------------------------------------------------------------------
PARAMS = dict(min_length=2, lower_threshold=0.05, upper_threshold=0.1)


@pytest.fixture(scope="module")
def three_channels():
    """the scene of tests/test_gpu_configs.py's `three_channels` fixture: seed 77, 8 x 160 x 200"""
    import tobac_flow_amd.flow as tf
    from test_gpu_detection import FakeDataArray
    rng = np.random.default_rng(77)
    bt = blob_sequence(rng, 8, 160, 200, n_blobs=6, vmax=1.5, noise=0.4)
    grow = np.linspace(0.6, 1.4, 8, dtype=np.float32)[:, None, None]
    bt = (290.0 - (290.0 - bt) * grow).astype(np.float32)
    flow = tf.create_flow(bt, vr_steps=1, smoothing_passes=1, interp_method="cubic")
    wvd = FakeDataArray(((250.0 - bt) / 2.0 - 10.0).astype(np.float32), minutes=5)
    return dict(flow=flow, bt=FakeDataArray(bt, minutes=5), wvd=wvd)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


_HOST = {}


def _host(scene, **kw):
    """_detect_growth_markers_multichannel_host of the scene, computed once per parameter set; do not modify"""
    from tobac_flow_amd.detection import _detect_growth_markers_multichannel_host
    key = tuple(sorted(kw.items()))
    if key not in _HOST:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _HOST[key] = _detect_growth_markers_multichannel_host(scene["flow"], scene["wvd"], scene["bt"], **kw)
    return _HOST[key]


def _device_fields(scene):
    import torch
    from tobac_flow_amd.detection import DeviceField
    return [DeviceField(torch.from_numpy(np.asarray(x)).cuda(), np.asarray(x.t.data)) for x in (scene["wvd"], scene["bt"])]


def test_multichannel_on_host_containers_equals_the_host_form(three_channels):
    from tobac_flow_amd.detection import detect_growth_markers_multichannel
    want = _host(three_channels, **PARAMS)
    assert want[2].max() > 0 and (want[2] == 0).any()
    got = detect_growth_markers_multichannel(three_channels["flow"], three_channels["wvd"], three_channels["bt"], **PARAMS)
    assert all(isinstance(g, np.ndarray) for g in got)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and got[2].dtype == want[2].dtype
    # the filter did filter: with min_length = 1 more markers survive
    assert _host(three_channels, **dict(PARAMS, min_length=1))[2].max() >= want[2].max()


def test_multichannel_on_device_fields_returns_device_tensors_equal_to_the_host_form(three_channels):
    import torch
    from tobac_flow_amd.detection import detect_growth_markers_multichannel
    want = _host(three_channels, **PARAMS)
    got = detect_growth_markers_multichannel(three_channels["flow"], *_device_fields(three_channels), **PARAMS)
    assert len(got) == 3 and all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
    assert _same(got[0].cpu().numpy(), want[0]) and _same(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[2].cpu().numpy(), want[2])


def test_multichannel_without_a_candidate_warns_and_returns_empty_labels_on_both_paths(three_channels):
    from tobac_flow_amd.detection import _detect_growth_markers_multichannel_host, detect_growth_markers_multichannel
    kw = dict(PARAMS, lower_threshold=1e6)
    flow, wvd, bt = three_channels["flow"], three_channels["wvd"], three_channels["bt"]
    with pytest.warns(RuntimeWarning, match="No regions detected"):
        want = _detect_growth_markers_multichannel_host(flow, wvd, bt, **kw)
    with pytest.warns(RuntimeWarning, match="No regions detected"):
        got = detect_growth_markers_multichannel(flow, wvd, bt, **kw)
    with pytest.warns(RuntimeWarning, match="No regions detected"):
        dev = detect_growth_markers_multichannel(flow, *_device_fields(three_channels), **kw)
    assert not want[2].any() and not got[2].any() and not dev[2].any().item()
    assert got[2].shape == want[2].shape == tuple(dev[2].shape) and _same(got[0], want[0]) and _same(got[1], want[1])


def test_multichannel_with_subsegmentation_agrees_between_the_two_paths(three_channels):
    from tobac_flow_amd.detection import detect_growth_markers_multichannel
    kw = dict(PARAMS, subsegment_shrink=0.1)
    want = _host(three_channels, **kw)
    assert want[2].max() > 0
    got = detect_growth_markers_multichannel(three_channels["flow"], three_channels["wvd"], three_channels["bt"], **kw)
    assert np.array_equal(got[2], want[2])
    dev = detect_growth_markers_multichannel(three_channels["flow"], *_device_fields(three_channels), **kw)
    assert np.array_equal(dev[2].cpu().numpy(), want[2])
