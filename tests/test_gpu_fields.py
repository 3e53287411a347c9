"""Field preparation on the GPU (tobac_flow_amd.dataloader, tf_stripe_deviation, tf_prepare_fields) against the NumPy
restatement of tests/fields_cases.py.

The contract: the fields and n_masked equal the restatement bit for bit (no stripe flag hangs on rounding: the cases assert a
margin while they are built); the stripe deviation lies within (W + 4) 2^-53 mean_x |term| of np.nanmean / np.nanstd per row
and is identical in two runs.  Every case runs from 16-byte aligned tensors ("aligned"), from tensors that start one
element later ("shifted": the element-load forms of the kernels) and from a [3:-2, 5:-1] view of a larger frame ("view":
the strides).  The shapes are the smallest at which the kernels can go wrong: (5, 37, 67) odd everything, a tail in every
vector loop, voxel groups that straddle rows; (2, 70, 1100) rows wider than the 1024 columns a workgroup of the column pass
and the 1024 elements a step of the row pass take; (1, 1030, 40) the column pass over several chunks of 256 rows, and
columns long enough for the order of the variance's sum to show."""
import warnings

import numpy as np
import pytest

import fields_cases as fc

pytestmark = pytest.mark.gpu
LAYOUTS = ("aligned", "shifted", "view")


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def place(lib, a, layout):
    """the (T, H, W) array on the device: at the start of an allocation, one element later, or as the [3:-2, 5:-1] cut of
    larger frames whose border holds other values"""
    t = lib.torch()
    if layout == "view":
        border = np.random.default_rng(7).integers(1, 100, tuple(s + p + q for s, (p, q) in zip(a.shape, fc.VIEW_PAD)))
        big = border.astype(a.dtype)
        big[fc.VIEW] = a
        out = t.from_numpy(big).to(lib.device())[fc.VIEW]
        assert not out.is_contiguous() and out.stride(2) == 1
        return out
    shift = 1 if layout == "shifted" else 0
    buf = t.empty(a.size + shift, dtype=t.from_numpy(a[:1]).dtype, device=lib.device())
    buf[shift:] = t.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(lib.device())
    out = buf[shift:].reshape(a.shape)
    assert out.data_ptr() % 16 == (shift * out.element_size()) % 16
    return out


def same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def check_fields(got, case):
    *fields, n_masked = got
    assert len(fields) == len(case["want"])
    for f, want in zip(fields, case["want"]):
        assert same(f.data, want)
        assert np.array_equal(f.t.values, case["t_out"]) and f.t.values.dtype == case["t_out"].dtype
    assert same(n_masked, case["n_masked"])


def goes_operands(lib, case, packed, layout):
    from tobac_flow_amd.dataloader import PackedChannel
    if packed:
        chans = [PackedChannel(place(lib, raw, layout), s, o, fill_value=fc.GOES_FILL, unsigned=True)
                 for raw, (s, o) in zip(case["raws"], fc.GOES_PACKING)]
    else:
        chans = [place(lib, x, layout) for x in case["decoded"]]
    return chans, [(place(lib, d, layout), fill) for d, fill in case["dqf"]]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("packed", (True, False), ids=("packed", "float32"))
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_goes_fields_equal_the_restatement_bit_for_bit(lib, shape, packed, layout):
    """packed unsigned channels with fills in different channels (or float32 with NaN, +inf, -inf), sparse DQF flags, a
    full stripe row, a partial stripe on either side of the threshold, a constant column, DQF fill values, unsorted times
    and a gap"""
    from tobac_flow_amd import dataloader
    case = fc.goes_case(shape, packed)
    chans, dqf = goes_operands(lib, case, packed, layout)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = dataloader.prepare_fields(chans, [(2,), (0, 1), (2, 3)], case["t"], dqf=dqf, time_gap=case["time_gap"], return_masked=True)
    check_fields(got, case)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_seviri_native_fields_clamp_before_the_mask(lib, layout):
    from tobac_flow_amd import dataloader
    case = fc.seviri_nat_case(fc.SHAPES[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bt, wvd, twd = dataloader.seviri_nat_fields(*(place(lib, x, layout) for x in case["chans"]), case["t"])
    for f, want in zip((bt, wvd, twd), case["want"]):
        assert same(f.data, want) and np.array_equal(f.t.values, case["t_out"])


def test_host_arrays_go_in_packed_and_come_back_as_asked(lib):
    """NumPy in: DeviceField's by default (on_device=True), NumPy arrays with on_device=False; a uint16 array is an
    unsigned packed channel; a strided NumPy view is taken by value"""
    from tobac_flow_amd import dataloader
    from tobac_flow_amd.detection import DeviceField
    case = fc.goes_case(fc.SHAPES[0])
    chans = [dataloader.PackedChannel(raw.view(np.uint16), s, o, fill_value=65535) for raw, (s, o) in zip(case["raws"], fc.GOES_PACKING)]
    assert all(c.unsigned and c.fill_value == 65535 for c in chans)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = dataloader.goes_fields(*chans, case["t"], dqf=case["dqf"])
        host = dataloader.goes_fields(*chans, case["t"], dqf=case["dqf"], on_device=False)
    for d, h, want in zip(dev, host, case["want"]):
        assert isinstance(d, DeviceField) and same(d.data, want) and isinstance(h, np.ndarray) and same(h, want)


def stripe_planes(shape):
    return fc.goes_case(shape)["dqf"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_stripe_deviation_within_the_summation_bound(lib, shape, layout):
    """dev within (W + 4) 2^-53 mean_x |term| of np.nanmean / np.nanstd per row, the same flags, identical in two runs"""
    from tobac_flow_amd import dataloader
    for k, (d, fill) in enumerate(stripe_planes(shape)):
        da = fc.dqf_float(d, fill)
        want, bound = fc.stripe_deviation(da), fc.dev_bound(da)
        x = place(lib, d, layout)
        got = dataloader.get_stripe_deviation(x, fill).cpu().numpy()
        again = dataloader.get_stripe_deviation(x, fill).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, again, equal_nan=True)         # identical in two runs
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got > fc.THRESHOLD, want > fc.THRESHOLD)
        ok = ~np.isnan(want)
        err = np.abs(got - want)[ok]
        print(f"plane {k}: max error {err.max():.3e}, max error / bound {(err / bound[ok]).max():.3f}")
        assert (err <= bound[ok]).all(), (k, float(err.max()), float((err / bound[ok]).max()))


def test_frames_follow_the_table(lib):
    """dropped, sorted and gap-filled frames in one pass: the order of the output frames, the NaN frames and their count"""
    from tobac_flow_amd import dataloader
    T, H, W = 6, 9, 13
    rng = np.random.default_rng(3)
    a = rng.random((T, H, W)).astype(np.float32)
    a[1, 2, 3] = np.inf
    t = np.datetime64("2021-07-01T00:00", "s") + np.array([50, 0, 10, 5, 999, 90]) * np.timedelta64(60, "s")
    keep = np.array([True, True, True, True, False, True])
    gap = fc.timedelta(minutes=15)
    (want,), n_masked, t_out = fc.prepare([a], ((0, None, None),), t, time_gap=gap, keep=keep)
    src, _ = fc.frame_table(t, gap, keep)
    assert src.tolist() == [1, 3, 2, -1, 0, -1, 5] and n_masked.tolist() == [1, 0, 0, H * W, 0, H * W, 0]
    with pytest.warns(RuntimeWarning, match="Invalid time stamps"):
        field, got_masked = dataloader.prepare_fields([a], [(0,)], t, time_gap=gap, keep=keep, return_masked=True)
    assert same(field.data, want) and same(got_masked, n_masked) and np.array_equal(field.t.values, t_out)
    # fill_time_gap_nan of a finished field keeps every value, the infinity included
    sorted_field = a[np.argsort(t)]
    filled, t_filled = dataloader.fill_time_gap_nan(sorted_field, np.sort(t), gap)
    src, want_t = fc.frame_table(np.sort(t), gap)
    want = np.full((len(src), H, W), np.nan, np.float32)
    want[src >= 0] = sorted_field[src[src >= 0]]
    assert same(filled, want) and np.isinf(filled).sum() == 1 and np.array_equal(t_filled, want_t)
    dev = dataloader.fill_time_gap_nan(lib.to_dev(sorted_field), np.sort(t), gap)[0]
    assert lib.is_tensor(dev) and same(dev, want)


def test_what_the_kernels_do_not_take_is_refused(lib):
    from tobac_flow_amd import dataloader
    a = np.zeros((2, 5, 6), np.float32)
    d = np.zeros((2, 5, 6), np.uint8)
    t = np.datetime64("2021-07-01T00:00", "s") + np.arange(2) * np.timedelta64(300, "s")
    with pytest.raises(ValueError, match="shape"):
        dataloader.prepare_fields([a, a[:, :4]], [(0, 1)], t)
    with pytest.raises(ValueError, match="shape"):
        dataloader.prepare_fields([a], [(0,)], t, dqf=[d[:, :, :5]])
    with pytest.raises(TypeError, match="float64"):
        dataloader.prepare_fields([a, a.astype(np.float64)], [(0, 1)], t)
    with pytest.raises(TypeError, match="float32"):
        dataloader.prepare_fields([a], [(0,)], t, dqf=[a])
    with pytest.raises(ValueError, match="at most 8 DQF"):
        dataloader.prepare_fields([a], [(0,)], t, dqf=[d] * 9)
    with pytest.raises(ValueError, match="8 channels"):
        dataloader.prepare_fields([a] * 9, [(0,)], t)
    with pytest.raises(TypeError, match="all be float32 or all be packed"):
        dataloader.prepare_fields([a, dataloader.PackedChannel(np.zeros((2, 5, 6), np.int16), 1, 0)], [(0, 1)], t)
    with pytest.raises(TypeError, match="int16"):
        dataloader.PackedChannel(np.zeros((2, 5, 6), np.int32), 1, 0)
    with pytest.raises(ValueError, match="not there"):
        dataloader.prepare_fields([a], [(0, 1)], t)
    with pytest.raises(ValueError, match="2 frames"):
        dataloader.prepare_fields([a], [(0,)], t[:1])
    with pytest.raises(TypeError, match="int8 or uint8"):
        dataloader.get_stripe_deviation(a)


def test_the_kernels_are_timed_with_their_bytes(lib):
    from tobac_flow_amd import dataloader
    case = fc.goes_case(fc.SHAPES[0])
    lib.profile_collect()
    lib.profile_enable(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dataloader.goes_fields(*case["decoded"], case["t"], dqf=case["dqf"])
        prof = lib.profile_collect()
    finally:
        lib.profile_enable(False)
    T, H, W = case["shape"]
    assert prof["stripe_columns"][0] == 4 and prof["stripe_rows"][0] == 4
    calls, ms, nbytes = prof["prepare_fields"]
    # five float32 operands, four DQF bytes and three float32 outputs per voxel of the six output frames
    assert calls == 1 and ms > 0 and nbytes == (T + 1) * H * W * (5 * 4 + 4 + 3 * 4)


def test_goes_fields_feed_create_flow_and_detect_cores(lib):
    """4 x 64 x 96 packed GOES stack -> DeviceField's -> create_flow, detect_cores; the flow equals, bit for bit, the flow of
    the host arrays the restatement makes from the same stack"""
    import tobac_flow_amd.flow as tf
    from helpers import blob_sequence
    from tobac_flow_amd import dataloader
    from tobac_flow_amd.detection import DeviceField, detect_cores
    rng = np.random.default_rng(11)
    shape = (4, 64, 96)
    cold = np.clip(280.0 - blob_sequence(rng, *shape, n_blobs=4, vmax=2.0, noise=0.5), 0, None)
    ramp = np.linspace(0.5, 1.4, shape[0], dtype=np.float32)[:, None, None]
    kelvin = [230.0 + ramp * cold / 6, 238.0 + 0 * cold, 290.0 - ramp * cold, 290.0 - ramp * cold - np.clip(8 - cold / 8, 0, None)]
    raws = [np.round((k - o) / s).astype(np.uint16).view(np.int16) for k, (s, o) in zip(kelvin, fc.GOES_PACKING)]
    dqf = [np.zeros(shape, np.uint8) for _ in range(4)]
    dqf[2][1, 10, 20:23] = 1
    t = np.datetime64("2018-06-19T17:00", "s") + np.arange(shape[0]) * np.timedelta64(120, "s")
    decoded = [fc.decode(raw, s, o, 65535, unsigned=True) for raw, (s, o) in zip(raws, fc.GOES_PACKING)]
    want, _, t_out = fc.prepare(decoded, fc.GOES_RECIPES, t, [fc.dqf_float(d) for d in dqf], fc.timedelta(minutes=15))
    assert np.isnan(want[0]).sum() == 3 and len(t_out) == shape[0]
    chans = [dataloader.PackedChannel(raw, s, o, fill_value=fc.GOES_FILL, unsigned=True) for raw, (s, o) in zip(raws, fc.GOES_PACKING)]
    bt, wvd, swd = dataloader.goes_fields(*chans, t, dqf=dqf)
    assert all(isinstance(f, DeviceField) and same(f.data, w) for f, w in zip((bt, wvd, swd), want))
    flow = tf.create_flow(bt, model="Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")
    host_flow = tf.create_flow(want[0], model="Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")
    for name in ("forward_flow", "backward_flow"):
        got = getattr(flow, name)
        assert same(got, np.asarray(getattr(host_flow, name)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cores = detect_cores(flow, bt, wvd, swd, min_length=2)
    assert lib.is_tensor(cores) and tuple(cores.shape) == shape and int(cores.max()) >= 1
