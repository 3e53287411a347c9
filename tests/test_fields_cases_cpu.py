"""The yardstick of the field preparation checked against answers worked out by hand, the host half of
tobac_flow_amd.dataloader (frame_table) and the build-time facts of csrc/fields.hip.  No GPU is needed."""
import ctypes
import warnings
from datetime import timedelta

import numpy as np
import pytest

import fields_cases as fc
import test_kernel_resources_cpu as kr


# ---- the restatement against hand-written answers ------------------------------------------------------------------------
def test_stripe_deviation_of_a_plane_worked_by_hand():
    # frame 0: row 1 is a stripe of ones.  Every column has mean 1/3 and std sqrt(2)/3, so a one gives
    # (2/3) / (sqrt(2)/3) = sqrt(2) and a zero -1/sqrt(2); the 1e-8 moves both by parts in 10^8.
    # frame 1: one flag in column 0, the other columns constant zero: their std is 0 and their terms 0 / 1e-8 = 0.
    d = np.zeros((2, 3, 4), np.uint8)
    d[0, 1, :] = 1
    d[1, 2, 0] = 1
    dev = fc.stripe_deviation(fc.dqf_float(d))
    r2 = np.sqrt(2.0)
    assert np.allclose(dev[0], [1 / r2, r2, 1 / r2], rtol=1e-7, atol=0)
    assert np.allclose(dev[1], [1 / r2 / 4, 1 / r2 / 4, r2 / 4], rtol=1e-7, atol=0)
    assert not (dev > fc.THRESHOLD).any()


def test_a_fill_is_left_out_of_every_mean():
    d = np.zeros((1, 3, 4), np.uint8)
    d[0, 1, :] = 1
    d[0, :, 3] = 255                                              # a column of nothing but fill: no term anywhere
    d[0, 0, 0] = 255                                              # column 0 keeps rows 1 and 2: mean 1/2, std 1/2
    dev = fc.stripe_deviation(fc.dqf_float(d, 255))
    r2 = np.sqrt(2.0)
    # row 0: columns 1, 2 -> -1/sqrt(2); row 1: 1, sqrt(2), sqrt(2); row 2: -1, -1/sqrt(2), -1/sqrt(2)
    assert np.allclose(dev[0], [1 / r2, (1 + 2 * r2) / 3, (1 + r2) / 3], rtol=1e-7, atol=0)
    d[0, 0, :] = 255                                              # a row of nothing but fill has no deviation and no flag
    dev = fc.stripe_deviation(fc.dqf_float(d, 255))
    assert np.isnan(dev[0, 0]) and not (dev > fc.THRESHOLD)[0, 0]


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_the_kernel_form_reproduces_numpy_columns_bit_for_bit(shape):
    """exact integer count and sum give np.nanmean's column mean, the row-ordered second pass np.nanstd's column std,
    both bit for bit; the deviation then differs by the summation order along x only and stays within the bound of the
    GPU test.  (The variance from integer moments, (n sum D^2 - (sum D)^2) / n^2, is more accurate than NumPy's and
    misses that bound on the 1030-row case by a factor of five: the difference is the rounding of NumPy's own sum.)"""
    import warnings as w
    for d, fill in fc.goes_case(shape)["dqf"]:
        da = fc.dqf_float(d, fill)
        want = fc.stripe_deviation(da)
        got, mean, std = fc.stripe_deviation_kernel_form(d, fill)
        with w.catch_warnings():
            w.simplefilter("ignore", RuntimeWarning)
            assert np.array_equal(mean, np.nanmean(da, 1), equal_nan=True)
            assert np.array_equal(std, np.nanstd(da, 1), equal_nan=True)
        assert np.array_equal(np.isnan(want), np.isnan(got))
        ok = ~np.isnan(want)
        assert (np.abs(got - want)[ok] <= fc.dev_bound(da)[ok]).all()
        assert np.array_equal(got > fc.THRESHOLD, want > fc.THRESHOLD)


def test_decode_with_fill_and_unsigned():
    raw = np.array([0, 1, -1, -2, 32767, -32768], np.int16)
    s, o = np.float32(0.5), np.float32(100.25)
    signed = fc.decode(raw, s, o, fill=-1)
    assert signed.dtype == np.float32
    assert np.array_equal(signed, np.array([100.25, 100.75, np.nan, 99.25, 16483.75, -16283.75], np.float32), equal_nan=True)
    unsigned = fc.decode(raw, s, o, fill=65535, unsigned=True)
    assert np.array_equal(unsigned, np.array([100.25, 100.75, np.nan, 32867.25, 16483.75, 16484.25], np.float32), equal_nan=True)
    # two float32 roundings, not a fused multiply-add: with C13's packing the two differ at raw = 143
    s, o = np.float32(0.06145), np.float32(89.62)
    fused = np.float32(np.float64(143) * np.float64(s) + np.float64(o))
    got = fc.decode(np.array([143], np.int16), s, o)[0]
    assert got == np.float32(np.float32(143) * s) + o and got != fused


def test_prepare_masks_jointly_and_clamps():
    a = np.array([[[1, np.inf, 3, 4]]], np.float32)
    b = np.array([[[2, 1, np.nan, 1]]], np.float32)
    t = np.array(["2020-01-01"], "datetime64[ns]")
    (x, y), n_masked, _ = fc.prepare([a, b], ((0, None, None), (0, 1, 0.0)), t)
    assert np.array_equal(x, [[[1, np.nan, np.nan, 4]]], equal_nan=True)
    assert np.array_equal(y, [[[0, np.nan, np.nan, 3]]], equal_nan=True) and n_masked.tolist() == [2]
    # -inf under the clamp is 0, finite: seviri_nat_dataloader clamps before it looks for non-finite values
    (y,), n_masked, _ = fc.prepare([np.array([[[-np.inf, 1]]], np.float32)], ((0, None, 0.0),), t)
    assert np.array_equal(y, [[[0, 1]]]) and n_masked.tolist() == [0]


# ---- dataloader.frame_table ----------------------------------------------------------------------------------------------
def minutes(*m, unit="ns"):
    """12:00 plus so many (fractions of) minutes"""
    ns = np.round(np.array(m, np.float64) * 60e9).astype(np.int64).astype("timedelta64[ns]")
    return np.datetime64("2020-03-01T12:00:00", unit) + ns.astype(f"timedelta64[{unit}]")


def both(t, time_gap=None, keep=None):
    from tobac_flow_amd import dataloader
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # the dropped frames; pandas on nanoseconds it discards
        got, want = dataloader.frame_table(t, time_gap, keep), fc.frame_table(t, time_gap, keep)
    assert got[0].dtype == np.int32 and got[1].dtype == t.dtype
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def test_frame_table_sorts_unsorted_times():
    src, t_out = both(minutes(10, 0, 5, 15), timedelta(minutes=15))
    assert src.tolist() == [1, 2, 0, 3] and np.array_equal(t_out, minutes(0, 5, 10, 15))


def test_frame_table_fills_two_gaps_one_after_the_other():
    src, t_out = both(minutes(0, 5, 40, 75, 80), timedelta(minutes=15))
    assert src.tolist() == [0, 1, -1, 2, -1, 3, 4]
    assert np.array_equal(t_out, minutes(0, 5, 22.5, 40, 57.5, 75, 80))
    # a gap of exactly time_gap is no gap
    assert both(minutes(0, 15), timedelta(minutes=15))[0].tolist() == [0, 1]
    assert both(minutes(0, 15), None)[0].tolist() == [0, 1]


def test_frame_table_keep_drops_frames_with_a_warning():
    from tobac_flow_amd import dataloader
    t = minutes(-600, 5, 0, 10)
    with pytest.warns(RuntimeWarning, match="Invalid time stamps"):
        src, t_out = dataloader.frame_table(t, timedelta(minutes=15), keep=np.array([False, True, True, True]))
    assert src.tolist() == [2, 1, 3] and np.array_equal(t_out, minutes(0, 5, 10))
    both(t, timedelta(minutes=15), keep=np.array([False, True, True, True]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                            # nothing dropped: no warning
        assert dataloader.frame_table(t[1:], None, keep=np.ones(3, bool))[0].tolist() == [1, 0, 2]


def test_frame_table_of_one_frame():
    src, t_out = both(minutes(7), timedelta(minutes=15))
    assert src.tolist() == [0] and np.array_equal(t_out, minutes(7))


def test_frame_table_duplicates_raise():
    from tobac_flow_amd import dataloader
    with pytest.raises(RuntimeError, match="Duplicate time steps in input index values"):
        dataloader.frame_table(minutes(0, 5, 0), timedelta(minutes=15))
    # a duplicate that `keep` drops is none
    assert both(minutes(0, 5, 0), None, keep=np.array([True, True, False]))[0].tolist() == [0, 1]


def test_frame_table_midpoints_are_datetime64_arithmetic():
    # an odd number of nanoseconds halves downwards, as timedelta64 / 2 does; in seconds the half second is lost
    t = np.array(["2020-03-01T12:00:00.000000000", "2020-03-01T12:20:00.000000001"], "datetime64[ns]")
    _, t_out = both(t, timedelta(minutes=15))
    assert t_out[1] == np.datetime64("2020-03-01T12:10:00.000000000", "ns") == t[0] + (t[1] - t[0]) / 2
    t = np.array(["2020-03-01T12:00:00", "2020-03-01T12:20:01"], "datetime64[s]")
    _, t_out = both(t, timedelta(minutes=15))
    assert t_out.dtype == t.dtype and t_out[1] == np.datetime64("2020-03-01T12:10:00", "s")


def test_the_cases_carry_a_gap_and_unsorted_times():
    case = fc.goes_case(fc.SHAPES[0])
    src, _ = fc.frame_table(case["t"], case["time_gap"])
    assert (src < 0).sum() == 1 and not np.array_equal(src[src >= 0], np.arange(case["shape"][0]))


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_check_their_arguments():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 109
    for name in ("tf_stripe_workspace_bytes", "tf_stripe_deviation", "tf_prepare_fields"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert ctypes.sizeof(_lib.FieldPlane) == 48 and ctypes.sizeof(_lib.FieldRecipe) == 24
    assert ctypes.sizeof(_lib.FieldPrep) == 32 + 16 + 16 * 48 + 4 * 24 + 24
    names = [L.tf_profile_kernel_name(i) for i in range(L.tf_profile_kernel_count())]
    assert {b"stripe_columns", b"stripe_rows", b"prepare_fields"} <= set(names)
    assert L.tf_stripe_workspace_bytes(16, 5424, 5424) >= 4 * 8 * 16 * 5424
    assert L.tf_stripe_workspace_bytes(1, 2 ** 24, 4) == 0 and L.tf_stripe_workspace_bytes(0, 4, 4) == 0
    # every refusal comes before a launch: no device is touched here
    somewhere = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value
    plane = _lib.FieldPlane(data=somewhere, frame_stride=16, row_stride=4, dtype=_lib.TF_U8)
    ws = ctypes.c_void_p(somewhere)
    assert L.tf_stripe_deviation(ctypes.byref(plane), 2, 4, 4, 2.0, None, None, ws, 0, None) == -2      # TF_ENOMEM
    plane.dtype = _lib.TF_F32
    assert L.tf_stripe_deviation(ctypes.byref(plane), 2, 4, 4, 2.0, None, None, ws, 1 << 20, None) == -1
    plane.dtype, plane.row_stride = _lib.TF_U8, 3
    assert L.tf_stripe_deviation(ctypes.byref(plane), 2, 4, 4, 2.0, None, None, ws, 1 << 20, None) == -1
    P = _lib.FieldPrep(T=2, H=4, W=4, T_out=2, n_channels=1, n_recipes=1, src=somewhere)
    P.channel[0] = _lib.FieldPlane(data=somewhere, frame_stride=16, row_stride=4, dtype=_lib.TF_F32)
    P.recipe[0] = _lib.FieldRecipe(a=0, b=1, out=somewhere)
    assert L.tf_prepare_fields(ctypes.byref(P), None) == -1 and b"recipe" in L.tf_last_error()
    P.recipe[0].b, P.channel[0].dtype = -1, _lib.TF_F64
    assert L.tf_prepare_fields(ctypes.byref(P), None) == -1
    P.channel[0].dtype, P.n_dqf = _lib.TF_F32, 9
    assert L.tf_prepare_fields(ctypes.byref(P), None) == -1 and b"DQF" in L.tf_last_error()


FIELD_KERNELS = ["_Z16k_stripe_columns", "_Z17k_stripe_variance", "_Z13k_stripe_rows"] + [
    f"_Z16k_prepare_fieldsILb{p}ELb{d}EE" for p in (0, 1) for d in (0, 1)]


@pytest.fixture(scope="module")
def field_resources(tmp_path_factory):
    if kr._hipcc() is None:
        pytest.skip("no hipcc")
    return kr._resources("fields.hip", str(tmp_path_factory.mktemp("field_resources")))


@pytest.mark.parametrize("kernel", FIELD_KERNELS)
def test_field_kernels_use_no_scratch(field_resources, kernel):
    k = kr._one(field_resources, kernel)
    print(kernel, k)
    assert k["scratch"] == 0
