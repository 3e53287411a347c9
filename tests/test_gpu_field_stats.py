"""ndimage_dev.field_stats (tf_field_stats) and the device path of get_bulk_stats / get_spatial_stats / get_temporal_stats
against the exactly rounded yardstick of tests/field_stats_cases.py, which test_field_stats_cases_cpu.py holds against the
reference-written fixture.

Contract (derived in field_stats_cases): count, median, max and min equal NumPy's as values; the float64 mean and std lie
within `bound` of the yardstick and are NaN or infinite exactly where NumPy's are; a public float32 result is off by at
most that bound plus half a float32 ulp; two runs give the same bits; a slice of one repeated float32 value c gives
mean == c and std == 0."""
import numpy as np
import pytest

import field_stats_cases as fc

pytestmark = pytest.mark.gpu

PUBLIC = {"all": "get_bulk_stats", "frame": "get_spatial_stats", "time": "get_temporal_stats"}
KEYS = ("count",) + fc.STATS


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the cases are read-only


def _host(v):
    return v.cpu().numpy()


def _hold(got, y, what):
    """the six outputs of field_stats against a yardstick"""
    import torch
    assert set(got) == set(KEYS), what
    assert got["count"].dtype == torch.int64 and all(got[k].dtype == torch.float64 for k in fc.STATS), what
    assert all(got[k].is_cuda and tuple(got[k].shape) == y["count"].shape for k in KEYS), what
    assert np.array_equal(_host(got["count"]), y["count"]), what
    for k in ("median", "max", "min"):
        fc.hold_values(_host(got[k]), y[k], f"{what} {k}")
    for k in ("mean", "std"):
        fc.hold_bound(_host(got[k]), y[k], fc.bound(y, k), f"{what} {k}")


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_every_case_against_the_yardstick(dtype, over):
    from tobac_flow_amd import ndimage_dev
    for name, a in fc.cases(dtype).items():
        if over in fc.geometries_of(name):
            _hold(ndimage_dev.field_stats(_dev(a), over), fc.yardstick(name, dtype, over), f"{dtype} {name} {over}")


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_public_functions_keep_dtype_shape_and_device(dtype, over):
    import torch
    from tobac_flow_amd import dataset
    from tobac_flow_amd.detection import DeviceField
    L = fc.lds_frames(dtype)
    for name in ("near_3x63x65", "nan_frame_and_column", f"near_T{L + 1}", f"special_frames_n{L}", f"special_columns_n{L}",
                 f"special_overflow_pair_n{L}", f"special_subnormal_n{L}"):
        if over not in fc.geometries_of(name):
            continue
        a = fc.cases(dtype)[name]
        y = fc.yardstick(name, dtype, over)
        x = _dev(a)
        ds = dataset.LabelDataset()
        field = DeviceField(x, np.arange(a.shape[0]).astype("datetime64[s]"))
        for arg in (x, field):
            got = getattr(dataset, PUBLIC[over])(arg, ds, name="f")
            assert isinstance(got, tuple) and len(got) == 5
            for stat, v in zip(fc.STATS, got):
                what = f"{dtype} {name} {over} {stat}"
                assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == x.dtype and tuple(v.shape) == y["count"].shape, what
                if stat in ("mean", "std"):
                    tol = fc.bound(y, stat) + (fc.half_ulp32(y[stat]) if dtype == "float32" else 0)
                    # a float64 value beyond float32's range rounds to infinity
                    with np.errstate(over="ignore"):
                        want = y[stat].astype(dtype).astype(np.float64) if dtype == "float32" else y[stat]
                    fc.hold_bound(_host(v), np.where(np.isinf(want), want, y[stat]), tol, what)
                else:
                    fc.hold_values(_host(v), y[stat], what)
        assert len(ds) == 5 and all(ds[k] is v for k, v in zip(ds, got))


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_a_view_gives_what_its_contiguous_copy_gives(dtype, over):
    import torch
    from tobac_flow_amd import ndimage_dev
    x = _dev(fc.cases(dtype)["near_3x63x65"])
    view = x[:, 1:-1, 2:-3]
    assert not view.is_contiguous()
    a, b = ndimage_dev.field_stats(view, over), ndimage_dev.field_stats(view.contiguous(), over)
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in KEYS)
    if over == "all":
        assert int(a["count"]) == view.numel() and float(a["max"]) == float(view.max())


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_two_runs_are_bit_identical(dtype, over):
    import torch
    from tobac_flow_amd import ndimage_dev
    L = fc.lds_frames(dtype)
    for name in ("mixed_4x129x257", "near_4x129x257", f"near_T{2 * L + 3}", f"near_T{L}"):
        x = _dev(fc.cases(dtype)[name])
        a = ndimage_dev.field_stats(x, over)
        a = {k: v.clone() for k, v in a.items()}
        b = ndimage_dev.field_stats(x, over)
        for k in KEYS:
            assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), (name, k)


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("shape", [(5, 37, 41), (67, 3, 67), (131, 2, 5)])
def test_a_constant_float32_slice_has_its_value_as_mean_and_no_deviation(shape, over):
    import torch
    from tobac_flow_amd import dataset, ndimage_dev
    c = np.float32(251.37109375)                                   # 24 significant bits: every partial sum k c is a float64
    x = torch.full(shape, float(c), dtype=torch.float32, device="cuda")
    got = ndimage_dev.field_stats(x, over)
    assert bool((got["mean"] == float(c)).all()) and bool((got["std"] == 0).all())
    assert bool((got["median"] == float(c)).all()) and bool((got["max"] == float(c)).all()) and bool((got["min"] == float(c)).all())
    mean, std = getattr(dataset, PUBLIC[over])(x)[:2]
    assert mean.dtype == torch.float32 and bool((mean == float(c)).all()) and bool((std == 0).all())


def test_an_empty_tensor_and_an_integer_tensor_raise():
    import torch
    from tobac_flow_amd import dataset, ndimage_dev
    for fn in PUBLIC.values():
        with pytest.raises(ValueError, match="at least one value"):
            getattr(dataset, fn)(torch.zeros((0, 4, 5), device="cuda"))
        for dtype in (torch.int32, torch.bool):
            with pytest.raises(TypeError, match="float32.*float64"):
                getattr(dataset, fn)(torch.zeros((2, 4, 5), dtype=dtype, device="cuda"))
    with pytest.raises(ValueError, match=r"\(t, y, x\)"):
        ndimage_dev.field_stats(torch.zeros((4, 5), device="cuda"), "frame")
    # the bulk form takes any shape
    assert float(ndimage_dev.field_stats(torch.arange(6., device="cuda").reshape(2, 3), "all")["median"]) == 2.5


def test_indices_beyond_2_to_the_31():
    """(2, 1, 2^30 + 3) float32 ones, 8.6 GB, with five planted values in frame 1 at the five flat indices above 2^31: +-1000
    and three times 257.  Every sum is an integer below 2^53, so the float64 sums are exact and the means are the closed forms' own
    divisions; the median stays 1."""
    import torch
    from tobac_flow_amd import ndimage_dev
    N = 2 ** 30 + 3
    x = torch.ones((2, 1, N), dtype=torch.float32, device="cuda")
    at = [2 ** 30 + 1, 2 ** 30 - 1, 2 ** 30 + 2, 2 ** 30 - 2, 2 ** 30]
    planted = [1000.0, -1000.0, 257.0, 257.0, 257.0]
    assert all(N + p > 2 ** 31 and p < N for p in at)
    for p, v in zip(at, planted):
        x[1, 0, p] = v
    extra = sum(planted) - len(planted)                            # what the planted values add to a sum of ones
    assert extra == 766.0

    def std_of(n, mean):
        return np.sqrt(((n - len(planted)) * (1.0 - mean) ** 2 + sum((v - mean) ** 2 for v in planted)) / n)

    got = {k: _host(v) for k, v in ndimage_dev.field_stats(x, "all").items()}
    M = 2 * N
    assert got["count"] == M and got["max"] == 1000.0 and got["min"] == -1000.0 and got["median"] == 1.0
    assert got["mean"] == (M + extra) / M
    s = std_of(M, (M + extra) / M)
    assert abs(got["std"] - s) <= (M + 8) * fc.U * s + M * fc.U * 2.0
    got = {k: _host(v) for k, v in ndimage_dev.field_stats(x, "frame").items()}
    assert got["count"].tolist() == [N, N] and got["max"].tolist() == [1.0, 1000.0] and got["min"].tolist() == [1.0, -1000.0]
    assert got["median"].tolist() == [1.0, 1.0] and got["mean"].tolist() == [1.0, (N + extra) / N]
    s = std_of(N, (N + extra) / N)
    assert got["std"][0] == 0.0 and abs(got["std"][1] - s) <= (N + 8) * fc.U * s + N * fc.U * 2.0
