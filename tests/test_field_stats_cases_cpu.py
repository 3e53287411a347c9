"""get_bulk_stats / get_spatial_stats / get_temporal_stats without a GPU: the float64 yardstick of
tests/field_stats_cases.py against the reference-written fixture (tests/golden/field_stats_ref.npz, made by
tests/golden/make_field_stats_golden.py), the NumPy path of the three public functions against the same fixture, and the
surface: names, dims, dtypes, `ds=`, the export list and the C ABI.

count, median, max and min are compared as values.  mean and std are NumPy sums in the field's own dtype, whose last bits
depend on the CPU's vector width: they are held to the summation bound of field_stats_cases.numpy_bound about the
exactly rounded yardstick."""
import os
import re
import warnings

import numpy as np
import pytest

import field_stats_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = {"all": "get_bulk_stats", "frame": "get_spatial_stats", "time": "get_temporal_stats"}
INFIX = {"all": "", "frame": "spatial_", "time": "temporal_"}
DIMS = {"all": (), "frame": ("t",), "time": ("y", "x")}


def _fixture(dtype, name, over):
    g = fc.golden()
    return {s: g[f"{dtype}/{name}/{over}/{s}"] for s in fc.STATS}


def _hold_against_yardstick(results, dtype, name, over):
    """five arrays of the field's dtype against the yardstick"""
    y = fc.yardstick(name, dtype, over)
    what = f"{dtype} {name} {over}"
    for stat, got in zip(fc.STATS, results):
        assert got.dtype == np.dtype(dtype) and got.shape == y["count"].shape, (what, stat, got.dtype, got.shape)
        if stat in ("mean", "std"):
            fc.hold_bound(got, y[stat], fc.numpy_bound(y, stat, dtype, over) + 0.5 * np.spacing(np.abs(y[stat]).astype(dtype)),
                          f"{what} {stat}")
        else:
            fc.hold_values(got, y[stat].astype(dtype), f"{what} {stat}")
    return y


@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_the_cases_are_the_ones_the_fixture_was_written_for(dtype):
    g = fc.golden()
    for name in fc.fixture_cases(dtype):
        assert str(g[f"{dtype}/{name}/fingerprint"]) == fc.fingerprint(fc.cases(dtype)[name]), name


def test_the_specials_are_what_their_names_say():
    for dtype in fc.DTYPES:
        for n in fc.SPECIAL_LENGTHS + (fc.lds_frames(dtype),):
            sp = fc.special_slices(n, dtype, 600 + n)
            count = {k: int((~np.isnan(v)).sum()) for k, v in sp.items()}
            assert count["all_nan"] == 0 and count["one_value"] == 1
            assert count["even_count"] % 2 == 0 and count["odd_count"] % 2 == 1
            s = np.sort(sp["last_bit"])
            assert np.nextafter(s[n // 2 - 1], s.dtype.type(np.inf)) == s[n // 2]
            s = np.sort(sp["duplicates"])
            run = int((s == s[n // 2]).sum())
            assert s[n // 2 - 1] == s[n // 2] and run == (1000 if n >= 1200 else n // 2)
            assert np.unique(sp["constant"]).size == 1
            assert np.isposinf(sp["plus_inf"]).sum() == 1 and not np.isneginf(sp["plus_inf"]).any()
            assert np.isposinf(sp["both_inf"]).sum() == 1 and np.isneginf(sp["both_inf"]).sum() == 1
            tiny = np.finfo(dtype).tiny
            assert (np.abs(sp["subnormal"]) < tiny).all() and (sp["subnormal"] != 0).sum() >= n - 1
            s = np.sort(sp["overflow_pair"]).astype(np.float32)
            with np.errstate(over="ignore"):
                assert np.isinf(s[n // 2 - 1] + s[n // 2])
            assert np.signbit(sp["signed_zero"][sp["signed_zero"] == 0]).any() and (~np.signbit(sp["signed_zero"][sp["signed_zero"] == 0])).any()
            assert (sp["negative"] < 0).all()


@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_frame_counts_lie_on_both_sides_of_the_single_read_limit(dtype):
    L = fc.lds_frames(dtype)
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    tag = {"float32": "F32", "float64": "F64"}[dtype]
    assert int(re.search(rf"#define TF_FIELD_STATS_LDS_FRAMES_{tag} (\d+)", header).group(1)) == L
    assert L * 256 * np.dtype(dtype).itemsize * 2 <= 160 * 1024            # two workgroups' tiles in a CU's LDS
    assert {L, L + 1, 2 * L + 3} <= set(fc.frame_counts(dtype))
    from tobac_flow_amd import ndimage_dev
    with pytest.raises(TypeError):
        ndimage_dev.FIELD_STATS_LDS_FRAMES["float32"] = 1


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_the_yardstick_equals_the_fixture(dtype, over):
    for name in fc.fixture_cases(dtype):
        if over not in fc.geometries_of(name):
            continue
        f = _fixture(dtype, name, over)
        y = _hold_against_yardstick([f[s] for s in fc.STATS], dtype, name, over)
        shape, rows = fc.slices(fc.cases(dtype)[name], over)
        assert np.array_equal(y["count"], (~np.isnan(rows)).sum(1).reshape(shape))


@pytest.mark.parametrize("over", fc.GEOMETRIES)
@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_the_numpy_path_gives_the_fixtures_names_dims_dtypes_and_values(dtype, over):
    from tobac_flow_amd import dataset
    g = fc.golden()
    names, dims = [str(n) for n in g[f"meta/{over}/names"]], tuple(d for d in str(g[f"meta/{over}/dims"][0]).split(",") if d)
    assert names == [f"field_{INFIX[over]}{s}" for s in fc.STATS] and dims == DIMS[over]
    for name in fc.fixture_cases(dtype):
        if over not in fc.geometries_of(name):
            continue
        a = np.array(fc.cases(dtype)[name])
        ds = dataset.LabelDataset()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = getattr(dataset, PUBLIC[over])(a, ds, name="field")
        assert isinstance(got, tuple) and len(got) == 5 and all(isinstance(v, np.ndarray) for v in got)
        _hold_against_yardstick(got, dtype, name, over)
        f = _fixture(dtype, name, over)
        for stat, v in zip(fc.STATS, got):
            assert v.dtype == f[stat].dtype and v.shape == f[stat].shape
            if stat not in ("mean", "std"):
                fc.hold_values(v, f[stat], f"{name} {stat} against the fixture")
        assert list(ds) == names and all(ds.dims[n] == dims for n in names)
        assert all(ds[n] is v for n, v in zip(names, got))


def test_ds_adds_the_fifteen_variables_and_takes_a_variable_by_name():
    from tobac_flow_amd import dataset
    ds = dataset.LabelDataset()
    ds.add("bt", np.array(fc.cases("float32")["near_2x5x13"]), ("t", "y", "x"))
    for fn in PUBLIC.values():
        out = getattr(dataset, fn)("bt", ds)
        assert len(out) == 5
    want = ["bt"] + [f"bt_{INFIX[o]}{s}" for o in fc.GEOMETRIES for s in fc.STATS]
    assert list(ds) == want and len(want) == 16
    assert [ds.dims[n] for n in want[1:]] == [DIMS[o] for o in fc.GEOMETRIES for _ in fc.STATS]
    assert all(ds[n].dtype == np.float32 for n in want)
    assert ds["bt_spatial_mean"].shape == (2,) and ds["bt_temporal_min"].shape == (5, 13) and ds["bt_median"].shape == ()
    with pytest.raises(ValueError, match="name="):
        dataset.get_bulk_stats(np.zeros((2, 3, 4), np.float32), ds)
    # without ds nothing is added and an array needs no name
    assert len(dataset.get_spatial_stats(np.zeros((2, 3, 4), np.float32))) == 5 and len(ds) == 16


def test_bulk_median_is_np_median_the_others_ignore_nan():
    from tobac_flow_amd import dataset
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    a[0, 0, 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.isnan(dataset.get_bulk_stats(a)[2]) and dataset.get_bulk_stats(a)[0] == np.nanmean(a)
        assert dataset.get_spatial_stats(a)[2][0] == np.nanmedian(a[0]) and dataset.get_temporal_stats(a)[2][0, 0] == 12.0


def test_the_three_names_are_exported():
    from tobac_flow_amd import dataset
    assert {"get_bulk_stats", "get_spatial_stats", "get_temporal_stats"} <= set(dataset.__all__)


def test_c_abi():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 112
    for name in ("tf_field_stats", "tf_field_stats_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    assert "int tf_field_stats(" in header and "size_t tf_field_stats_workspace_bytes(" in header
    # the workspace query is host arithmetic: 0 for arguments the entry point refuses
    q = L.tf_field_stats_workspace_bytes
    assert q(_lib.TF_F32, 16, 100, 100, 0) > 0 and q(_lib.TF_F64, 16, 100, 100, 1) > q(_lib.TF_F64, 1, 100, 100, 1)
    assert q(_lib.TF_F32, 16, 100, 100, 2) > 0
    assert q(_lib.TF_I32, 16, 100, 100, 0) == 0 and q(_lib.TF_F32, 0, 100, 100, 0) == 0 and q(_lib.TF_F32, 16, 100, 100, 3) == 0
    assert q(_lib.TF_F32, 65536, 10, 10, 1) == 0 and q(_lib.TF_F32, 65536, 10, 10, 0) > 0


def test_an_integer_or_bool_tensor_is_a_type_error_before_the_device_is_touched():
    import torch
    from tobac_flow_amd import dataset, ndimage_dev
    for dtype in (torch.int32, torch.bool, torch.float16):
        x = torch.zeros((2, 3, 4), dtype=dtype)
        with pytest.raises(TypeError, match="float32.*float64"):
            ndimage_dev.field_stats(x, "frame")
        with pytest.raises(TypeError, match="float32.*float64"):
            dataset.get_temporal_stats(x)
    with pytest.raises(ValueError, match="at least one value"):
        ndimage_dev.field_stats(torch.zeros((0, 3, 4)), "all")
    with pytest.raises(ValueError, match="over must be"):
        ndimage_dev.field_stats(torch.zeros((1, 3, 4)), "pixel")
    with pytest.raises(ValueError, match=r"\(t, y, x\)"):
        ndimage_dev.field_stats(torch.zeros((3, 4)), "time")
