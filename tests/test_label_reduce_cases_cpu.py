"""The yardsticks of the generic per-label reductions (tf_label_reduce, tf_label_order and the device path of
utils.label_utils.labeled_comprehension / apply_func_to_labels), without a device.

A NumPy restatement of the record's slot arithmetic stands in for the library pass; the package's own finish (slots to
values, NaN rules, default, cast) then has to reproduce the reference's results in tests/golden/label_reduce_ref.npz: the
exact classes bit for bit, the bounded classes within the bounds of tests/label_reduce_cases.hold.  Further: the fixture
equals what SciPy gives here, the dispatch table, NumPy inputs never reach the library, find_overlap_mode against
scipy.stats.mode, the ABI, the kernel bodies compiled for the host, and the register budget of the two pass kernels."""
import functools
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi
import scipy.stats

import label_reduce_cases as lrc
from test_kernel_resources_cpu import _allocated, _hipcc, _one, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lrc.build()


@pytest.fixture(scope="module")
def gold():
    return lrc.golden()


def _key(x):
    """lr_key of csrc/label_runs.h on float64 values, as int64 bit patterns"""
    u = (np.asarray(x, np.float64) + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63)).astype(np.uint64).view(np.int64)


def restated_records(lab, fld, name, ids):
    """what the library pass leaves per id (label_utils._records), from plain NumPy: the eight slots of the record and the
    two middle values"""
    labels, field = np.broadcast_arrays(lab.numpy(), fld.numpy())
    floating = field.dtype.kind == "f"
    rec, mid = np.zeros((len(ids), 8), np.int64), np.full((len(ids), 2), np.nan)
    occurs = set(np.unique(labels).tolist())
    for k, i in enumerate(ids):
        x = field[labels == i] if int(i) in occurs else field[:0].reshape(-1)
        if x.size == 0:
            rec[k, 4] = -1
            continue
        kept = x[~np.isnan(x)] if floating else x
        with np.errstate(all="ignore"):
            total = np.sum(kept.astype(np.float64)) if floating else np.sum(kept.astype(np.int64))
            rec[k, :3] = x.size, kept.size, np.count_nonzero(x)
            rec[k, 3] = np.float64(total).view(np.int64) if floating else total
            rec[k, 4] = _key(kept.astype(np.float64)).view(np.uint64).min().view(np.int64) if kept.size else -1
            rec[k, 5] = _key(kept.astype(np.float64)).view(np.uint64).max().view(np.int64) if kept.size else 0
            if kept.size:
                mean = np.float64(total) / np.float64(kept.size)
                rec[k, 6] = np.float64(np.sum((kept.astype(np.float64) - mean) ** 2)).view(np.int64)
                ordered = np.sort(kept.astype(np.float64)) + 0.0
                mid[k] = ordered[(kept.size - 1) // 2], ordered[kept.size // 2]
    return rec, mid


@pytest.fixture
def restated(monkeypatch):
    """utils.label_utils with the library pass replaced by the restatement: tensors stay on the host"""
    import torch
    from tobac_flow_amd.utils import label_utils as lu
    monkeypatch.setattr(lu, "_to_device", lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)))
    monkeypatch.setattr(lu, "_records", restated_records)
    return lu


def _call(lu, fn, c, func, field):
    if fn == "lc":
        return lu.labeled_comprehension(field, c["labels"], func, index=c["index"], dtype=c["dtype"], default=c["default"])
    return lu.apply_func_to_labels(c["labels"], field, func=func, index=c["index"], default=c["default"])


@pytest.mark.parametrize("name", list(CASES))
def test_restated_slots_and_the_finish_reproduce_the_reference(restated, gold, name):
    import torch
    c = CASES[name]
    field = torch.from_numpy(c["field"])                          # a tensor: the device path; labels stay NumPy, so does the result
    worst = 0.0
    for fn in (("lc", "af") if c["apply"] else ("lc",)):
        for reducer, func in lrc.REDUCERS.items():
            error = lrc.expected_error(gold, f"{fn}/{name}/{reducer}")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if error is not None:
                    with pytest.raises(error):
                        _call(restated, fn, c, func, field)
                    continue
                got = _call(restated, fn, c, func, field)
            assert isinstance(got, np.ndarray) or np.isscalar(got)
            worst = max(worst, lrc.hold(fn, name, reducer, got, c, gold))
    print(name, "largest share of a bound:", worst)


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_is_what_scipy_gives_here(gold, name):
    c = CASES[name]
    labels, field = np.broadcast_arrays(c["labels"], c["field"])
    ids = lrc.ids_of("lc", c)
    for reducer, func in lrc.REDUCERS.items():
        key = f"lc/{name}/{reducer}"
        if lrc.expected_error(gold, key) is not None:
            continue
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            here = ndi.labeled_comprehension(field, labels, ids, func, c["dtype"] or field.dtype, c["default"])
        assert here.dtype == gold[key].dtype and np.array_equal(here, gold[key], equal_nan=here.dtype.kind == "f"), key


def test_dispatch_table_recognises_the_listed_reducers_and_nothing_else():
    from tobac_flow_amd.utils import find_overlap_mode
    from tobac_flow_amd.utils import label_utils as lu
    for reducer, func in lrc.REDUCERS.items():
        assert lu._recognise(func) == ("size" if reducer == "len" else reducer, 0)
        assert lu._recognise(functools.partial(func)) == lu._recognise(func)
    assert lu._recognise(find_overlap_mode) == ("mode", 0)
    assert lu._recognise(functools.partial(find_overlap_mode, background=2)) == ("mode", 2)
    assert len(lu._device_reducers()) == len(lrc.REDUCERS) + 1 == len(lu.DEVICE_REDUCERS)
    for other in (lambda x: np.nanmean(x), np.percentile, np.argmin, np.argmax, functools.partial(np.sum, axis=0),
                  functools.partial(np.percentile, q=50), functools.partial(find_overlap_mode, 3), np.array([1])):
        assert lu._recognise(other) is None


def test_tensors_with_anything_else_are_a_type_error(restated):
    import torch
    c = CASES["tail_f32"]
    field = torch.from_numpy(c["field"])
    for call in (lambda: restated.labeled_comprehension(field, c["labels"], lambda x: x.mean()),
                 lambda: restated.labeled_comprehension(field, c["labels"], np.percentile),
                 lambda: restated.labeled_comprehension(field, c["labels"], np.nanmean, pass_positions=True),
                 lambda: restated.apply_func_to_labels(c["labels"], field, field, func=np.nanmean)):
        with pytest.raises(TypeError, match="np.nanmean.*NumPy arrays"):
            call()
    negative = torch.from_numpy(CASES["negative_labels"]["labels"])
    with pytest.raises(ValueError, match="labels >= 0"):
        restated.apply_func_to_labels(negative, c["field"], func=np.nanmean, default=np.nan)


def test_numpy_inputs_never_reach_the_library(monkeypatch, gold):
    from tobac_flow_amd import _lib
    from tobac_flow_amd.utils import label_utils as lu

    def refuse(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "to_dev", refuse)
    for name in ("tail_f32", "index_mixed", "int32_as_f64", "bool_field"):
        c = CASES[name]
        for reducer, func in lrc.REDUCERS.items():
            for fn in ("lc", "af"):
                key = f"{fn}/{name}/{reducer}"
                if lrc.expected_error(gold, key) is not None:
                    continue
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    got = _call(lu, fn, c, func, c["field"])
                assert got.dtype == gold[key].dtype, key
                if fn == "lc" or reducer in lrc.EXACT or (c["field"].dtype.kind != "f" and reducer in lrc.SUMS):
                    assert np.array_equal(got, gold[key], equal_nan=got.dtype.kind == "f"), key
                else:       # float sums: the host form hands func the values in C order, the reference in its argsort's
                    np.testing.assert_allclose(got, gold[key], rtol=2e-5, equal_nan=True, err_msg=key)
    c = CASES["tail_f32"]
    got = lu.labeled_comprehension(c["field"], c["labels"], lambda x: np.nanmax(x) - 1, default=np.nan)       # any callable
    assert np.array_equal(got, lrc.golden()["lc/tail_f32/nanmax"] - 1, equal_nan=True)


@pytest.mark.parametrize("name", list(lrc.mode_cases()))
def test_find_overlap_mode_is_scipys_mode(name):
    from tobac_flow_amd.utils import find_overlap_mode
    labels, field, index, background = lrc.mode_cases()[name]
    for i in index:
        x = field[labels == i]
        if x.size == 0:
            continue
        want = scipy.stats.mode(x[x != background], keepdims=False)[0] if np.any(x != background) else background
        assert find_overlap_mode(x, background=background) == want
    assert find_overlap_mode(np.array([7, 4, 4, 7, 0])) == 4       # a tie: the smaller value
    assert find_overlap_mode(np.zeros(3, np.int32)) == 0 and find_overlap_mode(np.full(3, 2), background=2) == 2


def test_abi_has_the_entry_points():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 110
    for name in ("tf_label_reduce_workspace_bytes", "tf_label_reduce", "tf_label_order_workspace_bytes", "tf_label_order"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.tf_label_reduce_workspace_bytes(-3, 5) >= 9 * 8
    assert L.tf_label_reduce_workspace_bytes(1, 1 + 2 ** 27) == 0 and L.tf_label_order_workspace_bytes(1, 1 + 2 ** 27, 10, 0) == 0


def test_kernel_bodies_on_the_host(tmp_path):
    """tools/label_reduce_host_check.cpp: the bodies of csrc/label_reduce_kernels.h, and the span form of the raveled run
    walker of csrc/label_runs.h under them, compiled for the CPU and run lane after lane on exactly-sized buffers (its
    first lines give the AddressSanitizer / UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "label_reduce_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "label_reduce_host_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout + out.stderr


PASSES = [f"_Z15k_lreduce_pass{p}I{e}E" for p in (1, 2) for e in "hifd"]


@pytest.fixture(scope="module")
def pass_resources(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    return _resources("label_reduce.hip", str(tmp_path_factory.mktemp("label_reduce_resources")))


@pytest.mark.parametrize("kernel", PASSES)
def test_pass_kernels_keep_8_waves_per_simd(pass_resources, kernel):
    """the project's standing budget for label passes: no scratch, at most 64 registers allocated"""
    k = _one(pass_resources, kernel)
    print(kernel, k, "allocated", _allocated(k))
    assert k["scratch"] == 0
    assert _allocated(k) <= 64
