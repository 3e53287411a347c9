"""tobac_flow_amd.postprocess (tf_label_wstats, tf_label_proportions) against the float64 restatement of
tests/wstats_cases.py, which test_wstats_cases_cpu.py holds against the reference's own results.

Bounds.  NaN patterns, min, max and the errors at them are exact.  The summed values (mean, std, uncertainty of the mean,
combined error) are held to rtol 1e-9 for float32 and float64 fields alike: the kernel sums in double, its sums have
N <= 10^4 terms of one sign (the fixture's fields, errors and weights are positive), so they are off by at most
N * 2^-53 ~ 1e-12 relative, and the cancelling sum of w (x - mean)^2 is taken about the finished mean on both sides; 1e-9
is a margin of 1000 over that.  Proportions are held to rtol 1e-12 (sums of at most 1 500 non-negative float32 weights in
double)."""
import functools

import numpy as np
import pytest

import wstats_cases as wc

pytestmark = pytest.mark.gpu

RTOL = 1e-9
LAYOUTS = ("volume", "plane")


@functools.lru_cache(maxsize=None)
def _variant(name, dtype, layout):
    """a fixture case with its operands as `dtype` and its weights in `layout`, and the restatement's results for it
    (computed once, shared, not written to)"""
    c = wc.with_dtype(wc.golden()[0][name], np.dtype(dtype))
    w = c["w"]
    if layout == "plane" and w.ndim == 3:
        w = w[0].copy()
    if layout == "volume" and w.ndim == 2:
        w = np.repeat(w[None], c["labels"].shape[0], 0)
    c = dict(c, w=w, wf=w.astype(np.float32))
    want8 = wc.restate_stats(c["labels"], c["x"], c["e"], c["w"], c["index"])
    want_p = wc.restate_proportions(c["labels"], c["flags"], c["wf"], c["flag_values"], c["index"])
    return c, want8, want_p


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _hold(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    n = got.shape[1]
    selected, summed = [k for k in wc.SELECTED if k < n], [k for k in wc.SUMMED if k < n]
    assert np.array_equal(got[:, selected], want[:, selected], equal_nan=True), what
    ok = ~np.isnan(want[:, summed])
    rel = np.abs(got[:, summed] - want[:, summed])[ok] / np.abs(want[:, summed][ok])
    print(what, "largest relative difference of the summed values:", float(rel.max()), "bound", RTOL)
    assert rel.max() <= RTOL, (what, float(rel.max()))


def _columns(results):
    return np.stack([np.asarray(v, np.float64) for _, v in results], 1)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", wc.CASES)
def test_statistics_match_the_restatement(name, dtype, layout, device):
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    c, want8, _ = _variant(name, dtype, layout)
    put = _dev if device else (lambda a: a)
    labels = put(c["labels"].copy())
    before = labels.clone() if device else labels.copy()
    fields = LabelDataset({"bt": put(c["x"]), "bt_uncertainty": put(c["e"])})
    weights = put(c["w"])
    ds = LabelDataset(coords={"anvil": c["index"]})
    ds.add("thick_anvil_label", labels, ("t", "y", "x"))
    assert pp.add_weighted_stats_to_dataset(ds, fields, weights, "bt", "anvil", dim_name="thick_anvil") is ds
    names = ["thick_anvil_bt_" + s for s in pp.STAT_NAMES]
    assert [n for n in ds if n != "thick_anvil_label"] == names
    for k, n in enumerate(names):
        assert ds.dims[n] == ("anvil",) and ds[n].dtype == np.dtype(dtype) and ds[n].shape == (c["index"].size,), n
        assert np.array_equal(np.isnan(ds[n]), np.isnan(want8[:, k])), n
        if k in wc.SELECTED:                                      # values of the field's own type: the cast keeps them
            assert np.array_equal(ds[n], want8[:, k].astype(dtype), equal_nan=True), n
    got = pp.weighted_label_stats(labels, weights, fields, "bt", c["index"], "anvil", dtype=np.float64, uncertainty=True)
    assert [n for n, _ in got] == ["anvil_bt_" + s for s in pp.STAT_NAMES]
    _hold(_columns(got), want8, f"{name} {dtype} {layout}")
    assert bool((labels == before).all())                         # the label volume is only read


@pytest.mark.parametrize("name", wc.CASES)
def test_without_uncertainty_four_results_and_the_error_field_is_not_read(name):
    from tobac_flow_amd import postprocess as pp

    class NoErrors(dict):
        def __getitem__(self, key):
            assert not key.endswith("_uncertainty"), "the uncertainty field was read"
            return dict.__getitem__(self, key)

    c, want8, _ = _variant(name, "float32", "volume")
    fields = NoErrors({"bt": c["x"], "bt_uncertainty": c["e"]})
    got = pp.weighted_label_stats(c["labels"], c["w"], fields, "bt", c["index"], "core", dtype=np.float64)
    assert [n for n, _ in got] == ["core_bt_mean", "core_bt_std", "core_bt_min", "core_bt_max"]
    _hold(_columns(got), want8[:, :4], name + " without uncertainty")
    # and a dataset without the error field gets four variables
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords={"core": c["index"]})
    ds.add("core_label", c["labels"], ("t", "y", "x"))
    pp.add_weighted_stats_to_dataset(ds, {"bt": c["x"]}, c["w"], "bt", "core")
    assert sorted(ds) == sorted(["core_label", "core_bt_mean", "core_bt_std", "core_bt_min", "core_bt_max"])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_tied_extremes_give_the_error_at_the_smallest_index(dtype):
    from tobac_flow_amd import postprocess as pp
    c = wc.with_dtype(wc.tie_case(), np.dtype(dtype))
    want = wc.restate_stats(c["labels"], c["x"], c["e"], c["w"], c["index"])
    fields = {"bt": c["x"], "bt_uncertainty": c["e"]}
    for weights in (c["w"], c["w"][0]):                           # 9 x 23 = 207 pixels: a plane that no lane's four voxels fit
        want = wc.restate_stats(c["labels"], c["x"], c["e"], weights, c["index"])
        got = _columns(pp.weighted_label_stats(c["labels"], weights, fields, "bt", c["index"], "core", uncertainty=True,
                                               dtype=np.float64))
        _hold(got, want, f"tie case {dtype} weights {weights.shape}")
    flat, x, e = c["labels"].ravel(), c["x"].ravel(), c["e"].ravel()
    for k, i in enumerate(c["index"]):
        at = np.flatnonzero(flat == i)
        assert got[k, 6] == e[at[x[at] == x[at].min()][0]] and got[k, 7] == e[at[x[at] == x[at].max()][0]]


def test_index_order_absent_ids_and_a_short_index():
    """ids in any order; an id beyond the largest label or absent from the volume is NaN; an index that stops below the
    largest label is served from fewer records"""
    from tobac_flow_amd import postprocess as pp
    c, want8, _ = _variant("A_f32_volume", "float32", "volume")
    fields = {"bt": c["x"], "bt_uncertainty": c["e"]}
    order = np.argsort(c["index"])[::-1]
    got = _columns(pp.weighted_label_stats(c["labels"], c["w"], fields, "bt", c["index"][order], "core", uncertainty=True,
                                           dtype=np.float64))
    _hold(got, want8[order], "reversed index")
    short = np.array([2, 1, 5], np.int32)
    rows = [int(np.flatnonzero(c["index"] == i)[0]) for i in short]
    got = _columns(pp.weighted_label_stats(c["labels"], c["w"], fields, "bt", short, "core", uncertainty=True, dtype=np.float64))
    _hold(got, want8[rows], "short index")
    got = pp.weighted_label_stats(c["labels"], c["w"], fields, "bt", np.zeros(0, np.int32), "core")
    assert len(got) == 4 and all(v.shape == (0,) and v.dtype == np.float32 for _, v in got)
    empty = np.zeros_like(c["labels"])
    got = _columns(pp.weighted_label_stats(empty, c["w"], fields, "bt", [1, 2], "core", uncertainty=True))
    assert got.shape == (2, 8) and np.isnan(got).all()


def test_a_nan_weight_reaches_the_weight_sum():
    """the record itself: n counts the finite values, the weight sum is NaN for the label with one NaN weight and for no other"""
    import torch
    from tobac_flow_amd import _lib
    c, _, _ = _variant("A_f32_volume", "float32", "volume")
    special = dict(zip(c["special_names"].tolist(), c["special_ids"].tolist()))
    L = _lib.lib()
    lab, x, w = _dev(c["labels"]), _dev(c["x"]), _dev(c["w"])
    n_labels = int(c["labels"].max())
    out = torch.empty((n_labels, 10), dtype=torch.float64, device="cuda")
    ws = torch.empty(L.tf_label_wstats_workspace_bytes(n_labels), dtype=torch.uint8, device="cuda")
    T, hw = lab.shape[0], lab.shape[1] * lab.shape[2]
    _lib.check(L.tf_label_wstats(_lib.ptr(lab), _lib.ptr(x), None, _lib.ptr(w), _lib.TF_F32, T, hw, 0, n_labels,
                                 _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_wstats")
    o = out.cpu().numpy()
    finite = np.isfinite(c["x"])
    assert np.array_equal(o[:, 0], np.bincount(c["labels"][finite & (c["labels"] > 0)], minlength=n_labels + 1)[1:])
    assert np.array_equal(np.flatnonzero(np.isnan(o[:, 1])) + 1, [special["nan_weight"]])
    assert np.isnan(o[special["nan_weight"] - 1, 2:]).all() and np.isnan(o[:, 6:]).all()
    assert o[special["zero_weight"] - 1, 1] == 0 and o[special["zero_weight"] - 1, 0] > 0
    # a workspace that is too small is reported, not overrun
    with pytest.raises(MemoryError):
        _lib.check(L.tf_label_wstats(_lib.ptr(lab), _lib.ptr(x), None, _lib.ptr(w), _lib.TF_F32, T, hw, 0, n_labels,
                                     _lib.ptr(out), _lib.ptr(ws), 64, _lib.stream_ptr()), "tf_label_wstats")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", wc.CASES)
def test_proportions_match_the_restatement(name, layout, device):
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    c, _, want = _variant(name, "float32", layout)
    put = _dev if device else (lambda a: a)
    labels = put(c["labels"].copy())
    before = labels.clone() if device else labels.copy()
    ds = LabelDataset(coords={"anvil": c["index"]})
    ds.add("anvil_label", labels, ("t", "y", "x"))
    out = pp.add_weighted_proportions_to_dataset(ds, put(c["flags"]), put(c["wf"]), "anvil", flag_values=c["flag_values"],
                                                 name="qcflag")
    assert out is ds and ds.dims["anvil_qcflag_proportion"] == ("anvil", "qcflag")
    assert np.array_equal(ds.coords["qcflag"], c["flag_values"])
    got = ds["anvil_qcflag_proportion"]
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    rows = got[~np.isnan(got).any(1)]
    # each share is a rounded quotient: their sum can pass 1 by the roundings of K = 4 terms, no more
    assert rows.size and rows.sum(1).max() <= 1 + 4 * np.finfo(np.float64).eps
    assert (rows[:, list(c["flag_values"]).index(4)] == 0).all() and (rows.sum(1) < 0.999).any()   # never occurs / 5 is not listed
    assert bool((labels == before).all())


def test_flag_types_duplicate_values_and_a_leading_one_on_the_weights():
    from tobac_flow_amd import postprocess as pp
    c, _, _ = _variant("B_f64_plane", "float32", "plane")
    values = [2, 0, 2, 7, 1]                                      # a duplicate, any order, one that never occurs
    want = wc.restate_proportions(c["labels"], c["flags"], c["wf"], values, c["index"])
    call = functools.partial(pp.get_weighted_proportions_da, labels=c["labels"], dim="anvil", index=c["index"],
                             flag_values=values, name="q")
    for flags in (c["flags"], c["flags"].astype(np.int64), c["flags"].astype(np.float32), c["flags"].astype(np.uint8)):
        np.testing.assert_allclose(call(flags, c["wf"][None]), want, rtol=1e-12, atol=0, equal_nan=True)
    mask = c["flags"] == 1
    want = wc.restate_proportions(c["labels"], mask, c["wf"], [True, False], c["index"])
    got = pp.get_weighted_proportions_da(mask, c["wf"], c["labels"], "anvil", index=c["index"], flag_values=[True, False], name="q")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    # default index: 1 .. labels.max()
    got = pp.get_weighted_proportions_da(c["flags"], c["wf"], c["labels"], "anvil", flag_values=[0, 1], name="q")
    ids = np.arange(1, int(c["labels"].max()) + 1)
    np.testing.assert_allclose(got, wc.restate_proportions(c["labels"], c["flags"], c["wf"], [0, 1], ids), rtol=1e-12, atol=0,
                               equal_nan=True)
    # float flags that are not all integral go to the host form and match no listed value there
    odd = c["flags"].astype(np.float64) + 0.5 * (c["flags"] == 5)
    np.testing.assert_allclose(call(odd, c["wf"]), wc.restate_proportions(c["labels"], odd, c["wf"], values, c["index"]),
                               rtol=1e-12, atol=0, equal_nan=True)
