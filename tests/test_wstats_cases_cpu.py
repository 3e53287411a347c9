"""The yardsticks of the per-label weighted statistics, without a device: the float64 restatement of tests/wstats_cases.py
and the per-region host forms of tobac_flow_amd.utils.stats_utils against the reference's own results in
tests/golden/wstats_ref.npz, the input validation of tobac_flow_amd.postprocess, and the kernel bodies compiled for the
host (tools/wstats_host_check.cpp).

Bounds.  NaN patterns are identical and min, max and the errors at them are equal.  The summed values (mean, std, uncertainty
of the mean, combined error) of the float32 case are held to 4 x the largest relative difference between the reference's
float32 results and the float64 restatement over the committed cases, measured when the fixture was written and stored in
it (1.43e-7: the reference's own float32 summation error; the assertion therefore sits at 5.7e-7, below the project's
rtol 2e-5 for this class); those of the float64 case to rtol 1e-12."""
import os
import shutil
import subprocess
from functools import partial

import numpy as np
import pytest

import wstats_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound(name, meta):
    if name.startswith("A_f32"):
        measured = float(meta["max_rel_f32"])
        assert 0 < 4 * measured < 2e-5
        return 4 * measured
    return 1e-12


def _hold(got, want, rtol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    n = got.shape[1]
    selected = [k for k in wc.SELECTED if k < n]
    summed = [k for k in wc.SUMMED if k < n]
    assert np.array_equal(got[:, selected], want[:, selected], equal_nan=True), what
    ok = ~np.isnan(want[:, summed])
    rel = np.abs(got[:, summed] - want[:, summed])[ok] / np.abs(want[:, summed][ok])
    print(what, "largest relative difference of the summed values:", float(rel.max()), "bound", rtol)
    assert rel.max() <= rtol, (what, float(rel.max()))


@pytest.mark.parametrize("name", wc.CASES)
def test_restatement_matches_the_references_results(name):
    cases, meta = wc.golden()
    c = cases[name]
    rtol = _bound(name, meta)
    _hold(wc.restate_stats(c["labels"], c["x"], c["e"], c["w"], c["index"]), c["stats8"], rtol, name + " stats8")
    _hold(wc.restate_stats(c["labels"], c["x"], None, c["w"], c["index"])[:, :4], c["stats4"], rtol, name + " stats4")
    got = wc.restate_proportions(c["labels"], c["flags"], c["wf"], c["flag_values"], c["index"])
    want = c["proportions"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", wc.CASES)
def test_fixture_holds_the_special_labels(name):
    c = wc.golden()[0][name]
    special = dict(zip(c["special_names"].tolist(), c["special_ids"].tolist()))
    row = {int(i): k for k, i in enumerate(c["index"])}
    s8, top = c["stats8"], int(c["labels"].max())
    assert sorted(int(i) for i in c["index"] if i > top) == [top + 3, top + 9]
    assert np.count_nonzero(c["labels"] == special["absent"]) == 0 and np.count_nonzero(c["labels"] == special["one_voxel"]) == 1
    for what in ("absent", "all_nonfinite", "zero_weight", "nan_weight"):
        assert np.isnan(s8[row[special[what]]]).all(), what
    for i in (top + 3, top + 9):
        assert np.isnan(s8[row[i]]).all()
    for what in ("one_voxel", "one_weighted_voxel"):
        r = s8[row[special[what]]]
        assert np.isnan(r[1]) and np.isnan(r[5]) and not np.isnan(r[[0, 2, 3, 4, 6, 7]]).any(), what
    r = s8[row[special["extreme_at_zero_weight"]]]
    at = np.nonzero(c["labels"] == special["extreme_at_zero_weight"])
    assert r[3] == c["x"][at].max() and np.broadcast_to(c["w"], c["labels"].shape)[at][np.argmax(c["x"][at])] == 0
    r = s8[row[special["nan_error"]]]
    assert np.isnan(r[4]) and np.isnan(r[5]) and not np.isnan(r[[0, 1, 2, 3, 6, 7]]).any()
    x = c["x"]
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert c["flags"].dtype == np.int8 and 5 in c["flags"] and 5 not in c["flag_values"]
    assert 4 in c["flag_values"] and 4 not in c["flags"] and np.isnan(c["wf"]).any()
    assert c["w"].ndim == (3 if name.startswith("A") else 2) and x.dtype == (np.float32 if name.startswith("A") else np.float64)


def _regions(c):
    """(row, raveled indices in ascending order) of every id of the case's index that has voxels"""
    flat = c["labels"].ravel()
    for k, i in enumerate(c["index"]):
        at = np.flatnonzero(flat == i)
        if at.size:
            yield k, at


@pytest.mark.parametrize("name", wc.CASES)
def test_host_forms_match_the_references_results_region_by_region(name):
    from tobac_flow_amd.utils import stats_utils as su
    cases, meta = wc.golden()
    c = cases[name]
    rtol = _bound(name, meta)
    x, e = c["x"].ravel(), c["e"].ravel()
    w = np.broadcast_to(c["w"], c["labels"].shape).ravel()
    wf, flags = np.broadcast_to(c["wf"], c["labels"].shape).ravel(), c["flags"].ravel()
    got8, got4 = np.full(c["stats8"].shape, np.nan), np.full(c["stats4"].shape, np.nan)
    got_p = np.full(c["proportions"].shape, np.nan)
    for k, at in _regions(c):
        got8[k] = su.weighted_stats_and_uncertainties(x[at], e[at], w[at])
        got4[k] = su.weighted_stats(x[at], w[at])
        got_p[k] = su.get_weighted_proportions(flags[at], wf[at], c["flag_values"])
        mean, std = got4[k][:2]
        assert np.array_equal(got8[k][4:], su.weighted_uncertainties(x[at], e[at], w[at], std), equal_nan=True)
        keep = np.isfinite(x[at])
        if not np.isnan(mean):
            both = su.weighted_average_and_std(x[at][keep], w[at][keep])
            assert both[0] == mean and (both[1] == std or (np.isnan(both[1]) and np.isnan(std)))
            assert su.weighted_average_uncertainty(e[at][keep], w[at][keep]) == got8[k][4] or np.isnan(got8[k][4])
    _hold(got8, c["stats8"], rtol, name + " host stats8")
    _hold(got4, c["stats4"], rtol, name + " host stats4")
    np.testing.assert_allclose(got_p, c["proportions"], rtol=1e-12, atol=0, equal_nan=True)


def test_tie_case_has_ties_and_the_restatement_takes_the_smallest_index():
    c = wc.tie_case()
    got = wc.restate_stats(c["labels"], c["x"], c["e"], c["w"], c["index"])
    flat, x, e = c["labels"].ravel(), c["x"].ravel(), c["e"].ravel()
    for k, i in enumerate(c["index"]):
        at = np.flatnonzero(flat == i)
        assert (x[at] == x[at].min()).sum() > 1 and (x[at] == x[at].max()).sum() > 1
        assert got[k, 6] == e[at[x[at] == x[at].min()][0]] and got[k, 7] == e[at[x[at] == x[at].max()][0]]
    two = np.flatnonzero(flat == 2)
    zeros = two[x[two] == 0]
    assert np.signbit(x[zeros]).any() and not np.signbit(x[zeros[0]]) and got[1, 6] == e[zeros[0]]


# ---- input validation of tobac_flow_amd.postprocess: before anything touches a device ----------------------------------
def _small():
    labels = np.zeros((2, 4, 6), np.int32)
    labels[:, 1:3, 1:4] = 1
    labels[1, 3, 4:] = 2
    fields = {"bt": np.full(labels.shape, 250.0, np.float32), "bt_uncertainty": np.ones(labels.shape, np.float32)}
    return labels, fields, np.ones(labels.shape, np.float32)


def test_shape_mismatch_is_a_value_error():
    from tobac_flow_amd import postprocess as pp
    labels, fields, weights = _small()
    with pytest.raises(ValueError, match="same shape"):
        pp.weighted_label_stats(labels, weights[:, :, :5], fields, "bt", [1, 2], "core")
    with pytest.raises(ValueError, match="same shape"):
        pp.weighted_label_stats(labels, weights, {"bt": fields["bt"][:1, :3]}, "bt", [1, 2], "core")
    with pytest.raises(ValueError, match="same shape"):
        pp.get_weighted_proportions_da(np.zeros((2, 4, 5), np.int8), weights, labels, "core", index=[1], flag_values=[0], name="q")


@pytest.mark.parametrize("index", [[0, 1], [2, -1], np.array([1, 0], np.int32)])
def test_an_id_below_one_is_a_value_error(index):
    from tobac_flow_amd import postprocess as pp
    labels, fields, weights = _small()
    with pytest.raises(ValueError, match="id < 1"):
        pp.weighted_label_stats(labels, weights, fields, "bt", index, "core", uncertainty=True)
    with pytest.raises(ValueError, match="id < 1"):
        pp.get_weighted_proportions_da(np.zeros(labels.shape, np.int8), weights, labels, "core", index=index,
                                       flag_values=[0, 1], name="q")


def test_flag_values_and_name_are_required_keywords():
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    labels, _, weights = _small()
    flags = np.zeros(labels.shape, np.int8)
    with pytest.raises(TypeError, match="flag_values"):
        pp.get_weighted_proportions_da(flags, weights, labels, "core", index=[1], name="q")
    with pytest.raises(TypeError, match="name"):
        pp.get_weighted_proportions_da(flags, weights, labels, "core", index=[1], flag_values=[0])
    ds = LabelDataset(coords={"core": np.array([1, 2], np.int32)})
    ds.add("core_label", labels, ("t", "y", "x"))
    with pytest.raises(TypeError, match="name"):
        pp.add_weighted_proportions_to_dataset(ds, flags, weights, "core", flag_values=[0])
    with pytest.raises(TypeError):
        pp.get_weighted_proportions_da(flags, weights, labels, "core", None, [1], [0], "q")      # not positional


def test_more_than_64_flag_values_take_the_host_form_and_equal_the_restatement():
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    c = wc.golden()[0]["B_f64_plane"]
    rng = np.random.default_rng(5)
    flags = rng.integers(0, 80, c["labels"].shape).astype(np.int16)
    values = np.arange(70)[::-1].copy()                           # 70 distinct values, 70 .. 79 are not listed
    want = wc.restate_proportions(c["labels"], flags, c["wf"], values, c["index"])
    got = pp.get_weighted_proportions_da(flags, c["wf"], c["labels"], "anvil", index=c["index"], flag_values=values, name="q")
    assert got.shape == (c["index"].size, 70) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    assert np.nanmax(got.sum(1)) <= 1 + 1e-12
    ds = LabelDataset(coords={"anvil": c["index"]})
    ds.add("anvil_label", c["labels"], ("t", "y", "x"))
    assert pp.add_weighted_proportions_to_dataset(ds, flags, c["wf"], "anvil", flag_values=values, name="q") is ds
    assert ds.dims["anvil_q_proportion"] == ("anvil", "q") and np.array_equal(ds.coords["q"], values)
    np.testing.assert_allclose(ds["anvil_q_proportion"], want, rtol=1e-12, atol=0, equal_nan=True)


def test_operands_that_merely_broadcast_take_the_host_form():
    """a (T, 1, W) weight array is neither a volume nor a plane: evaluated on the host, equal to the restatement"""
    from tobac_flow_amd import postprocess as pp
    c = wc.golden()[0]["A_f32_volume"]
    w = c["w"][:, :1, :].copy()
    want = wc.restate_stats(c["labels"], c["x"], c["e"], w, c["index"])
    fields = {"bt": c["x"], "bt_uncertainty": c["e"]}
    got = pp.weighted_label_stats(c["labels"], w, fields, "bt", c["index"], "anvil", uncertainty=True, dtype=np.float64)
    assert [n for n, _ in got] == ["anvil_bt_" + s for s in pp.STAT_NAMES]
    got = np.stack([v for _, v in got], 1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[:, wc.SELECTED], want[:, wc.SELECTED], equal_nan=True)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)


def test_kernel_bodies_on_the_host_against_plain_loops(tmp_path):
    """tools/wstats_host_check.cpp: the bodies of csrc/wstats_kernels.h, and the raveled run walker of csrc/label_runs.h
    under them, compiled for the CPU and run lane after lane on exactly-sized buffers (its first lines give the
    AddressSanitizer / UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "wstats_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "wstats_host_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout + out.stderr
