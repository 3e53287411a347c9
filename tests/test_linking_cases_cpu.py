"""The second stage (tobac_flow_amd/linking.py) without a device: the restatement of tests/linking_cases.py and the
package's functions on NumPy containers against tests/golden/linking_ref.npz, which the reference's own functions wrote
where they can run without xarray (the fixture's `source/...` entries say which).

process_file composes dataset.py's functions, which compute on the device whatever the container; here the four of them
that launch kernels (flag_nan_adjacent_labels, link_cores_and_anvils, add_step_labels, link_step_labels) and the id scan
of add_label_coords are replaced by oracle/np_dataset.py, so that the chain's order, the trim and the cuts to the remaining
labels are checked; tests/test_gpu_linking.py runs the chain as it is."""
import os
import pathlib
import re
from datetime import datetime

import numpy as np
import pytest

import label_glue_cases as gc
import linking_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = lc.chains()


@pytest.fixture(scope="module")
def gold():
    return lc.fixture()


@pytest.fixture(scope="module")
def restated():
    """{case: (overlap results, links)} of the restatement"""
    return {case: lc.np_link_chain(names, store) for case, (names, store) in CHAINS.items()}


def _as_int(a):
    a = np.asarray(a)
    return a.astype("datetime64[ns]").astype(np.int64) if a.dtype.kind == "M" else a


def _check(gold, prefix, arrays):
    """every fixture entry under `prefix` is there and equal, and nothing else is"""
    want = {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}
    assert want and set(want) == set(arrays), (prefix, sorted(set(want) ^ set(arrays)))
    for k, v in want.items():
        got = _as_int(arrays[k])
        assert got.shape == v.shape and np.array_equal(got, v), prefix + k


def _links_dataset(links):
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords=dict(links["coords"]))
    for k, v in links.items():
        if k != "coords":
            ds.add(k, v, ("core",) if k == "core_labels" else ("anvil",) if k == "anvil_labels" else ("filename",))
    return ds


def test_fixture_names_its_sources(gold):
    sources = {k.split("/", 1)[1]: str(v) for k, v in gold.items() if k.startswith("source/")}
    assert set(lc.NEW_FUNCTIONS) <= set(sources)
    for name in ("find_overlaps", "find_overlap_between_cores", "find_overlap_between_anvils", "find_new_labels",
                 "get_dates_from_filename"):
        assert sources[name] == "reference"
    for name in ("process_linking_output", "merge_previous_file", "process_file"):
        assert sources[name] == "restatement"


@pytest.mark.parametrize("case", list(CHAINS))
def test_restatement_equals_the_fixture(gold, restated, case):
    names, store = CHAINS[case]
    results, links = restated[case]
    for i, result in enumerate(results):
        for kind in ("core", "anvil"):
            lo, hi, x, y = result[kind]
            _check(gold, f"{case}/overlap/{i}/{kind}/", {"minmax": np.array([lo, hi]), "x": x, "y": y})
    _check(gold, f"{case}/links", lc.flatten_product("", links))
    for j, name in enumerate(names):
        _check(gold, f"{case}/dates/{j}", {"": np.array([np.datetime64(d, "ns") for d in lc.np_get_dates_from_filename(name)])})
        _check(gold, f"{case}/map/{j}/", {"core": lc.np_get_core_label_map_for_file(name, links),
                                         "anvil": lc.np_get_anvil_label_map_for_file(name, links)})
        for merge, key in ((False, "relabel"), (True, "merge")):
            ds = lc.np_relabel_and_merge_file(name, links, store, merge=merge)
            _check(gold, f"{case}/{key}/{j}/", {n: ds[n] for n, _ in lc.VOLUMES})
    if case in lc.WORLDS:
        processed = [lc.np_process_file(name, links, store) for name in names]
        for j, ds in enumerate(processed):
            _check(gold, f"{case}/process/{j}", lc.flatten_product("", ds))
        lc.np_increment_step_coords(processed[1], processed[0])
        _check(gold, f"{case}/increment/", {k: processed[1]["coords"][k] for k in ("core_step", "thick_anvil_step", "thin_anvil_step")})
        lc.merged_partition_check(case)


def test_find_overlaps_equals_the_reference(gold):
    from tobac_flow_amd import linking
    for name in lc.RULE_CASES:
        left, right, grid = gc.window_cases()[name]
        top = int(right.max())
        counts = np.maximum(np.bincount(right.ravel(), minlength=top + 1), 1)
        for fn in (linking.find_overlaps, lc.np_find_overlaps):
            rows = [(g, int(i), int(m)) for g, (atol, rtol) in enumerate(grid) for i in np.unique(left[left > 0])
                    for m in fn(right[left == i], atol, rtol, top, counts)]
            assert np.array_equal(np.array(rows).reshape(-1, 3), gold[f"find_overlaps/{name}"]), name


@pytest.mark.parametrize("case", list(CHAINS))
def test_package_on_numpy_containers_equals_the_fixture(gold, restated, case):
    from tobac_flow_amd import linking
    names, plain_store = CHAINS[case]
    store = lc.to_store(plain_store)
    results = [linking.find_overlap_between_files(a, b, store) for a, b in zip(names[:-1], names[1:])]
    for i, result in enumerate(results):
        assert (result["filename_1"], result["filename_2"]) == (names[i], names[i + 1]) and set(result) == {"filename_1", "filename_2", "anvil", "core"}
        for kind in ("core", "anvil"):
            lo, hi, x, y = result[kind]
            _check(gold, f"{case}/overlap/{i}/{kind}/", {"minmax": np.array([lo, hi]), "x": x, "y": y})
            ref = restated[case][0][i][kind]
            assert isinstance(lo, int) and isinstance(hi, int) and x.dtype == ref[2].dtype and y.dtype == ref[3].dtype
    links = linking.process_linking_output(results)
    _check(gold, f"{case}/links", lc.product_arrays(links))
    assert links.dims["core_labels"] == ("core",) and links.dims["anvil_start"] == ("filename",)
    assert links["core_start"].dtype == links["anvil_labels"].dtype == np.int32
    for kind in ("core", "anvil"):
        x = np.concatenate([r[kind][2] + s for r, s in zip(results, links[kind + "_start"])])
        y = np.concatenate([r[kind][3] + s for r, s in zip(results, links[kind + "_start"][1:])])
        assert np.array_equal(linking.find_new_labels(x, y, links[kind + "_labels"].size), gold[f"{case}/links/{kind}_labels"])
    for j, name in enumerate(names):
        _check(gold, f"{case}/map/{j}/", {"core": linking.get_core_label_map_for_file(name, links),
                                         "anvil": linking.get_anvil_label_map_for_file(name, links)})
        before = {n: store[name][n].copy() for n, _ in lc.VOLUMES}
        plain = linking.relabel_and_merge_file(name, links, store, merge=False)
        _check(gold, f"{case}/relabel/{j}/", {n: plain[n] for n, _ in lc.VOLUMES})
        merged = linking.relabel_and_merge_file(name, links, store)
        _check(gold, f"{case}/merge/{j}/", {n: merged[n] for n, _ in lc.VOLUMES})
        assert all(merged[n].dtype == np.int32 for n, _ in lc.VOLUMES)
        # the same from the single steps: relabel, then the two merges one after the other
        ds = linking.relabel_cores_and_anvils(lc.to_label_dataset(plain_store[name]), name, links)
        _check(gold, f"{case}/relabel/{j}/", {n: ds[n] for n, _ in lc.VOLUMES})
        ds = linking.merge_next_file(linking.merge_previous_file(ds, name, links, store), name, links, store)
        _check(gold, f"{case}/merge/{j}/", {n: ds[n] for n, _ in lc.VOLUMES})
        assert all(np.array_equal(store[name][n], before[n]) for n in before), "a product of the store was written to"


def test_combine_labels_fills_the_zeros_in_place():
    from tobac_flow_amd import linking
    names, plain_store = CHAINS["tiny"]
    ds, other = lc.to_label_dataset(plain_store[names[0]]), lc.to_label_dataset(lc.cut(plain_store[names[1]], [2, 0]))
    want = {n: ds[n].copy() for n, _ in lc.VOLUMES}
    at = np.searchsorted(ds.coords["t"], other.coords["t"])
    for n in want:
        want[n][at] = np.where(want[n][at] == 0, other[n], want[n][at])
    volumes = {n: ds[n] for n in want}
    assert linking.combine_labels(ds, other) is ds
    assert all(ds[n] is volumes[n] and np.array_equal(ds[n], want[n]) for n in want)
    other.coords["t"] = other.coords["t"] + np.timedelta64(1, "s")
    with pytest.raises(KeyError):
        linking.combine_labels(ds, other)


def test_frame_count_edges(gold):
    from tobac_flow_amd import linking
    for name, pairs in (("common3", True), ("common2", False), ("common1", False), ("common0", False), ("gap", True)):
        names, plain_store = CHAINS[f"time/{name}"]
        store = lc.to_store(plain_store)
        for fn, coord in ((linking.find_overlap_between_cores, "core"), (linking.find_overlap_between_anvils, "anvil")):
            lo, hi, x, y = fn(store[names[0]], store[names[1]])
            assert (lo, hi) == (store[names[0]].coords[coord].max(), store[names[1]].coords[coord].max())
            assert (x.size > 0) == pairs and x.size == y.size and x.dtype == np.int32 and y.dtype == np.int32
    # one common frame: nothing is merged; two: the previous product gives the first, the next one the last
    for name, changed in (("common0", False), ("common1", False), ("common2", True)):
        names, plain_store = CHAINS[f"time/{name}"]
        assert any(not np.array_equal(gold[f"time/{name}/relabel/0/{n}"], gold[f"time/{name}/merge/0/{n}"]) for n, _ in lc.VOLUMES) == changed


def test_relabel_refuses_ids_outside_the_map(restated):
    from tobac_flow_amd import linking
    names, plain_store = CHAINS["tiny"]
    links = _links_dataset(restated["tiny"][1])
    top = linking.get_core_label_map_for_file(names[1], links).size
    for bad in (top + 1, -1):
        ds = lc.to_label_dataset(plain_store[names[1]])
        ds["core_label"][0, 0, 0] = bad
        with pytest.raises(ValueError):
            linking.relabel_cores_and_anvils(ds, names[1], links)
    ds = lc.to_label_dataset(plain_store[names[1]])
    ds["core_label"][0, 0, 0] = top                      # the largest id of the map is accepted
    linking.relabel_cores_and_anvils(ds, names[1], links)
    with pytest.raises(KeyError):
        linking.get_core_label_map_for_file("no such file", links)


def test_store_may_be_a_callable(gold, restated):
    from tobac_flow_amd import linking
    names, plain_store = CHAINS["tiny"]
    store = lc.to_store(plain_store)
    opened = []
    merged = linking.relabel_and_merge_file(names[1], _links_dataset(restated["tiny"][1]), lambda n: opened.append(n) or store[n])
    _check(gold, "tiny/merge/1/", {n: merged[n] for n, _ in lc.VOLUMES})
    assert set(opened) == set(names)


def _host_dataset_functions(monkeypatch):
    """dataset.py's device work replaced by oracle/np_dataset.py (module docstring)"""
    from oracle import np_dataset
    from tobac_flow_amd import dataset

    def adapt(fn, dims_of):
        def call(ds, *args, **kwargs):
            plain = dict(ds)
            plain["coords"] = ds.coords
            fn(plain, *args, **kwargs)
            for k, v in plain.items():
                if k != "coords":
                    ds[k] = v
                    if k in dims_of:
                        ds.dims[k] = dims_of[k]
        return call

    kinds = (("core", "core"), ("thick_anvil", "anvil"), ("thin_anvil", "anvil"))
    monkeypatch.setattr(dataset, "_present_ids", lambda *v: np_dataset._ids(*v))
    monkeypatch.setattr(dataset, "flag_nan_adjacent_labels", adapt(np_dataset.flag_nan_adjacent_labels, {k + "_nan_flag": (d,) for k, d in kinds}))
    monkeypatch.setattr(dataset, "link_cores_and_anvils", adapt(np_dataset.link_cores_and_anvils, {"core_anvil_index": ("core",), "anvil_core_count": ("anvil",)}))
    monkeypatch.setattr(dataset, "add_step_labels", adapt(np_dataset.add_step_labels, {k + "_step_label": ("t", "y", "x") for k, _ in kinds}))
    monkeypatch.setattr(dataset, "link_step_labels", adapt(np_dataset.link_step_labels, {
        "core_step_core_index": ("core_step",), "thick_anvil_step_anvil_index": ("thick_anvil_step",),
        "thin_anvil_step_anvil_index": ("thin_anvil_step",)}))


@pytest.mark.parametrize("world", list(lc.WORLDS))
def test_process_file_chain_on_host_stand_ins(gold, restated, monkeypatch, world):
    from tobac_flow_amd import linking
    _host_dataset_functions(monkeypatch)
    names, plain_store = CHAINS[world]
    store, links = lc.to_store(plain_store), _links_dataset(restated[world][1])
    processed = [linking.process_file(name, links, store) for name in names]
    for j, ds in enumerate(processed):
        _check(gold, f"{world}/process/{j}", lc.product_arrays(ds))
        a, b = lc.OWNED[j]
        assert np.array_equal(ds.coords["t"], lc.times(range(a, b))) and ds["core_label"].shape[0] == b - a
    relabelled = linking.process_file(names[1], links, store, merge=False)
    assert np.array_equal(relabelled["core_label"], gold[f"{world}/relabel/1/core_label"][1:5])
    assert linking.increment_step_coords(processed[1], processed[0]) is processed[1]
    _check(gold, f"{world}/increment/", {k: processed[1].coords[k] for k in ("core_step", "thick_anvil_step", "thin_anvil_step")})


def test_datetime_helpers(gold):
    from tobac_flow_amd.utils import datetime_utils as du
    assert {"get_dates_from_filename", "trim_file_start", "trim_file_end", "trim_file_start_and_end", "get_datetime_from_coord",
            "time_diff", "get_time_diff_from_coord"} == set(du.__all__)
    names, plain_store = CHAINS["tiny"]
    for j, name in enumerate(names):
        for form in (name, pathlib.Path(name)):
            dates = du.get_dates_from_filename(form)
            assert all(type(d) is datetime for d in dates)
            assert np.array_equal(np.array([np.datetime64(d, "ns") for d in dates]).astype(np.int64), gold[f"tiny/dates/{j}"])
    with pytest.raises(ValueError):
        du.get_dates_from_filename(b"bytes")
    ds = lc.to_label_dataset(plain_store[names[1]])                       # frames 4 .. 10, the name claims 5 .. 8
    ds.add("per_frame", np.arange(7), ("t",))
    ds.add("lat", np.zeros((3, 5)), ("y", "x"))
    for fn, frames in ((du.trim_file_start, range(5, 11)), (du.trim_file_end, range(4, 9)), (du.trim_file_start_and_end, range(5, 9))):
        cut = fn(ds, names[1])
        at = np.array(frames) - 4
        assert cut is not ds and np.array_equal(cut.coords["t"], lc.times(frames)) and np.array_equal(cut["per_frame"], at)
        assert np.array_equal(cut["thin_anvil_label"], ds["thin_anvil_label"][at]) and np.shares_memory(cut["core_label"], ds["core_label"])
        assert cut["lat"] is ds["lat"] and cut.dims["per_frame"] == ("t",) and np.array_equal(cut.coords["core"], ds.coords["core"])
    assert ds["core_label"].shape[0] == 7 and ds.coords["t"].size == 7


def test_the_kernel_is_declared_exported_and_versioned():
    import ctypes
    from tobac_flow_amd import _lib, linking
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    declared = set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert "tf_relabel_merge" in declared and "tf_relabel_merge" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "tf_relabel_merge")
    assert _lib.lib().tf_version() >= 111
    assert len(_lib._PROTOS["tf_relabel_merge"][1]) == 18
    assert set(lc.NEW_FUNCTIONS) == set(linking.__all__)
