"""CPU tests of the third stage: the restatement of tests/objects_cases.py against the reference-written fixture
(tests/golden/objects_ref.npz), the package's NumPy path against both, the exported names, and the argument checks that
must fire before the library is touched."""
import os
import re

import numpy as np
import pytest

import objects_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    got = got.view(np.int64) if got.dtype.kind in "mM" else got
    want = want.view(np.int64) if want.dtype.kind in "mM" else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), what


@pytest.fixture(scope="module")
def tables():
    return {case: oc.record_table(**oc.KERNEL_TABLES[case]) for case in oc.FIXTURE_TABLES}


@pytest.fixture(scope="module")
def restated(tables):
    return {case: oc.np_group_reduce(t["ids"], t["coord"], oc.all_ops(t)) for case, t in tables.items()}


@pytest.fixture(scope="module")
def chains():
    out = {}
    for name, kwargs in oc.WORLDS.items():
        stages = {}
        out[name] = (oc.np_chain(oc.world(**kwargs), stages), stages)
    return out


def test_fixture_records_its_sources():
    fx = oc.fixture()
    for name in oc.STATS_NAMES + oc.FILTER_NAMES + oc.SEL_NAMES + oc.PROCESS_NAMES:
        assert str(fx[f"source/{name}"]) in ("reference", "restatement"), name
    assert str(fx["source/combined_std_groupby"]) == "reference"


@pytest.mark.parametrize("case", oc.FIXTURE_TABLES)
def test_restatement_equals_fixture_on_tables(case, restated):
    fx = oc.fixture()
    for k, (values, _) in enumerate(restated[case]):
        _same(values, fx[f"table/{case}/op/{k}"], f"{case} op {k}")


@pytest.mark.parametrize("case", oc.FIXTURE_TABLES)
def test_numpy_path_matches_restatement_on_tables(case, tables, restated):
    from tobac_flow_amd import _groups
    table = tables[case]
    ops = oc.all_ops(table)
    got = _groups.reduce_groups(table["ids"], table["coord"], ops)
    assert len(ops) > 16
    for k, (op, values, (want, bound)) in enumerate(zip(ops, got, restated[case])):
        assert values.dtype == want.dtype, (op[0], values.dtype)
        if bound.any():
            assert oc.close(values, want, bound) <= 0, (case, k, op[0])
        else:
            _same(values, want, (case, k, op[0]))


@pytest.mark.parametrize("case", oc.FIXTURE_TABLES)
@pytest.mark.parametrize("name", oc.GROUPBY_NAMES)
def test_groupby_helpers_numpy_path(case, name, tables):
    """package against the fixture: equalities where no sum is involved; where the reference wrote the value, both sides
    are accumulated sums within the bound of the exactly rounded one, hence within twice the bound of each other"""
    from tobac_flow_amd.utils import stats_utils
    fx = oc.fixture()
    want, bound = oc.np_groupby(name, tables[case])
    recorded = fx[f"groupby/{case}/{name}"]
    got = oc.call_groupby(stats_utils, name, tables[case])
    if name in oc.EXACT_GROUPBY:
        _same(want, recorded, name)
        _same(got, recorded, name)
        return
    by_reference = str(fx[f"source/{name}"]) == "reference"
    assert oc.close(recorded, want, bound) <= 0
    assert oc.close(got, want, bound) <= 0
    assert oc.close(got, recorded, (2 if by_reference else 1) * bound) <= 0


def test_calc_combined_forms_match_the_reference_values(tables):
    from tobac_flow_amd.utils import stats_utils
    fx = oc.fixture()
    table = tables["many_int64"]
    wide = {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in table.items()}
    found = oc.members(table["ids"], table["coord"])
    _, bound_mean = oc.np_groupby("combined_mean_groupby", table)
    _, bound_std = oc.np_groupby("combined_std_groupby", table)
    mean = np.array([stats_utils.calc_combined_mean(wide["m"][m], wide["w"][m]) for m in found])
    std = np.array([stats_utils.calc_combined_std(wide["s"][m], wide["m"][m], wide["w"][m]) for m in found])
    assert oc.close(mean, fx["groupby/many_int64/combined_mean_groupby"], 2 * bound_mean) <= 0
    assert oc.close(std, fx["groupby/many_int64/combined_std_groupby"], 2 * bound_std) <= 0


@pytest.mark.parametrize("world", list(oc.WORLDS))
def test_restated_chain_equals_fixture(world, chains):
    fx = oc.fixture()
    final, stages = chains[world]
    for stage, table in stages.items():
        for dim, coord in table.coords.items():
            _same(coord, fx[f"world/{world}/{stage}/coords/{dim}"], (stage, dim))
    names = {k.split("/")[-1] for k in fx if k.startswith(f"world/{world}/final/")}
    assert names == set(final)
    for name, value in final.items():
        _same(value, fx[f"world/{world}/final/{name}"], name)


@pytest.mark.parametrize("world", list(oc.WORLDS))
def test_package_chain_on_numpy_tables(world, chains):
    """linked_statistics_goes.py:260-276 with the package's names on NumPy columns: cut coordinates, decisions, picks, times
    and flags equal the fixture; what derives from a sum lies within the restatement's bound"""
    fx = oc.fixture()
    final, _ = chains[world]
    stages = {}
    got = oc.package_chain(oc.to_label_dataset(oc.world(**oc.WORLDS[world])), stages)
    for stage, table in stages.items():
        for dim, coord in table.coords.items():
            _same(coord, fx[f"world/{world}/{stage}/coords/{dim}"], (stage, dim))
    assert set(got) == set(final)
    for name, want in final.items():
        assert got.dims[name] == final.dims[name], name
        if name in final.bounds:
            assert oc.close(got[name], fx[f"world/{world}/final/{name}"], final.bounds[name]) <= 0, name
        else:
            _same(got[name], fx[f"world/{world}/final/{name}"], name)
    if world == "full":
        assert "thick_anvil_max_cth_corrected_t" not in got and "thick_anvil_min_ctt_corrected_t" in got   # postprocess.py:808
        assert "core_propagation_speed" not in got


def test_sel_and_isel():
    from tobac_flow_amd.utils import xarray_utils as xu
    fx = oc.fixture()
    base = oc.np_remove_orphan_coords(oc.world())
    ds = oc.to_label_dataset(base)
    cores, anvils = base.coords["core"][[3, 7, 8]], base.coords["anvil"][[1, 4]]
    for got, want in ((xu.sel_core(ds, cores), oc.np_sel_core(base, cores)), (xu.isel_core(ds, [3, 7, 8]), oc.np_isel_core(base, [3, 7, 8])),
                      (xu.sel_anvil(ds, anvils), oc.np_sel_anvil(base, anvils)), (xu.isel_anvil(ds, [1, 4]), oc.np_isel_anvil(base, [1, 4]))):
        assert set(got) == set(want)
        for dim, coord in want.coords.items():
            _same(got.coords[dim], coord, dim)
        for name, value in want.items():
            _same(got[name], value, name)
    for dim in ("core", "core_step"):
        _same(xu.sel_core(ds, cores).coords[dim], fx[f"world/full/sel_core/coords/{dim}"], dim)
    for dim in ("anvil", "thick_anvil_step", "thin_anvil_step"):
        _same(xu.sel_anvil(ds, anvils).coords[dim], fx[f"world/full/sel_anvil/coords/{dim}"], dim)
    with pytest.raises(KeyError):
        xu.sel_core(ds, [4])


def test_propagation_with_a_geodesic_inverse():
    """geod_inv given: direction and speed per core on the host, after get_mean_object_azimuth_and_speed; a flat-earth
    stand-in for pyproj.Geod.inv is enough to pin the plumbing (sorting by time, finite mask, circular mean)"""
    from scipy.stats import circmean
    from tobac_flow_amd import postprocess

    def flat_inv(lon1, lat1, lon2, lat2):
        dx, dy = (np.asarray(lon2) - lon1) * 111e3, (np.asarray(lat2) - lat1) * 111e3
        return np.degrees(np.arctan2(dx, dy)), None, np.hypot(dx, dy)

    base = oc.np_filter_cores(oc.np_remove_orphan_coords(oc.world()))
    got = postprocess.process_core_properties(oc.to_label_dataset(base), geod_inv=flat_inv)
    for k, members in enumerate(oc.members(base["core_step_core_index"], base.coords["core"])):
        t = base["core_step_t"][members].view(np.int64)
        order = np.argsort(t)
        az, _, dist = flat_inv(base["core_step_lon"][members][order][:-1], base["core_step_lat"][members][order][:-1],
                               base["core_step_lon"][members][order][1:], base["core_step_lat"][members][order][1:])
        speed = dist / (np.diff(t[order]) / 1e9)
        assert got["core_propagation_direction"][k] == circmean(az, high=180, low=-180)
        assert got["core_propagation_speed"][k] == np.mean(speed)


def test_names_are_exported():
    from tobac_flow_amd import postprocess, utils
    from tobac_flow_amd.utils import filter_utils, stats_utils, xarray_utils
    assert set(oc.STATS_NAMES) <= set(stats_utils.__all__) and set(oc.STATS_NAMES) <= set(utils.__all__)
    assert set(oc.FILTER_NAMES) == set(filter_utils.__all__)
    assert set(oc.SEL_NAMES) <= set(xarray_utils.__all__) and set(oc.SEL_NAMES) <= set(utils.__all__)
    assert set(oc.PROCESS_NAMES) <= set(postprocess.__all__)


def test_kernel_is_declared_and_exported():
    from tobac_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("tf_group_reduce", "tf_group_reduce_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS
    L = _lib.lib()
    assert L.tf_version() >= 113
    assert tuple(_lib.GROUP_OPS) == oc.OPS
    for name, code in _lib.GROUP_OPS.items():
        assert re.search(rf"#define TF_GROUP_{name} {code}\b", header), name
    assert L.tf_group_reduce_workspace_bytes(2 ** 31, 1) == 0 and L.tf_group_reduce_workspace_bytes(10, 3) > 0


def test_bad_inputs_raise_before_the_library(monkeypatch):
    from tobac_flow_amd import _groups, _lib
    from tobac_flow_amd.utils import stats_utils

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    ids, coord, f = np.array([1, 2, 2]), np.array([1, 2]), np.array([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="sorted"):
        stats_utils.counts_groupby(ids, coord[::-1])
    with pytest.raises(ValueError, match="sorted"):
        stats_utils.counts_groupby(ids, np.array([1, 1, 2]))
    with pytest.raises(ValueError, match="shape"):
        stats_utils.weighted_average_groupby(f[:2], f, ids, coord)
    with pytest.raises(ValueError, match="1-D"):
        stats_utils.counts_groupby(ids.reshape(3, 1), coord)
    with pytest.raises(ValueError, match="integer"):
        stats_utils.counts_groupby(f, coord)
    with pytest.raises(TypeError):
        stats_utils.weighted_average_groupby(np.array(["a", "b", "c"]), f, ids, coord)
    with pytest.raises(ValueError, match="unknown"):
        _groups.reduce_groups(ids, coord, [("MEDIAN", f)])
    with pytest.raises(ValueError, match="column"):
        _groups.reduce_groups(ids, coord, [("WEIGHTED_AVERAGE", f)])
    with pytest.raises(ValueError, match="not in coord"):
        stats_utils.counts_groupby(np.array([1, 2, 5]), coord)
    with pytest.raises(ValueError, match="without a record"):
        stats_utils.counts_groupby(ids, np.array([1, 2, 3]))
    assert stats_utils.counts_groupby(np.zeros(0, np.int64), np.zeros(0, np.int64)).size == 0
