"""GPU tests of the third stage.  First tf_group_reduce itself, through its ctypes table, against the restatement of
tests/objects_cases.py on record tables that sit on its edges; then every Python function on device tables against the
fixture (tests/golden/objects_ref.npz) and against the same call on NumPy tables.

Counts, minima, maxima, picks, differences, flags, filter decisions, cut coordinates and gradients are equalities; what
derives from a sum is compared with the restatement's exactly rounded value within the bound stated in objects_cases.py."""
import numpy as np
import pytest

import objects_cases as oc

pytestmark = pytest.mark.gpu


def dev(x, odd_offset=False):
    """a NumPy column as a device tensor (datetimes as int64 ticks); odd_offset: at element 1 of a larger allocation"""
    import torch
    x = np.asarray(x)
    x = x.view(np.int64) if x.dtype.kind in "mM" else x
    if not odd_offset:
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    room = torch.empty(x.size + 1, dtype=torch.from_numpy(x[:0].copy()).dtype, device="cuda")
    room[1:] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return room[1:]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(got, want, what):
    got, want = host(got), np.asarray(want)
    got = got.view(np.int64) if got.dtype.kind in "mM" else got
    want = want.view(np.int64) if want.dtype.kind in "mM" else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), what


def run_ops(table, ops, odd_offset=False):
    """tf_group_reduce over device copies of the table: the ops split over calls of at most 16 -> (values, status)"""
    import torch
    from tobac_flow_amd import _groups, _lib
    ids, coord = dev(table["ids"]), dev(table["coord"])
    cache = {}

    def column(c):
        if c is None:
            return None
        key = id(c)
        if key not in cache:
            cache[key] = dev(c, odd_offset)
        return cache[key]

    dev_ops = [(op[0],) + tuple(column(c) for c in (tuple(op[1:]) + (None, None, None))[:3]) for op in ops]
    outs = [torch.empty(coord.numel(), dtype=torch.int64 if oc.int_result(op[0], op[1] if len(op) > 1 else None) else torch.float64,
                        device="cuda") for op in ops]
    status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    for at in range(0, max(len(ops), 1), _lib.GROUP_MAX_OPS):
        _groups.group_reduce_call(ids, coord, dev_ops[at:at + 16], outs[at:at + 16], status)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], status.cpu().numpy()


@pytest.fixture(scope="module")
def tables():
    return {case: oc.record_table(**kwargs) for case, kwargs in oc.KERNEL_TABLES.items()}


@pytest.fixture(scope="module")
def restated(tables):
    return {case: oc.np_group_reduce(t["ids"], t["coord"], oc.all_ops(t)) for case, t in tables.items()}


@pytest.fixture(scope="module")
def chains():
    return {name: oc.np_chain(oc.world(**kwargs)) for name, kwargs in oc.WORLDS.items()}


def check_against(ops, got, want, what):
    for k, (op, values, (expected, bound)) in enumerate(zip(ops, got, want)):
        assert values.dtype == expected.dtype, (what, k, op[0])
        if bound.any():
            assert oc.close(values, expected, bound) <= 0, (what, k, op[0])
        else:
            same(values, expected, (what, k, op[0]))                # gradients included: bit for bit


@pytest.mark.parametrize("case", list(oc.KERNEL_TABLES))
def test_group_reduce_against_restatement(case, tables, restated):
    """groups of 1, 63, 64, 65, 256, 257 and 4097 records interleaved in record order; dense, sparse int32 (up to 2^31 - 1)
    and int64 ids; float32 and float64 columns; all-NaN and part-NaN groups, infinities, tied extremes, zero weights,
    equal times; 27 operations, hence two calls"""
    ops = oc.all_ops(tables[case])
    got, status = run_ops(tables[case], ops)
    assert status.tolist() == [0, 0]
    check_against(ops, got, restated[case], case)
    if case in oc.FIXTURE_TABLES:
        fx = oc.fixture()
        for k, (values, (_, bound)) in enumerate(zip(got, restated[case])):
            if not bound.any():
                same(values, fx[f"table/{case}/op/{k}"], (case, k))


def test_group_reduce_columns_at_an_odd_element_offset_and_repeatable(tables, restated):
    ops = oc.all_ops(tables["edges_f32_sparse"])
    got, _ = run_ops(tables["edges_f32_sparse"], ops, odd_offset=True)
    check_against(ops, got, restated["edges_f32_sparse"], "odd offset")
    again, _ = run_ops(tables["edges_f32_sparse"], ops)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()                           # the same bits from run to run


def test_group_reduce_status_counts():
    """a record whose id is missing from coord, a coord id without records; N = 0 and G = 0"""
    from tobac_flow_amd.utils import stats_utils
    table = oc.record_table(seed=21, lengths=[3, 1, 4, 2, 5], ids="sparse32")
    ops = oc.all_ops(table)[:16]
    want = oc.np_group_reduce(table["ids"], table["coord"], ops)
    broken = dict(table)
    coord = table["coord"]
    gone = table["ids"] == coord[1]
    broken["ids"] = np.where(gone, coord[1] + 1, table["ids"]).astype(table["ids"].dtype)   # group 1 loses its record to an unknown id
    broken["coord"] = np.concatenate([coord[:3], [coord[3] - 1, coord[3]], coord[4:]]).astype(coord.dtype)   # and an id nobody has
    got, status = run_ops(broken, oc.all_ops(broken)[:16])
    assert status.tolist() == [int(gone.sum()), 2]
    keep = np.array([0, 2, 4, 5])                                   # the groups that are intact keep their values
    for k, (values, (expected, bound)) in enumerate(zip(got, want)):
        picks = np.array([0, 2, 3, 4])
        if bound.any():
            assert oc.close(values[keep], expected[picks], bound[picks]) <= 0, k
        else:
            same(values[keep], expected[picks], k)
    with pytest.raises(ValueError, match="not in coord"):
        stats_utils.counts_groupby(dev(broken["ids"]), broken["coord"])
    with pytest.raises(ValueError, match="without a record"):
        stats_utils.counts_groupby(dev(table["ids"]), np.concatenate([[coord[0] - 1], coord]))

    empty = oc.record_table(seed=1, lengths=[])
    got, status = run_ops(empty, oc.all_ops(empty)[:16])
    assert status.tolist() == [0, 0] and all(v.size == 0 for v in got)
    no_records = dict(empty, coord=np.array([4, 9, 11], np.int32))
    got, status = run_ops(no_records, [("COUNT",), ("SUM", empty["f"]), ("PICK_IDXMIN", empty["f"]), ("GRADIENT_MIN", empty["f"], None, empty["t"])])
    assert status.tolist() == [0, 3]
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0] and got[2].tolist() == [-1, -1, -1] and np.isnan(got[3]).all()
    no_groups = dict(table, coord=np.zeros(0, np.int32))
    got, status = run_ops(no_groups, [("COUNT",)])
    assert status.tolist() == [table["ids"].size, 0]


@pytest.mark.parametrize("case", oc.FIXTURE_TABLES)
def test_groupby_helpers_on_device_tables(case, tables):
    from tobac_flow_amd.utils import stats_utils
    fx = oc.fixture()
    for name in oc.GROUPBY_NAMES:
        want, bound = oc.np_groupby(name, tables[case])
        got = oc.call_groupby(stats_utils, name, tables[case], dev)
        on_host = oc.call_groupby(stats_utils, name, tables[case])
        assert got.is_cuda, name
        recorded = fx[f"groupby/{case}/{name}"]
        if name in oc.EXACT_GROUPBY:
            same(got, recorded, name)
            same(got, on_host, name)
        else:
            by_reference = str(fx[f"source/{name}"]) == "reference"
            assert oc.close(host(got), want, bound) <= 0, name
            assert oc.close(host(got), recorded, (2 if by_reference else 1) * bound) <= 0, name
            assert oc.close(host(got), on_host, 2 * bound) <= 0, name


def check_chain(got, final, fixture_prefix=None):
    fx = oc.fixture()
    assert set(got) == set(final)
    for dim, coord in final.coords.items():
        same(got.coords[dim], coord, dim)
    for name, want in final.items():
        assert got[name].is_cuda, name
        recorded = want if fixture_prefix is None else fx[f"{fixture_prefix}/{name}"]
        if name in final.bounds:
            assert oc.close(host(got[name]), recorded, final.bounds[name]) <= 0, name
        else:
            same(got[name], recorded, name)


@pytest.mark.parametrize("world", list(oc.WORLDS))
def test_chain_on_device_tables(world, chains, monkeypatch):
    """remove_orphan_coords -> filter_cores -> process_core_properties -> filter_anvils -> process_thick / thin
    anvil_properties -> remove_orphan_coords -> add_validity_flags on a LabelDataset of device tensors: every variable
    stays a device tensor, no column goes through the download path, and the result is the fixture's"""
    from tobac_flow_amd import _lib
    fx = oc.fixture()

    def no_download(*a, **k):
        raise AssertionError("a column visited the host")
    monkeypatch.setattr(_lib, "to_host", no_download)
    stages = {}
    got = oc.package_chain(oc.to_label_dataset(oc.world(**oc.WORLDS[world]), dev), stages)
    for stage, table in stages.items():
        for dim, coord in table.coords.items():
            same(coord, fx[f"world/{world}/{stage}/coords/{dim}"], (stage, dim))
    check_chain(got, chains[world], f"world/{world}/final")
    on_host = oc.package_chain(oc.to_label_dataset(oc.world(**oc.WORLDS[world])))
    for name, want in chains[world].items():
        if name in chains[world].bounds:
            assert oc.close(host(got[name]), on_host[name], 2 * chains[world].bounds[name]) <= 0, name
        else:
            same(got[name], on_host[name], name)


def test_chain_on_float32_device_tables():
    kwargs = dict(oc.WORLDS["full"], float_dtype=np.float32)
    final = oc.np_chain(oc.world(**kwargs))
    got = oc.package_chain(oc.to_label_dataset(oc.world(**kwargs), dev))
    assert set(got) == set(final)
    for dim, coord in final.coords.items():
        same(got.coords[dim], coord, dim)
    for name, want in final.items():
        value = host(got[name])
        if name in final.bounds:
            assert oc.close(value, want, final.bounds[name]) <= 0, name
        elif want.dtype == np.float32:
            same(value.astype(np.float32), want, name)             # values picked from a float32 column
        else:
            same(value, want, name)


def test_sel_on_device_tables():
    from tobac_flow_amd.utils import xarray_utils as xu
    fx = oc.fixture()
    base = oc.np_remove_orphan_coords(oc.world())
    ds = oc.to_label_dataset(base, dev)
    cores, anvils = base.coords["core"][[3, 7, 8]], base.coords["anvil"][[1, 4]]
    for got, want in ((xu.sel_core(ds, cores), oc.np_sel_core(base, cores)), (xu.isel_core(ds, [3, 7, 8]), oc.np_isel_core(base, [3, 7, 8])),
                      (xu.sel_anvil(ds, anvils), oc.np_sel_anvil(base, anvils)), (xu.isel_anvil(ds, [1, 4]), oc.np_isel_anvil(base, [1, 4]))):
        for dim, coord in want.coords.items():
            same(got.coords[dim], coord, dim)
        for name, value in want.items():
            assert got[name].is_cuda
            same(got[name], value, name)
    same(xu.sel_core(ds, cores).coords["core_step"], fx["world/full/sel_core/coords/core_step"], "core_step")
    same(xu.sel_anvil(ds, anvils).coords["thin_anvil_step"], fx["world/full/sel_anvil/coords/thin_anvil_step"], "thin_anvil_step")
