"""The validation stage on the GPU (tobac_flow_amd.validation: flash_list, get_edge_filter_dev, the five validate_*
wrappers, validate_detection; ndimage_dev.flash_list / edt_cylinder_at / edge_filter) against np.repeat, the volumes of
edt_cylinder gathered at the list, the host get_edge_filter (SciPy's binary_dilation), and the reference's own five
wrappers in tests/golden/validate_ref.npz.

Everything computed is an integer or one correctly rounded square root of one, so the bound is equality throughout.  The
one freedom is the label reported at a flash where several labels are equally near: there the kernel's scan order is
allowed, and the label must be one of the nearest set found by brute force."""
from types import SimpleNamespace

import numpy as np
import pytest

import validate_cases as cases
import validation_cases as vc

pytestmark = pytest.mark.gpu
M, TM = cases.MARGIN, cases.TIME_MARGIN


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def host(x):
    return x.cpu().numpy()


# ---- the flash list ----------------------------------------------------------------------------------------------------
def _sizes():
    from tobac_flow_amd import ndimage_dev
    tile = ndimage_dev.flash_tile()
    return [1, tile - 1, tile, tile + 1, 3 * tile + 5]


def _patterns(n, tile):
    """{name: float64 counts}: what the fill can meet, for a grid of n voxels"""
    out = {"zero": np.zeros(n), "one": np.ones(n)}
    for big in (65, 1025, 5000):                                  # more flashes in one voxel than a wave, a workgroup, a tile has lanes
        places = {"first": 0, "last": n - 1, "boundary": min(tile, n) - 1, "after": min(tile, n - 1)}
        for where, at in places.items():
            g = np.zeros(n)
            g[at] = big
            out[f"{big}_{where}"] = g
    rng = np.random.default_rng(n)
    out["5000_then_sparse"] = np.where(rng.random(n) < 0.05, 1.0, 0.0)
    out["5000_then_sparse"][0] = 5000
    out["fractions"] = np.where(rng.random(n) < 0.3, 2.9, 0.4)   # 2.9 -> 2, 0.4 -> 0
    out["sparse"] = np.where(rng.random(n) < 0.01, rng.integers(1, 4, n), 0).astype(np.float64)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
@pytest.mark.parametrize("k", range(5))
def test_flash_list_equals_np_repeat(lib, dtype, k):
    from tobac_flow_amd import ndimage_dev
    n, tile = _sizes()[k], ndimage_dev.flash_tile()
    for name, counts in _patterns(n, tile).items():
        grid = counts.astype(dtype)
        want = np.repeat(np.arange(n), grid.astype(int).ravel())
        got = ndimage_dev.flash_list(lib.to_dev(grid))
        assert got.dtype == lib.torch().int64 and got.is_cuda, name
        assert np.array_equal(host(got), want), (name, n, dtype)
        assert np.array_equal(host(ndimage_dev.flash_list(lib.to_dev(grid))), host(got)), name      # two runs, one list
    assert _patterns(n, tile)["zero"].sum() == 0 and ndimage_dev.flash_list(lib.to_dev(np.zeros(n, dtype))).numel() == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_flash_list_refuses_what_np_repeat_refuses(lib, dtype):
    from tobac_flow_amd import ndimage_dev, validation as v
    tile = ndimage_dev.flash_tile()
    bad = [-1] if dtype == np.int32 else [-1, -0.5, np.nan]
    for value in bad:
        for at in (0, tile, 3 * tile + 4):
            grid = np.ones(3 * tile + 5, dtype)
            grid[at] = value
            with pytest.raises(ValueError, match="repeats may not contain negative values"):
                ndimage_dev.flash_list(lib.to_dev(grid))
    volume = np.zeros(cases.SHAPE, dtype)
    volume[2, 3, 4] = -1
    for give in (lambda a: a, lib.to_dev):
        with pytest.raises(ValueError, match="repeats may not contain negative values"):
            v.flash_list(give(volume))
    huge = np.zeros(3 * tile + 5, dtype)
    huge[tile + 1] = 2 ** 31 - 1 if dtype == np.int32 else 2.0 ** 31
    if dtype != np.int32:                                         # int32 cannot hold it; its largest value is a count like any other
        with pytest.raises(ValueError, match="2\\^31 or more"):
            ndimage_dev.flash_list(lib.to_dev(huge))
        huge[0] = -1
        with pytest.raises(ValueError, match="repeats may not contain negative values"):
            ndimage_dev.flash_list(lib.to_dev(huge))
    flashes = v.flash_list(np.abs(volume) * 3)
    assert len(flashes) == flashes.n == 3 and flashes.shape == cases.SHAPE
    assert host(flashes.voxel).tolist() == [np.ravel_multi_index((2, 3, 4), cases.SHAPE)] * 3


# ---- the cylinder at the flashes ---------------------------------------------------------------------------------------
def _flashes_on(shape, seed):
    """a flash grid over a volume: sparse counts 1 .. 3 and one voxel with 70 flashes"""
    rng = np.random.default_rng(seed)
    g = np.where(rng.random(shape) < 0.02, rng.integers(1, 4, shape), 0).astype(np.float32)
    g[shape[0] - 1, shape[1] // 2, shape[2] - 1] = 70
    return g


@pytest.mark.parametrize("name,tm", [("boxes", 0), ("boxes", 2), ("boxes", 7), ("borders", 0), ("borders", 2), ("borders", 4)])
def test_cylinder_at_equals_the_cylinder_volumes_gathered_at_the_list(lib, name, tm):
    from tobac_flow_amd import ndimage_dev
    t = lib.torch()
    markers = lib.to_dev({"boxes": vc.boxes, "borders": vc.borders}[name]())
    assert tm in (0, 2) or tm >= markers.shape[0]
    voxel = ndimage_dev.flash_list(lib.to_dev(_flashes_on(tuple(markers.shape), 7)))
    d2, nearest = ndimage_dev.edt_squared_frames(markers, return_nearest=True)
    dist, src = ndimage_dev.edt_cylinder(d2, nearest, tm)
    want_dist = host(dist.reshape(-1)[voxel])
    at = src.reshape(-1)[voxel]
    want_closest = host(t.where(at < 0, t.zeros_like(at), markers.reshape(-1)[at.clamp(min=0)].to(t.int64)))
    if name == "boxes" and tm == 0:                               # frames 2 and 5 hold no box: +inf and 0
        assert np.isinf(want_dist).any() and (want_closest[np.isinf(want_dist)] == 0).all() and np.isfinite(want_dist).any()
    for margin in (0, 3, 4.5, 1e9):
        got_dist, got_closest, within = ndimage_dev.edt_cylinder_at(d2, nearest, markers, tm, voxel, margin, get_closest=True)
        assert host(got_dist).tobytes() == want_dist.tobytes() and got_dist.dtype == t.float64          # bit for bit
        assert np.array_equal(host(got_closest), want_closest) and got_closest.dtype == t.int64
        assert within.dtype == t.int64 and int(within) == int((want_dist <= margin).sum())
        plain, none, within2 = ndimage_dev.edt_cylinder_at(d2, None, None, tm, voxel, margin)
        assert none is None and host(plain).tobytes() == want_dist.tobytes() and int(within2) == int(within)
    assert 0 < int((want_dist <= 4.5).sum()) < voxel.numel()
    empty = ndimage_dev.edt_cylinder_at(d2, nearest, markers, tm, voxel[:0], 4.0, get_closest=True)
    assert empty[0].numel() == 0 and empty[1].numel() == 0 and int(empty[2]) == 0


# ---- the edge filter ---------------------------------------------------------------------------------------------------
def _edge_grids():
    """{name: grid}: the missing-data cases of the case module and a (3, 33, 300) grid whose rows are longer than a workgroup"""
    grids = dict(cases.missing_cases())
    wide = np.zeros((3, 33, 300), np.float32)
    wide[1, 16, 0], wide[1, 0, 299], wide[2, 20, 150] = -1, -1, -1
    grids["wide"] = wide
    return grids


_HOST_FILTER = {}


def _host_filter(name, grid, times, key, margin, time_margin):
    from tobac_flow_amd import validation as v
    if (name, key, margin, time_margin) not in _HOST_FILTER:
        _HOST_FILTER[name, key, margin, time_margin] = v.get_edge_filter(SimpleNamespace(glm_flashes=grid, t=times), margin, time_margin)
    return _HOST_FILTER[name, key, margin, time_margin]


@pytest.mark.parametrize("margin", cases.EDGE_MARGINS)
@pytest.mark.parametrize("time_margin", [0, 1, 2])
def test_edge_filter_dev_equals_the_host_filter(lib, margin, time_margin):
    from tobac_flow_amd import validation as v
    t = lib.torch()
    for name, grid in _edge_grids().items():
        for gap in (None, 1):
            times = vc.flash_times(grid.shape[0], gap_after=gap)
            want = _host_filter(name, grid, times, gap, margin, time_margin)
            for give in (lambda a: a, lib.to_dev):
                got = v.get_edge_filter_dev({"glm_flashes": give(grid), "t": times}, margin, time_margin)
                assert got.dtype == t.bool and got.is_cuda
                assert np.array_equal(host(got), want), (name, gap, margin, time_margin)
    if time_margin == 1:                                          # the dilation clears something exactly where the structure is not empty
        grids, times = _edge_grids(), vc.flash_times(5)
        plain = _host_filter("absent", grids["absent"], times, None, margin, 1)
        for name in ("interior", "frame"):
            assert (_host_filter(name, grids[name], times, None, margin, 1).sum() < plain.sum()) == (margin != 3), (name, margin)


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int64, np.int16])
def test_edge_filter_dev_takes_every_grid_dtype(lib, dtype):
    from tobac_flow_amd import validation as v
    grid = cases.missing_cases()["interior"]
    times = vc.flash_times(grid.shape[0])
    want = v.get_edge_filter({"glm_flashes": grid, "t": times}, 7, 1)
    got = v.get_edge_filter_dev({"glm_flashes": lib.to_dev(grid.astype(dtype)), "t": times}, 7, 1)
    assert np.array_equal(host(got), want)


def test_edge_filter_dev_equals_the_reference_fixture(lib):
    from tobac_flow_amd import validation as v
    a = vc.golden()["boxes"]
    for grid, times, key in ((a["glm_grid_raw"], a["times"], "edge_filter"), (a["glm_grid_raw"], a["times_gap"], "edge_filter_gap"),
                             (a["glm_grid_missing"], a["times"], "edge_filter_missing")):
        got = v.get_edge_filter_dev({"glm_flashes": lib.to_dev(grid), "t": times}, vc.MARGIN, vc.TIME_MARGIN)
        same(host(got), a[key])


# ---- the five wrappers and the stage -----------------------------------------------------------------------------------
_TIES = {}


def _ties(labels, grid):
    key = labels.tobytes()
    if key not in _TIES:
        _TIES[key] = cases.tie_flashes(labels, grid, TM)
    return _TIES[key]


def _check_dataset(lib, ds, golden, labels_of, grid, device):
    """every variable of the fixture case, by name, dims, dtype and value; `flash_*_index` may differ at tie flashes"""
    dims = dict(entry.split("=") for entry in golden["dims"])
    assert set(ds) == set(dims), set(ds) ^ set(dims)
    for name, want in ((n, golden[n]) for n in dims):
        got = ds[name]
        assert ",".join(ds.dims[name]) == dims[name], name
        if want.ndim:
            assert lib.is_tensor(got) == device, name
            got = host(got) if device else got
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
        if name.startswith("flash_") and name.endswith("_index"):
            ties, sets, values = _ties(labels_of[name[len("flash_"):-len("_index")]], grid)
            assert vc.in_set(got.astype(np.int64), sets, values).all(), name
            assert np.array_equal(got[~ties], want[~ties]), name
        else:
            assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), name


def _as_dataset(lib, product, device):
    from tobac_flow_amd.dataset import LabelDataset
    coords = {k: product[k] for k in ("core", "anvil", "anvil_marker")}
    ds = LabelDataset(coords=coords)
    for name, value in product.items():
        if name.endswith("_label"):
            ds.add(name, lib.to_dev(value) if device else value, ("t", "y", "x"))
    ds.add("core_anvil_index", product["core_anvil_index"], ("core",))
    return ds


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("get_closest", [0, 1])
def test_the_five_wrappers_equal_the_reference(lib, device, get_closest):
    from tobac_flow_amd import validation as v
    from tobac_flow_amd.dataset import LabelDataset
    g = cases.golden()["inputs"]
    give = lib.to_dev if device else (lambda a: a)
    product = cases.product()
    detection = _as_dataset(lib, product, device)
    operands = [give(g["glm_grid"]), give(g["glm_distance"]), give(g["edge_filter"]), g["n_glm_in_margin"], M, TM]
    wrappers = (v.validate_cores, v.validate_cores_with_anvils, v.validate_anvils, v.validate_anvils_with_cores, v.validate_anvil_markers)
    separate, shared = LabelDataset(), LabelDataset()
    flashes = v.flash_list(operands[0])
    for wrapper in wrappers:
        wrapper(detection, separate, *operands, get_closest=bool(get_closest))
        wrapper(detection, shared, *operands, get_closest=bool(get_closest), flashes=flashes)
    labels_of = {name: labels for name, (labels, _) in cases.restate_subsets(product).items()}
    _check_dataset(lib, separate, cases.golden()[f"wrappers{get_closest}"], labels_of, g["glm_grid"], device)
    plain = lambda x: host(x) if lib.is_tensor(x) else np.asarray(x)             # noqa: E731
    for name in separate:                                                         # one shared list or five: the same dataset
        a, b = plain(separate[name]), plain(shared[name])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f") and separate.dims[name] == shared.dims[name]
    same(separate.coords["core_with_anvil"], product["core"][product["core_anvil_index"] != 0])
    same(separate.coords["anvil_with_core"], np.array([1, 2, 3, 4], np.int32))
    # a plain mapping with the coordinates beside the variables serves as well
    mapping = LabelDataset()
    v.validate_anvils_with_cores({k: (give(x) if k.endswith("_label") else x) for k, x in product.items()}, mapping, *operands)
    same(plain(mapping["anvil_with_core_glm_distance"]), plain(separate["anvil_with_core_glm_distance"]))


def test_validate_markers_with_a_shared_list_equals_the_reference(lib):
    from tobac_flow_amd import validation as v
    g, product = cases.golden(), cases.product()
    i = g["inputs"]
    flashes = v.flash_list(i["glm_grid"])
    for get_closest in (0, 1):
        got = v.validate_markers(product["anvil_marker_label"], i["glm_grid"], i["glm_distance"], i["edge_filter"], i["n_glm_in_margin"],
                                 coord=product["anvil_marker"], margin=M, time_margin=TM, get_closest=bool(get_closest), flashes=flashes)
        want = g[f"markers{get_closest}"]
        for k, name in enumerate(("flash_distance", "flash_closest", "marker_distance", "pod", "far", "n_marker_in_margin", "margin_flag")):
            if got[k] is None:
                assert name not in want
            else:
                same(got[k], want[name])


def test_a_label_above_the_coordinate_is_refused(lib):
    from tobac_flow_amd import validation as v
    from tobac_flow_amd.dataset import LabelDataset
    g, product = cases.golden()["inputs"], cases.product()
    product["core_label"] = product["core_label"].copy()
    product["core_label"][0, 0, 0] = 9
    with pytest.raises(ValueError, match="above the largest id"):
        v.validate_cores_with_anvils(product, LabelDataset(), g["glm_grid"], g["glm_distance"], g["edge_filter"], g["n_glm_in_margin"], M, TM)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("get_closest", [0, 1])
def test_validate_detection_equals_the_reference_and_leaves_its_grid_alone(lib, device, get_closest):
    from tobac_flow_amd import validation as v
    product = cases.product()
    raw = cases.flash_grid()
    grid = lib.to_dev(raw) if device else raw.copy()
    detection = _as_dataset(lib, product, device)
    ds = v.validate_detection(detection, {"glm_flashes": grid, "t": cases.flash_times()}, M, TM, get_closest=bool(get_closest))
    same(host(grid) if device else grid, raw)                                     # the script zeroes its argument; this does not
    same(detection.coords["core"], product["core"])
    labels_of = {name: labels for name, (labels, _) in cases.restate_subsets(cases.cut_to_present(product)).items()}
    _check_dataset(lib, ds, cases.golden()[f"stage{get_closest}"], labels_of, cases.golden()["inputs"]["glm_grid"], device)
    # without the anvil markers' coordinate that set is left out
    del detection.coords["anvil_marker"]
    fewer = v.validate_detection(detection, {"glm_flashes": grid, "t": cases.flash_times()}, M, TM)
    assert not any("anvil_marker" in name for name in fewer) and "anvil_pod" in fewer


def test_validate_detection_trims_the_product_by_its_file_name(lib):
    """`filename=` cuts the padding frames of the product (here the last one); the flash grid is the caller's, already on
    the trimmed frames.  The result equals the stage on a product sliced by hand."""
    from tobac_flow_amd import validation as v
    product, times = cases.product(), cases.flash_times()
    detection = _as_dataset(lib, product, True)
    detection.coords["t"] = times
    name = "detected_dccs_G16_S20180619_170000_E20180619_172500_X0000_0070_Y0000_0037.nc"      # 17:00 .. 17:24:59: frames 0 .. 4
    flash_ds = {"glm_flashes": lib.to_dev(cases.flash_grid()[:5]), "t": times[:5]}
    got = v.validate_detection(detection, flash_ds, M, TM, get_closest=True, filename=name)
    sliced = _as_dataset(lib, {k: (x[:5] if k.endswith("_label") else x) for k, x in product.items()}, True)
    want = v.validate_detection(sliced, flash_ds, M, TM, get_closest=True)
    assert set(got) == set(want) and got["core_glm_distance"].shape[0] == 7 and detection["core_label"].shape[0] == 6
    for key in want:
        a, b = (host(x) if lib.is_tensor(x) else x for x in (got[key], want[key]))
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f") and got.dims[key] == want.dims[key], key
    assert want["flash_count_in_margin"] < cases.golden()["stage1"]["flash_count_in_margin"]    # frame 4 is an end frame now
    with pytest.raises(ValueError, match="same shape"):           # a grid that was not gridded onto the trimmed product
        v.validate_detection(detection, {"glm_flashes": lib.to_dev(cases.flash_grid()), "t": times}, M, TM, filename=name)
