"""subsegment_labels on the GPU (tobac_flow_amd.label.subsegment_labels, tf_subseg_prepare, tf_subseg_rank, Flow.label with
subsegment_shrink != 0) under the contract of tests/subsegment_cases.py: equal to the NumPy restatement on EVERY case (both
select peaks with the same host code), equal to the reference's own result (tests/golden/subsegment_ref.npz) on every case
without a peak-selection tie; the prepare pass equals numpy bit for bit; the flow-linked labels equal the reference's
flow_label."""
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

import subsegment_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def host(x):
    return x.cpu().numpy()


@pytest.mark.parametrize("volume", sc.VOLUMES)
def test_subsegment_labels_equals_the_restatement_everywhere_and_the_reference_without_ties(lib, volume):
    from tobac_flow_amd.label import subsegment_labels
    mask = sc.masks(volume)
    mask_dev = lib.to_dev(mask)
    pinned = 0
    for k, (shrink, distance) in enumerate(sc.GRID):
        got_t = subsegment_labels(mask_dev, shrink, distance)
        assert lib.is_tensor(got_t) and got_t.dtype == lib.torch().int32 and tuple(got_t.shape) == mask.shape
        got = host(got_t)
        want = sc.restated(volume, shrink, distance)
        assert np.array_equal(got, want), (volume, shrink, distance, int((got != want).sum()))
        if sc.tie_free(volume, shrink, distance):
            ref = sc.reference(volume, shrink, distance)
            assert np.array_equal(got, ref), (volume, shrink, distance, int((got != ref).sum()))
            pinned += 1
        if k % 4 == 0:                                            # NumPy in, NumPy out (int32), for some of the grid
            got_n = subsegment_labels(mask, shrink_factor=shrink, peak_min_distance=distance)
            assert isinstance(got_n, np.ndarray) and got_n.dtype == np.int32 and np.array_equal(got_n, got)
    assert pinned >= 3


def test_defaults_are_the_reference_s(lib):
    from tobac_flow_amd.label import subsegment_labels
    mask = sc.masks("dumbbell")
    assert np.array_equal(subsegment_labels(mask), sc.restate(mask, 0.1, 5))
    assert np.array_equal(subsegment_labels(mask.astype(np.float32) * 3.5, 0.3, 10), sc.reference("dumbbell", 0.3, 10))  # != 0 counts
    from tobac_flow_amd.label import subsegment_labels_dev
    stats = []
    subsegment_labels_dev(lib.to_dev(mask), 0.3, 10, stats=stats)
    assert [frame for frame, _ in stats] == [0, 1] and all("sweeps" in st for _, st in stats)       # the empty frame is not flooded


def _prepare_numpy(labels, d2, counts, shrink):
    n_labels = counts.size - 1
    ok = (labels >= 0) & (labels <= n_labels)
    safe = np.where(ok, labels, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.sqrt(d2.astype(np.float64)) / ((counts / np.pi) ** 0.5)[safe]
    dist = np.where(ok, dist, 0.0)
    return dist, (dist > shrink).astype(np.uint8)


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (4, 0), (1027, 0), (1027, 1), (70001, 0), (70001, 3), (4 * 256 * 9 + 2, 0)])
def test_prepare_equals_numpy_bit_for_bit(lib, n, offset):
    """tf_subseg_prepare on arbitrary labels, squared distances and counts: lengths that are no multiple of 4 (the tail),
    more than one workgroup, and views that start 4, or 12, bytes into a buffer (the one-voxel-per-lane form)"""
    t = lib.torch()
    rng = np.random.default_rng(n + offset)
    n_labels = 37
    counts = rng.integers(1, 5000, n_labels + 1).astype(np.int64)
    labels = rng.integers(0, n_labels + 1, n).astype(np.int32)
    labels[rng.integers(0, n, max(n // 50, 1))] = rng.choice([-1, n_labels + 1, 2 ** 31 - 1, -2 ** 31])   # no count: background
    d2 = np.where(labels > 0, rng.integers(1, 2 ** 20, n), 0).astype(np.int32)
    d2[rng.integers(0, n, 2)] = 2 ** 31 - 1
    shrink = 0.3
    want_dist, want_mask = _prepare_numpy(labels, d2, counts, shrink)
    pad = 8
    lab_d, d2_d = (lib.to_dev(np.concatenate([np.zeros(offset, np.int32), a, np.zeros(pad, np.int32)]))[offset:offset + n]
                   for a in (labels, d2))
    dist_d = t.full((offset + n + pad,), -7.0, dtype=t.float64, device=lab_d.device)
    mask_d = t.full((offset + n + pad,), 9, dtype=t.uint8, device=lab_d.device)
    counts_d = lib.to_dev(counts)
    rc = lib.lib().tf_subseg_prepare(lib.ptr(lab_d), lib.ptr(d2_d), lib.ptr(counts_d), n_labels, n, shrink,
                                     lib.ptr(dist_d[offset:]), lib.ptr(mask_d[offset:]), lib.stream_ptr())
    assert rc == 0, lib.lib().tf_last_error()
    dist, mask = host(dist_d), host(mask_d)
    assert np.array_equal(dist[offset:offset + n], want_dist) and np.array_equal(mask[offset:offset + n], want_mask)
    assert (dist[:offset] == -7.0).all() and (dist[offset + n:] == -7.0).all()            # nothing written outside [0, n)
    assert (mask[:offset] == 9).all() and (mask[offset + n:] == 9).all()
    assert n < 100 or (want_mask.any() and not want_mask.all())


def test_prepare_on_a_volume_equals_the_restatement_s_distance_mask(lib):
    """the chain tf_label -> tf_edt2d_frames -> tf_label_sizes -> tf_subseg_prepare against SciPy's float64 transform divided
    by numpy's radius: array_equal, for every shrink factor of the grid"""
    from tobac_flow_amd import ndimage_dev as nd
    from tobac_flow_amd.label import _label_sizes_dev
    t = lib.torch()
    for volume in ("blobs", "wide", "border"):
        want_labels, want_dist = sc.distance_mask(sc.masks(volume))
        labels = nd.flat_label(lib.to_dev(sc.masks(volume)))
        assert np.array_equal(host(labels), want_labels)
        d2, _ = nd.edt_squared_frames(labels == 0)
        counts = _label_sizes_dev(labels, int(labels.max()))
        for shrink in sc.SHRINKS:
            dist, shrunk = t.empty(labels.shape, dtype=t.float64, device=labels.device), t.empty(labels.shape, dtype=t.uint8, device=labels.device)
            assert lib.lib().tf_subseg_prepare(lib.ptr(labels), lib.ptr(d2), lib.ptr(counts), counts.numel() - 1, labels.numel(),
                                               shrink, lib.ptr(dist), lib.ptr(shrunk), lib.stream_ptr()) == 0
            assert np.array_equal(host(dist), want_dist)
            assert np.array_equal(host(shrunk), (want_dist > shrink).astype(np.uint8))


@pytest.mark.parametrize("n,n_keys", [(1, 1), (5, 2), (70001, 1), (70001, 977), (70001, 70001)])
def test_rank_equals_searchsorted(lib, n, n_keys):
    """tf_subseg_rank: values that differ in the last bits of float64 (equal in float32) get different ranks; the rank is
    that of -value among the distinct -values"""
    t = lib.torch()
    rng = np.random.default_rng(n_keys)
    keys = np.unique(np.concatenate([[0.0], 1.0 + np.arange(n_keys - 1) * 2.0 ** -45]))[:n_keys]
    assert keys.size == n_keys
    values = keys[rng.integers(0, n_keys, n)]
    values[:min(n, n_keys)] = keys[:min(n, n_keys)][::-1]             # (every key occurs when n >= n_keys)
    want = sc.rank_key(-values) if n >= n_keys else (n_keys - 1 - np.searchsorted(keys, values)).astype(np.float32)
    rank = t.full((n + 4,), -1.0, dtype=t.float32, device=lib.device())
    values_d, keys_d = lib.to_dev(values), lib.to_dev(keys)
    rc = lib.lib().tf_subseg_rank(lib.ptr(values_d), n, lib.ptr(keys_d), n_keys, lib.ptr(rank), lib.stream_ptr())
    assert rc == 0, lib.lib().tf_last_error()
    got = host(rank)
    assert np.array_equal(got[:n], want) and (got[n:] == -1.0).all()


def test_error_paths(lib):
    from tobac_flow_amd.label import subsegment_labels
    full = np.zeros((3, 6, 7), bool)
    full[2] = True
    full[0, 1:3, 2:5] = True
    with pytest.raises(ValueError, match="frame 2 has no background"):
        subsegment_labels(full)
    with pytest.raises(ValueError, match="frame 2 has no background"):
        subsegment_labels(lib.to_dev(full), 0.3, 2)
    with pytest.raises(ValueError):
        subsegment_labels(np.zeros((6, 7), bool))
    keys = lib.to_dev(np.arange(4, dtype=np.float64))
    out = lib.torch().empty(4, dtype=lib.torch().float32, device=keys.device)
    with pytest.raises(ValueError, match="distinct keys"):                     # the rank overflow: refused before any launch
        lib.check(lib.lib().tf_subseg_rank(lib.ptr(keys), 4, lib.ptr(keys), 2 ** 24 + 1, lib.ptr(out), lib.stream_ptr()), "tf_subseg_rank")
    assert subsegment_labels(np.zeros((2, 6, 7), bool)).sum() == 0             # nothing to split is no error


def _flow(case):
    import tobac_flow_amd.flow as tf
    return tf.Flow(case["forward"], case["backward"])


def test_flow_label_with_subsegment_shrink_equals_the_reference(lib):
    """Flow.label(mask, overlap=0.5, subsegment_shrink=0.3) against the reference's flow_label on the same mask and (integer-
    valued) flows; raised NotImplementedError before subsegment_labels existed"""
    case, p = sc.flow_case(), dict(sc.FLOW_PARAMS)
    assert p["overlap"] == 0.5 and p["subsegment_shrink"] == 0.3
    flow = _flow(case)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = flow.label(case["mask"], **p)
        got_t = flow.label(lib.to_dev(case["mask"]), **p)
    assert not [w for w in caught if "Not all regions" in str(w.message)]      # every region has a marker here
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    assert np.array_equal(got, case["labels"]), int((got != case["labels"]).sum())
    assert lib.is_tensor(got_t) and np.array_equal(host(got_t), case["labels"])
    from tobac_flow_amd.label import flow_link_overlap, subsegment_labels
    flat = subsegment_labels(case["mask"], p["subsegment_shrink"], p["peak_min_distance"])
    assert np.array_equal(flat, case["subseg"])
    assert np.array_equal(flow_link_overlap(flow, flat, overlap=p["overlap"], absolute_overlap=p["absolute_overlap"]), case["labels"])


def test_flow_label_warns_where_a_region_gets_no_marker(lib):
    """a thin region inside the border zone of the peak search that the shrinking removes has no marker and stays 0:
    the reference's "Not all regions present" warning (label.py:172-174)"""
    case = sc.flow_case()
    mask = case["mask"].copy()
    mask[:, 0, :] = False
    mask[:, 1, :] = False
    mask[1, 0, 3:40] = True                                                    # dist 1 everywhere, radius sqrt(37 / pi) > 1 / 0.3
    want_flat = sc.restate(mask, 0.3, 5)
    assert not want_flat[1, 0].any()
    with pytest.warns(RuntimeWarning, match="Not all regions present"):
        got = _flow(case).label(mask, overlap=0.5, absolute_overlap=1, subsegment_shrink=0.3, peak_min_distance=5)
    assert np.array_equal(got != 0, want_flat != 0)


def test_get_anvil_markers_with_subsegment_shrink_equals_the_host_composition(lib):
    from oracle import np_label
    from tobac_flow_amd.analysis import find_object_lengths
    from tobac_flow_amd.detection import _get_anvil_markers_host, get_anvil_markers
    from tobac_flow_amd.utils import remap_labels
    case = sc.flow_case()
    flow = _flow(case)
    field = np.where(case["mask"], 0.0, -10.0).astype(np.float32)
    kw = dict(threshold=-5, overlap=0.5, absolute_overlap=4, subsegment_shrink=0.3, min_length=1)
    got = get_anvil_markers(flow, field, **kw)
    s = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    opened = ndi.binary_opening(field >= -5, structure=s)
    flat = sc.restate(opened, 0.3, 5)                                          # Flow.label's peak_min_distance default
    lab = np_label.flow_link_overlap(case["forward"], case["backward"], flat, overlap=0.5, absolute_overlap=4)
    want = remap_labels(lab, find_object_lengths(lab) > 1)
    assert got.dtype == want.dtype and np.array_equal(got, want) and want.max() > 1
    assert np.array_equal(_get_anvil_markers_host(flow, field, **kw), want)
    got_t = get_anvil_markers(flow, lib.to_dev(field), **kw)
    assert lib.is_tensor(got_t) and np.array_equal(host(got_t), want)
