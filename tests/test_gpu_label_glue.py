"""The label glue on the GPU (tf_label, tf_flow_label, tf_flow_link_overlap, tf_pair_counts, tf_pair_rank, tf_slice_labels,
tf_apply_lut, tf_window_overlap_pairs and their Python entry points) against what the REFERENCE's own functions wrote into
tests/golden/label_glue_ref.npz, on the cases of tests/label_glue_cases.py: the shapes at which the kernels change path, the
two overlap rules ON their decision boundaries, labels that warp out of the frame, ids without pixels, empty and full
volumes.  Every comparison is an equality of integers; entry points that take both are run on numpy input and on device
tensors."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

import label_glue_cases as gc

pytestmark = pytest.mark.gpu

FLOW_CASES = gc.flow_label_cases()
DEFAULT = ndi.generate_binary_structure(3, 1)


@pytest.fixture(scope="module")
def L():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib.lib()


@pytest.fixture(scope="module")
def ref():
    return gc.fixture()


@pytest.fixture(scope="module")
def link_cases(ref):
    return gc.link_cases({gc.shape_name(s): ref[f"utils/{gc.shape_name(s)}/make_step_labels"] for s in gc.SHAPES})


def f32(v):
    return v.astype(np.float32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def view_from_frame_one(a, fill=0):
    """the array as the frames 1 .. T of a device allocation of T + 1 frames: for int32 volumes with an odd H * W the view
    is 4-byte aligned only, for uint8 ones it has no alignment at all"""
    import torch
    big = torch.full((a.shape[0] + 1,) + tuple(a.shape[1:]), fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    big[1:] = dev(a)
    return big[1:]


def flows_of(forward, backward, on_device):
    from tobac_flow_amd.flow import Flow
    return Flow(dev(f32(forward)), dev(f32(backward))) if on_device else Flow(f32(forward), f32(backward))


@pytest.fixture(autouse=True)
def no_runtime_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)              # "Not all regions present": none of these cases subsegments
        yield


def test_label_with_the_flat_structures_equals_flat_label(L):
    from tobac_flow_amd import ndimage_dev as nd
    for name in gc.FLAT_CASES:
        mask = FLOW_CASES[name][0]
        for which, structure in (("default", DEFAULT), ("full", gc.FULL)):
            want = gc.expected_flat(name, which)
            plane = np.array(structure, bool)
            plane[0] = plane[2] = False
            got, n = nd.label(dev(mask), plane)
            assert got.dtype.is_floating_point is False and np.array_equal(host(got), want) and n == want.max(), (name, which)
            assert np.array_equal(host(nd.flat_label(dev(mask.astype(np.uint8)), structure)), want), (name, which)


@pytest.mark.parametrize("name", list(FLOW_CASES))
def test_flow_label_equals_the_reference(L, name):
    mask, forward, backward, grid = FLOW_CASES[name]
    for on_device in (False, True):
        flow = flows_of(forward, backward, on_device)
        for (overlap, absolute), want in gc.expected_flow_label(name, grid).items():
            got = flow.label(dev(mask) if on_device else mask, overlap=overlap, absolute_overlap=absolute)
            assert (hasattr(got, "cpu")) == on_device
            got = host(got)
            assert got.dtype == np.int32 and np.array_equal(got, want), \
                f"{name} overlap {overlap} absolute_overlap {absolute} device input {on_device}: {int((got != want).sum())} px differ"


def test_link_overlap_equals_the_reference(L, link_cases):
    for name, (flat, forward, backward, grid) in link_cases.items():
        for on_device in (False, True):
            flow = flows_of(forward, backward, on_device)
            for (overlap, absolute), (want, _) in gc.expected_link(name, flat, grid).items():
                got = host(flow.link_overlap(dev(flat) if on_device else flat, overlap=overlap, absolute_overlap=absolute))
                assert got.dtype == np.int32 and np.array_equal(got, want), (name, overlap, absolute, on_device)


def _c_abi(L, fn, size_fn, volume, forward, backward, overlap, absolute):
    """tf_flow_label / tf_flow_link_overlap the way a C host calls them, input and output on views that start at frame 1 of
    larger allocations; returns (labels, n_objects_host)"""
    import torch
    from tobac_flow_amd import _lib
    T, H, W = volume.shape
    src = view_from_frame_one(volume)
    out = view_from_frame_one(np.full(volume.shape, -7, np.int32), fill=-7)
    fw, bw = dev(f32(forward)), dev(f32(backward))
    st = np.ascontiguousarray(DEFAULT, np.uint8)
    ws = torch.empty(size_fn(T, H, W, 0), dtype=torch.uint8, device="cuda")
    n_obj = ctypes.c_int(-1)
    rc = fn(_lib.ptr(src), _lib.ptr(fw), _lib.ptr(bw), T, H, W, st.ctypes.data_as(_lib._P), float(overlap), int(absolute),
            _lib.ptr(out), ctypes.byref(n_obj), _lib.ptr(ws), ws.numel(), None)
    assert rc == 0, L.tf_last_error()
    big = out._base if out._base is not None else out
    assert (big.reshape(-1)[:H * W] == -7).all()                         # nothing written in front of the view
    return host(out), n_obj.value


def test_c_abi_on_views_that_start_at_frame_one(L, ref, link_cases):
    unaligned = gc.seeded_name(gc.UNALIGNED, 1)
    for name in ("product_edge", unaligned):
        mask, forward, backward, grid = FLOW_CASES[name]
        for (overlap, absolute), want in gc.expected_flow_label(name, grid).items():
            got, n = _c_abi(L, L.tf_flow_label, L.tf_flow_label_workspace_bytes, mask.astype(np.uint8), forward, backward, overlap, absolute)
            assert np.array_equal(got, want) and n == want.max(), (name, overlap, absolute, n)
    for name in ("gap_ids", f"steps/{gc.shape_name(gc.UNALIGNED)}"):
        flat, forward, backward, grid = link_cases[name]
        for (overlap, absolute), (want, groups) in gc.expected_link(name, flat, grid).items():
            got, n = _c_abi(L, L.tf_flow_link_overlap, L.tf_flow_link_workspace_bytes, flat, forward, backward, overlap, absolute)
            assert np.array_equal(got, want) and n == groups, (name, overlap, absolute, n, groups)
            assert name == "gap_ids" or groups == want.max()


def test_make_step_labels_dev_on_aligned_and_unaligned_views(L, ref):
    from tobac_flow_amd.label import make_step_labels_dev
    for shape in gc.SHAPES:
        labels, want = gc.tile_labels(shape), ref[f"utils/{gc.shape_name(shape)}/make_step_labels"]
        view = view_from_frame_one(labels)
        assert (view.data_ptr() % 16 != 0) == ((shape[1] * shape[2] * 4) % 16 != 0)
        for given in (labels, dev(labels), view):
            got = make_step_labels_dev(given)
            assert got.dtype.is_floating_point is False and np.array_equal(host(got), want), shape
    assert view_from_frame_one(gc.tile_labels(gc.UNALIGNED)).data_ptr() % 16 and not view_from_frame_one(gc.tile_labels(gc.ALIGNED)).data_ptr() % 16


def test_slice_labels_dev_equals_slice_labels(L, ref):
    from tobac_flow_amd.label import slice_labels_dev
    for shape in gc.SHAPES:
        labels, want = gc.tile_labels(shape), ref[f"utils/{gc.shape_name(shape)}/slice_labels"]
        for given in (labels, dev(labels), view_from_frame_one(labels)):
            got, n = slice_labels_dev(given)
            assert np.array_equal(host(got), want) and n == want.max(), shape


def test_remap_labels_and_apply_lut_equal_remap_labels(L, ref):
    import torch
    from tobac_flow_amd import _lib, ndimage_dev as nd
    for shape in gc.SHAPES:
        key = f"utils/{gc.shape_name(shape)}/"
        labels = gc.tile_labels(shape)
        forms = gc.remap_arguments(labels)
        for given in (dev(labels), view_from_frame_one(labels)):
            assert np.array_equal(host(nd.remap_labels(given, forms["bool"][0])), ref[key + "remap_bool"]), shape
            tables = {"new": np.concatenate([[0], forms["new"][1]]).astype(np.int32)}
            picked, new = forms["int"]
            tables["int"] = np.zeros(max(int(labels.max()), new.size) + 1, np.int32)
            tables["int"][picked] = new
            for form, table in tables.items():
                out = view_from_frame_one(np.zeros(shape, np.int32))
                lut = dev(table)
                assert L.tf_apply_lut(_lib.ptr(given), given.numel(), _lib.ptr(lut), lut.numel(), _lib.ptr(out), None) == 0
                torch.cuda.synchronize()
                assert np.array_equal(host(out), ref[key + "remap_" + form]), (shape, form)


def test_pair_counts_reproduce_find_overlapping_labels(L):
    """label.pair_counts on (step labels, warped labels) and the reference's rule -- count > absolute_overlap and
    count >= overlap * min(n, size), a product -- give the neighbours find_overlapping_labels gave label by label"""
    from tobac_flow_amd.label import pair_counts
    for name in gc.OVERLAPPING_CASES:
        mask, forward, backward, _ = FLOW_CASES[name]
        flat = gc.expected_flat(name)
        back, fwd = gc.warped_labels(flat, forward, backward)
        sizes = np.bincount(flat.ravel())
        for on_device in (False, True):
            counted = [pair_counts(dev(flat), dev(w)) if on_device else pair_counts(flat, w) for w in (fwd, back)]
            for (overlap, absolute), want in gc.expected_overlapping(name, gc.overlapping_grid(name)).items():
                rows = []
                for d, (a, b, c) in enumerate(counted):
                    ok = (c > absolute) & (c >= overlap * np.minimum(sizes[a], sizes[b]))
                    rows.append(np.stack([np.full(int(ok.sum()), d), a[ok], b[ok]], 1))
                assert np.array_equal(np.concatenate(rows), want), (name, overlap, absolute, on_device)


def test_overlap_pairs_and_the_stitch_equal_the_reference(L):
    from tobac_flow_amd.parallel import overlap_pairs, stitch_lut
    for name, (left, right, grid) in gc.window_cases().items():
        n_left, n_right = int(left.max()), int(right.max())
        left_dev, right_dev = dev(left), dev(right)
        for (atol, rtol), (pairs, components) in gc.expected_window(name, grid).items():
            got = overlap_pairs(left_dev, right_dev, atol, rtol)
            assert got.dtype == np.int64 and np.array_equal(got, pairs), (name, atol, rtol, got.tolist(), pairs.tolist())
            luts = stitch_lut([n_left, n_right], [got])
            assert len(luts[0]) == n_left + 1 and len(luts[1]) == n_right + 1
            stitched = np.concatenate([luts[0][1:], luts[1][1:]])          # the nodes 1 .. n_left + n_right of node_ids' graph
            assert np.array_equal(gc.canonical_partition(stitched), gc.canonical_partition(components[1:])), (name, atol, rtol)
