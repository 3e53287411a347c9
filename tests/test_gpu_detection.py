"""Detection recipes end to end on the GPU path against the same recipes assembled from oracle pieces
(the scipy.ndimage glue is identical by construction; what is checked is the plumbing through Flow.diff /
convolve / sobel / watershed / label, i.e. SURVEY.md section 8 row a17)."""
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

from helpers import blob_sequence, rand_flow

pytestmark = pytest.mark.gpu


class FakeCoord:
    """the part of an xarray coordinate the recipes touch: `.values` / `.data` give the datetime64 array
    (a plain ndarray would not do: ndarray.data is the raw buffer, which numpy refuses for datetime64)"""

    def __init__(self, values):
        self.values = self.data = values

    def __array__(self, dtype=None, copy=None):
        return self.values if dtype is None else self.values.astype(dtype)

    def __len__(self):
        return len(self.values)

    def __getitem__(self, i):
        return self.values[i]


class FakeDataArray(np.ndarray):
    """ndarray with the two xarray attributes the recipes touch: `.t` (time coordinate) and `.to_numpy()`"""

    def __new__(cls, data, minutes=10):
        obj = np.asarray(data).view(cls)
        obj.t = FakeCoord(np.datetime64("2020-06-01T00:00") + np.arange(obj.shape[0]) * np.timedelta64(minutes, "m"))
        return obj

    def __array_finalize__(self, obj):
        self.t = getattr(obj, "t", None)

    def to_numpy(self):
        return np.asarray(self)


@pytest.fixture(scope="module")
def scene():
    import tobac_flow_amd.flow as tf
    rng = np.random.default_rng(42)
    bt = blob_sequence(rng, 6, 96, 120, n_blobs=5, vmax=2.0, noise=0.5)
    flow = tf.create_flow(bt, smoothing_passes=1, interp_method="cubic")
    return dict(tf=tf, bt=bt, flow=flow, fwd=flow.forward_flow, bwd=flow.backward_flow)


def test_detect_anvils_matches_oracle_recipe(scene):
    from oracle import np_ops, ws_oracle
    from tobac_flow_amd.detection import detect_anvils
    from tobac_flow_amd.analysis import find_object_lengths, mask_labels
    from tobac_flow_amd.utils import linearise_field, remap_labels
    bt, fwd, bwd = scene["bt"], scene["fwd"], scene["bwd"]
    wvd = (250.0 - bt) / 2.0 - 10.0           # WVD-like: positive in the cold cores
    got = detect_anvils(scene["flow"], wvd, upper_threshold=-5, lower_threshold=-15, min_length=1)
    # the same recipe from oracle pieces (reference detection.py:538-587)
    field = linearise_field(wvd, -15, -5)
    s = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    markers = field >= 1
    seeds = markers * ndi.binary_erosion(markers != 0, structure=s).astype(int)
    nan = np.isnan(field)
    bg = ndi.binary_erosion(np.logical_or(field <= 0, nan), structure=np.ones([3, 3, 3]), iterations=1, border_value=1)
    bg[nan] = True
    seeds[bg] = -1
    edges = np_ops.sobel(field, fwd, bwd, "cubic", None, np.nan, "uphill")
    edges[edges > 0] += 1
    edges = edges - field
    edges[np.isnan(field)] = np.inf
    lab = ws_oracle.watershed(fwd, bwd, edges, seeds, None, ndi.generate_binary_structure(3, 1))
    lab[lab < 0] = 0
    lab *= ndi.binary_opening(lab != 0, structure=s).astype(int)
    lab[markers > 0] = markers[markers > 0]
    want = remap_labels(lab, np.logical_and(find_object_lengths(lab) > 1, mask_labels(lab, markers != 0)))
    assert got.shape == bt.shape and np.array_equal(got, want)
    assert got.max() >= 1


def test_detect_anvils_with_component_markers_equals_the_reference_kernel(scene):
    """the drop-in call with markers = component ids (scripts/dcc_detect_goes.py:221-235 pass labelled cores) --
    equal-valued markers of DIFFERENT labels then decide voxels, and the default call must return what the reference's own
    heap returns (oracle twin in the reference's semantics, tie_mode=0), on the numpy path and on the device path; no
    warning is left to give."""
    import torch
    from oracle import np_ops, ws_oracle
    from tobac_flow_amd.detection import detect_anvils
    from tobac_flow_amd.analysis import find_object_lengths, mask_labels
    from tobac_flow_amd.utils import linearise_field, remap_labels
    tf = scene["tf"]
    bt = blob_sequence(np.random.default_rng(43), 6, 128, 160, n_blobs=14, vmax=2.0, noise=0.5)      # several cold cores
    flow = tf.create_flow(bt, smoothing_passes=1, interp_method="cubic")
    fwd, bwd = flow.forward_flow, flow.backward_flow
    wvd = (250.0 - bt) / 2.0 - 10.0
    field = linearise_field(wvd, -15, -5)
    s = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    markers = ndi.label(field >= 1)[0].astype(np.int32)               # component ids
    assert markers.max() >= 3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = detect_anvils(flow, wvd, markers=markers, upper_threshold=-5, lower_threshold=-15, min_length=1)
        got_dev = detect_anvils(flow, torch.from_numpy(wvd.astype(np.float32)).cuda(), markers=torch.from_numpy(markers).cuda(),
                                upper_threshold=-5, lower_threshold=-15, min_length=1)
    seeds = markers * ndi.binary_erosion(markers != 0, structure=s).astype(int)
    nan = np.isnan(field)
    bg = ndi.binary_erosion(np.logical_or(field <= 0, nan), structure=np.ones([3, 3, 3]), iterations=1, border_value=1)
    bg[nan] = True
    seeds[bg] = -1
    edges = np_ops.sobel(field, fwd, bwd, "cubic", None, np.nan, "uphill")
    edges[edges > 0] += 1
    edges = edges - field
    edges[np.isnan(field)] = np.inf
    lab = ws_oracle.watershed(fwd, bwd, edges, seeds, None, ndi.generate_binary_structure(3, 1), tie_mode=0)
    lab[lab < 0] = 0
    lab *= ndi.binary_opening(lab != 0, structure=s).astype(int)
    lab[markers > 0] = markers[markers > 0]
    want = remap_labels(lab, np.logical_and(find_object_lengths(lab) > 1, mask_labels(lab, markers != 0)))
    assert np.array_equal(got, want)
    assert np.array_equal(got_dev.cpu().numpy(), want)


def test_growth_rate_and_markers_match_oracle(scene):
    from oracle import np_ops
    from tobac_flow_amd.detection import filtered_tdiff, get_growth_rate
    bt, fwd, bwd, flow = scene["bt"], scene["fwd"], scene["bwd"], scene["flow"]
    da = FakeDataArray(-bt, minutes=10)
    for method in ("linear", "cubic"):
        got = get_growth_rate(flow, da, method=method)
        dt = np.full(bt.shape[0], 10.0)
        rate = np_ops.diff(np.asarray(da), fwd, bwd, method) / dt[:, None, None]
        s_struct = ndi.generate_binary_structure(3, 1)
        s_struct[0] = 0
        s_struct[2] = 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np_ops.convolve(rate, fwd, bwd, s_struct, method, func=lambda x: np.nanmean(x, 0))
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    raw = flow.diff(bt)
    t_struct = np.zeros([3, 3, 3])
    t_struct[:, 1, 1] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np_ops.convolve(raw, fwd, bwd, t_struct, "linear", func=lambda x: np.nanmean(x, 0))
    got = filtered_tdiff(flow, raw)
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want))


def test_get_anvil_markers_and_relabel(scene):
    from oracle import np_label
    from tobac_flow_amd.analysis import find_object_lengths
    from tobac_flow_amd.detection import get_anvil_markers, relabel_anvils
    from tobac_flow_amd.utils import remap_labels
    from tobac_flow_amd.utils.label_utils import make_step_labels
    bt, fwd, bwd, flow = scene["bt"], scene["fwd"], scene["bwd"], scene["flow"]
    wvd = (250.0 - bt) / 2.0 - 10.0
    got = get_anvil_markers(flow, wvd, threshold=-5, overlap=0.5, absolute_overlap=5, min_length=1)
    s = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    mask = ndi.binary_opening(wvd >= -5, structure=s)
    lab = np_label.flow_label(fwd, bwd, mask, overlap=0.5, absolute_overlap=5)
    want = remap_labels(lab, find_object_lengths(lab) > 1)
    assert np.array_equal(got, want) and got.max() >= 1
    re = relabel_anvils(flow, got, overlap=0.5, absolute_overlap=5, min_length=1)
    lk = np_label.flow_link_overlap(fwd, bwd, make_step_labels(got), overlap=0.5, absolute_overlap=5)
    want = remap_labels(lk, find_object_lengths(lk) > 1)
    assert np.array_equal(re, want)
    # round 5: the recipes run in HBM whatever the container; the variants with the reference's own numpy / SciPy glue between
    # the device operators give the same labels, and device input gives device output
    import torch
    from tobac_flow_amd.detection import _get_anvil_markers_host, _relabel_anvils_host
    assert np.array_equal(_get_anvil_markers_host(flow, wvd, threshold=-5, overlap=0.5, absolute_overlap=5, min_length=1), got)
    for markers in (None, (wvd >= -2)):
        want_re = _relabel_anvils_host(flow, got, markers=markers, overlap=0.5, absolute_overlap=5, min_length=1)
        assert np.array_equal(relabel_anvils(flow, got, markers=markers, overlap=0.5, absolute_overlap=5, min_length=1), want_re)
        dev = relabel_anvils(flow, torch.from_numpy(got).cuda(), markers=None if markers is None else torch.from_numpy(markers).cuda(),
                             overlap=0.5, absolute_overlap=5, min_length=1)
        assert isinstance(dev, torch.Tensor) and np.array_equal(dev.cpu().numpy(), want_re)


def test_make_step_labels_on_the_device_equals_the_host_function():
    """utils.label_utils.make_step_labels (reference: label_utils.py:183-200) as tf_label + tf_pair_counts + tf_pair_rank:
    pieces connected within a step, split into the labels they contain, numbered by (piece, label) -- on volumes where one
    piece holds several labels, one label several pieces, labels touch diagonally only, and on an empty volume."""
    import torch
    from tobac_flow_amd.label import make_step_labels_dev
    from tobac_flow_amd.utils.label_utils import make_step_labels
    rng = np.random.default_rng(8)
    vols = []
    for shape in ((4, 37, 53), (2, 64, 64), (3, 5, 9), (1, 1, 7)):
        blobs = ndi.gaussian_filter(rng.normal(size=shape), (0, 2, 2)) > 0.02
        ids = rng.integers(1, 6, size=shape).astype(np.int32)
        ids = ndi.maximum_filter(ids, size=(1, 5, 5))                 # patches of equal label inside the blobs
        vols.append((blobs * ids).astype(np.int32))
    vols.append(np.zeros((2, 8, 8), np.int32))
    checker = np.indices((2, 9, 9)).sum(0) % 2
    vols.append((checker * 3).astype(np.int32))                       # 4-connected: every pixel its own piece
    for v in vols:
        want = make_step_labels(v)
        got = make_step_labels_dev(torch.from_numpy(v).cuda())
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), v.shape
    with pytest.raises(ValueError, match="negative"):
        make_step_labels_dev(torch.from_numpy(np.array([[[1, -1, 0]]], np.int32)).cuda())
    # a contiguous VIEW whose first voxel is not 16-byte aligned (labels[1:] with H * W % 4 != 0: ADVICE r5 -- tf_pair_rank used to
    # refuse it, where the reference's function takes any array)
    v = vols[0]                                                       # (4, 37, 53): 37 * 53 = 1961 voxels per frame, 1961 % 4 == 1
    dev = torch.from_numpy(v).cuda()
    view = dev[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert np.array_equal(make_step_labels_dev(view).cpu().numpy(), make_step_labels(v[1:]))


def test_get_combined_filters_runs_and_matches_any_reduction(scene):
    """detect_cores' cloud-top filter: the int32 / nearest / np.any convolve path"""
    from functools import partial
    from oracle import np_ops
    bt, fwd, bwd, flow = scene["bt"], scene["fwd"], scene["bwd"], scene["flow"]
    seed = (bt < 265).astype(int)
    t_struct = np.zeros([3, 3, 3], dtype=bool)
    t_struct[:, 1, 1] = True
    got = flow.convolve(seed, structure=t_struct, method="nearest", fill_value=False, dtype=np.int32,
                        func=partial(np.any, axis=0))
    want = np_ops.convolve(seed.astype(np.int32), fwd, bwd, t_struct, "nearest", np.int32, False, func=partial(np.any, axis=0))
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- section 8f-2: ndimage glue on the GPU
# 45: byte-per-thread kernel; multiples of 4: the word kernel (k_binary_morph4); multiples of 16: k_binary_morph16 (16: one
# thread per row, 1040: 65 threads = two waves per row)
@pytest.mark.parametrize("width", [45, 48, 4, 260, 16, 1040])
@pytest.mark.parametrize("iterations,border", [(1, 0), (1, 1), (3, 0), (2, 1)])
def test_binary_morphology_matches_scipy(iterations, border, width):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    rng = np.random.default_rng(iterations * 10 + border)
    x = ndi.gaussian_filter(rng.normal(size=(5, 37, width)), (0.5, 1.5, 1.5)) > 0.0
    cross = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    skew = np.zeros((3, 3, 3), bool)
    skew[0, 0, 1] = skew[1, 1, 1] = skew[1, 1, 2] = skew[2, 2, 0] = True            # asymmetric: checks the reflection rule
    for st in (cross, np.ones((3, 3, 3), bool), ndi.generate_binary_structure(3, 1), skew):
        xd = torch.from_numpy(x).cuda()
        got = nd.binary_erosion(xd, st, iterations, border).cpu().numpy()
        assert np.array_equal(got, ndi.binary_erosion(x, structure=st, iterations=iterations, border_value=border))
        got = nd.binary_dilation(xd, st, iterations, border).cpu().numpy()
        assert np.array_equal(got, ndi.binary_dilation(x, structure=st, iterations=iterations, border_value=border))
        got = nd.binary_opening(xd, st, iterations).cpu().numpy()
        assert np.array_equal(got, ndi.binary_opening(x, structure=st, iterations=iterations))


def test_device_glue_matches_numpy_glue(scene):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    from tobac_flow_amd.analysis import find_object_lengths, mask_labels
    from tobac_flow_amd.detection import get_watershed_mask
    from tobac_flow_amd.utils import linearise_field, remap_labels
    bt = scene["bt"]
    wvd = ((250.0 - bt) / 2.0 - 10.0).astype(np.float32)
    wvd[1, 10:14, 20:30] = np.nan
    for lo, hi in ((-15, -5), (-5, -15)):
        want = linearise_field(wvd, lo, hi)
        got = nd.linearise_field(torch.from_numpy(wvd).cuda(), lo, hi).cpu().numpy()
        assert want.dtype == np.float32 and np.array_equal(np.nan_to_num(got, nan=-7), np.nan_to_num(want, nan=-7))
    lin = linearise_field(wvd, -15, -5)
    for e in (1, 2):
        assert np.array_equal(get_watershed_mask(torch.from_numpy(lin).cuda(), e).cpu().numpy(), get_watershed_mask(lin, e))
    lab = ndi.label(lin > 0.3)[0].astype(np.int32)
    msk = lin >= 1
    lengths, hits, _ = nd.label_filter(torch.from_numpy(lab).cuda(), [torch.from_numpy(msk).cuda()])
    hit = hits[:, 0]
    assert np.array_equal(lengths, find_object_lengths(lab)) and np.array_equal(hit, mask_labels(lab, msk))
    keep = np.logical_and(lengths > 1, hit)
    assert np.array_equal(nd.remap_labels(torch.from_numpy(lab).cuda(), keep).cpu().numpy(), remap_labels(lab, keep))


def test_detect_anvils_device_path_equals_numpy_path(scene):
    import torch
    from tobac_flow_amd.detection import detect_anvils
    bt = scene["bt"]
    wvd = ((250.0 - bt) / 2.0 - 10.0).astype(np.float32)
    from tobac_flow_amd.detection import _detect_anvils_host
    want = _detect_anvils_host(scene["flow"], wvd, upper_threshold=-5, lower_threshold=-15, min_length=1)   # the reference's own glue
    assert np.array_equal(detect_anvils(scene["flow"], wvd, upper_threshold=-5, lower_threshold=-15, min_length=1), want)
    got = detect_anvils(scene["flow"], torch.from_numpy(wvd).cuda(), upper_threshold=-5, lower_threshold=-15, min_length=1)
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_label_matches_scipy(conn):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    rng = np.random.default_rng(conn)
    for shape, thr in (((4, 33, 47), 0.0), ((1, 64, 64), 0.3), ((6, 20, 130), -0.2), ((2, 1, 1), -9.0)):
        x = ndi.gaussian_filter(rng.normal(size=shape), (0.4, 1.2, 1.2)) > thr
        st = ndi.generate_binary_structure(3, conn)
        want, n = ndi.label(x, structure=st)
        got, ng = nd.label(torch.from_numpy(x).cuda(), st)
        assert ng == n and np.array_equal(got.cpu().numpy(), want)
        flat = st.copy()
        flat[0] = 0
        flat[-1] = 0
        want = ndi.label(x, structure=flat, output=np.int32)[0]
        assert np.array_equal(nd.flat_label(torch.from_numpy(x).cuda(), st).cpu().numpy(), want)
    snake = np.zeros((1, 40, 41), bool)           # long serpentine component: deep union-find chains
    snake[0, ::2, :] = True
    snake[0, 1::4, -1] = True
    snake[0, 3::4, 0] = True
    want, n = ndi.label(snake)
    got, ng = nd.label(torch.from_numpy(snake).cuda())
    assert ng == n == 1 and np.array_equal(got.cpu().numpy(), want)


def test_anvil_pipeline_device_resident_equals_numpy(scene):
    """get_anvil_markers -> detect_anvils(markers=...) entirely on the device == the numpy recipes"""
    import torch
    from tobac_flow_amd.detection import _detect_anvils_host, _get_anvil_markers_host, detect_anvils, get_anvil_markers
    bt, flow = scene["bt"], scene["flow"]
    wvd = ((250.0 - bt) / 2.0 - 10.0).astype(np.float32)
    m_np = _get_anvil_markers_host(flow, wvd, threshold=-5, overlap=0.5, absolute_overlap=5, min_length=1)
    a_np = _detect_anvils_host(flow, wvd, markers=m_np, upper_threshold=-5, lower_threshold=-15, min_length=1)
    assert np.array_equal(detect_anvils(flow, wvd, markers=m_np, upper_threshold=-5, lower_threshold=-15, min_length=1), a_np)
    wd = torch.from_numpy(wvd).cuda()
    m_dev = get_anvil_markers(flow, wd, threshold=-5, overlap=0.5, absolute_overlap=5, min_length=1)
    a_dev = detect_anvils(flow, wd, markers=m_dev, upper_threshold=-5, lower_threshold=-15, min_length=1)
    assert isinstance(m_dev, torch.Tensor) and np.array_equal(m_dev.cpu().numpy(), m_np)
    assert np.array_equal(a_dev.cpu().numpy(), a_np) and a_np.max() >= 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(3, 40, 50), (2, 5, 7), (1, 17, 3), (2, 1, 9), (4, 33, 65)])
def test_gaussian_filter_matches_scipy_bit_for_bit(dtype, shape):
    """ndi.gaussian_filter as the recipes call it (detection.py:65, 137-138, 150) and with a time sigma
    (detect_growth_markers_multichannel); axes shorter than the kernel radius exercise the repeated reflection."""
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    rng = np.random.default_rng(sum(shape))
    x = (rng.normal(size=shape) * 10).astype(dtype)
    xd = torch.from_numpy(x).cuda()
    for sigma in [(0, 2, 2), (1, 2, 2), (0, 0.7, 3.1), 1.5, (0, 0, 0), (2.5, 0, 0)]:
        want = ndi.gaussian_filter(x, sigma)
        got = nd.gaussian_filter(xd, sigma)
        assert got.dtype == xd.dtype and got.data_ptr() != xd.data_ptr()
        got = got.cpu().numpy()
        assert np.array_equal(got, want), f"sigma {sigma}: {int((got != want).sum())} values differ, max {np.abs(got - want).max()}"
    w, r = nd.gaussian_kernel1d(2.0)
    from scipy.ndimage._filters import _gaussian_kernel1d
    assert r == 8 and np.array_equal(w, _gaussian_kernel1d(2.0, 0, 8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(2, 9, 11), (1, 1, 6), (3, 4, 1), (3, 31, 47)])
def test_grey_morphology_matches_scipy_including_nan_placement(dtype, shape):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    rng = np.random.default_rng(7 + sum(shape))
    x = rng.normal(size=shape).astype(dtype)
    x[rng.random(shape) < 0.08] = np.nan
    xd = torch.from_numpy(x).cuda()
    cross2d = ndi.generate_binary_structure(2, 1)[np.newaxis, ...]                  # detection.py:105
    diag = np.zeros((3, 3, 3), bool)
    diag[0, 0, 0] = diag[1, 1, 1] = diag[2, 2, 2] = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fp in (cross2d, ndi.generate_binary_structure(3, 1), ndi.generate_binary_structure(3, 2), diag):
            for name in ("grey_erosion", "grey_dilation", "grey_opening"):
                want = getattr(ndi, name)(x, footprint=fp)
                got = getattr(nd, name)(xd, fp).cpu().numpy()
                assert np.array_equal(got, want, equal_nan=True), f"{name} {fp.shape}: {int((~np.isclose(got, want, equal_nan=True)).sum())} differ"
    with pytest.raises(NotImplementedError):
        nd.grey_erosion(xd, np.ones((3, 3, 3), bool))
    with pytest.raises(ValueError):
        skew = np.zeros((3, 3, 3), bool)
        skew[1, 1, 1] = skew[1, 1, 2] = True
        nd.grey_erosion(xd, skew)


@pytest.mark.parametrize("shape", [(4, 41, 53), (1, 30, 30), (3, 8, 9)])
def test_binary_fill_holes_matches_scipy(shape):
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    rng = np.random.default_rng(11 + sum(shape))
    field = ndi.gaussian_filter(rng.normal(size=shape), (0.7, 2, 2))
    rings = np.logical_and(field > 0.02, field < 0.09)                              # thin closed curves: many holes
    blobs = field > 0.05
    per_frame = ndi.generate_binary_structure(3, 1)
    per_frame[0] = 0
    per_frame[2] = 0                                                                # detection.py:72-74
    for x in (rings, blobs, np.zeros(shape, bool), np.ones(shape, bool)):
        xd = torch.from_numpy(x).cuda()
        for st in (per_frame, ndi.generate_binary_structure(3, 1), ndi.generate_binary_structure(3, 3)):
            want = ndi.binary_fill_holes(x, structure=st)
            got = nd.binary_fill_holes(xd, st).cpu().numpy()
            assert got.dtype == bool and np.array_equal(got, want), f"{int((got != want).sum())} px differ"
    if shape[1] >= 30:                                                              # (the 8 x 9 case is too small to enclose anything)
        assert ndi.binary_fill_holes(rings, structure=per_frame).sum() > rings.sum()    # the case really has holes


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("direction", ["negative", "positive"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_curvature_filter_device_path_equals_scipy_path(scene, direction, dtype):
    import torch
    from tobac_flow_amd.detection import get_curvature_filter
    field = (-scene["bt"]).astype(dtype)
    for sigma, threshold in [(2, 0), (1.2, 0.01)]:
        want = get_curvature_filter(field, sigma=sigma, threshold=threshold, direction=direction)
        got = get_curvature_filter(torch.from_numpy(field).cuda(), sigma=sigma, threshold=threshold, direction=direction)
        assert isinstance(got, torch.Tensor) and _same(got.cpu().numpy(), want)
        assert 0 < want.sum() < want.size                      # a non-trivial filter
    with pytest.raises(ValueError):
        get_curvature_filter(torch.from_numpy(field).cuda(), direction="sideways")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_gaussian_filter_device_path_equals_scipy_path(scene, dtype):
    import torch
    from tobac_flow_amd.detection import nan_gaussian_filter
    rng = np.random.default_rng(5)
    a = scene["bt"].astype(dtype)
    a[rng.random(a.shape) < 0.05] = np.nan
    a[1, 20:60, 30:90] = np.nan                               # a hole wider than the kernel: 0 / 0 -> NaN branch
    for propagate in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = nan_gaussian_filter(a, (0, 2, 2), propagate_nan=propagate)
        got = nan_gaussian_filter(torch.from_numpy(a).cuda(), (0, 2, 2), propagate_nan=propagate).cpu().numpy()
        assert _same(got, want), f"{int((~np.isclose(got, want, equal_nan=True, rtol=0, atol=0)).sum())} differ"
    assert np.isnan(want[1, 40, 60])


def _growing_wvd(scene, minutes):
    """WVD-like field: the cold blobs of the scene are MAXIMA that intensify with time (only they exceed -5)"""
    bt = scene["bt"]
    ramp = np.linspace(0.6, 1.2, bt.shape[0], dtype=np.float32)[:, None, None]
    field = ramp * np.clip(250.0 - bt, 0, None) / 3 - 8 + np.clip(250.0 - bt, None, 0) / 40
    return FakeDataArray(field.astype(np.float32), minutes=minutes)


def test_detect_growth_markers_device_resident_equals_scipy_glue(scene):
    """detect_growth_markers keeps every intermediate in HBM; the variant that runs the reference's SciPy glue on the
    host between the same device operators must give the same derivative field and the same labels.  The field is
    chosen so that every filter removes something and something survives."""
    from tobac_flow_amd.detection import _detect_growth_markers_host, detect_growth_markers
    wvd = _growing_wvd(scene, minutes=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_diff, want_labels = _detect_growth_markers_host(scene["flow"], wvd)
        got_diff, got_labels = detect_growth_markers(scene["flow"], wvd)
    want_labels, got_labels = np.asarray(want_labels), np.asarray(got_labels)
    assert want_labels.max() >= 2 and 0 < (want_diff >= 0.5).sum() < (want_diff >= 0.25).sum() < want_diff.size / 4
    assert _same(np.asarray(got_diff), np.asarray(want_diff))
    assert _same(got_labels, want_labels)


def test_detect_growth_markers_without_survivors_behaves_like_the_reference(scene):
    """When no marker lasts three time steps the reference passes SciPy an empty label range
    (analysis.py:78-86); with this SciPy that is a ValueError.  Both variants must do the same thing."""
    from tobac_flow_amd.detection import _detect_growth_markers_host, detect_growth_markers
    wvd = _growing_wvd(scene, minutes=5)
    outcome = []
    for fn in (_detect_growth_markers_host, detect_growth_markers):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                outcome.append(("ok", np.asarray(fn(scene["flow"], wvd)[1])))
            except Exception as e:                                   # noqa: BLE001 - the type is what is compared
                outcome.append(("raised", type(e)))
    assert outcome[0][0] == outcome[1][0]
    if outcome[0][0] == "raised":
        assert outcome[0][1] is outcome[1][1] is ValueError
    else:
        assert np.array_equal(outcome[0][1], outcome[1][1]) and outcome[0][1].max() == 0


@pytest.mark.parametrize("emptied_after", [None, 0, 1, 2])
def test_growth_marker_filter_in_one_pass_equals_the_three_host_stages(emptied_after):
    """detect_growth_markers filters by length, then by two masks, renumbering after each stage; the device form measures
    once and renumbers once.  Hand-made labels: 1 lasts two frames (and touches both masks), 2 lasts four and misses the
    first mask, 3 lasts four, touches the first and misses the second, 4 and 5 pass everything.  The variants leave nothing
    after stage 0, 1 or 2: both forms must then return equal arrays or raise the same exception type."""
    import torch
    from tobac_flow_amd.analysis import filter_labels_by_length, filter_labels_by_mask
    from tobac_flow_amd.detection import _growth_marker_filter_dev
    lab = np.zeros((5, 4, 6), np.int32)
    lab[0:2, 0, 0:2] = 1
    lab[0:4, 1, 0:3] = 2
    lab[1:5, 2, 1:4] = 3
    lab[0:5, 3, 0:2] = 4
    lab[1:4, 3, 4:6] = 5
    filtered = np.zeros(lab.shape, np.float64)
    wvd = np.full(lab.shape, -10.0, np.float32)
    filtered[1, 0, 0] = filtered[2, 2, 2] = filtered[4, 3, 1] = 0.5
    filtered[3, 3, 5] = 2.0
    wvd[0, 0, 1] = wvd[3, 1, 0] = wvd[0, 3, 0] = -5.0
    wvd[2, 3, 4] = 1.0
    if emptied_after == 0:
        lab[2:] = 0                                                     # nothing lasts three frames
    elif emptied_after == 1:
        filtered[lab > 1] = 0.25                                        # only the short label touches filtered >= 0.5
    elif emptied_after == 2:
        wvd[lab > 3] = -5.5                                             # labels 4 and 5 miss wvd >= -5

    def host():
        out = filter_labels_by_length(lab.copy(), 3)
        out = filter_labels_by_mask(out, filtered >= 0.5)
        return filter_labels_by_mask(out, wvd >= -5)

    def device():
        return _growth_marker_filter_dev(*(torch.from_numpy(a).cuda() for a in (lab, filtered, wvd))).cpu().numpy()

    outcome = []
    for fn in (host, device):
        try:
            outcome.append(("ok", fn()))
        except Exception as e:                                       # noqa: BLE001 - the type is what is compared
            outcome.append(("raised", type(e)))
    assert outcome[0][0] == outcome[1][0]
    if outcome[0][0] == "raised":
        assert outcome[0][1] is outcome[1][1] and emptied_after in (0, 1)
    else:
        assert np.array_equal(outcome[0][1], outcome[1][1])
        assert outcome[0][1].max() == (2 if emptied_after is None else 0)
        if emptied_after is None:
            assert np.array_equal(outcome[0][1], (lab == 4) + 2 * (lab == 5))


def test_peak_local_max_2d_on_device_equals_scikit_image_goldens():
    """GPU candidate mask + shared selection against scikit-image 0.18.3's own output (tests/golden/peak_local_max_skimage.npz)"""
    import os
    import torch
    from tobac_flow_amd import ndimage_dev as nd
    from tobac_flow_amd.utils.peak_utils import peak_local_max
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peak_local_max_skimage.npz"))
    n = 0
    for name in z["names"]:
        img = z[f"{name}/image"]
        for d in (1, 3, 10):
            got = nd.peak_local_max_2d(torch.from_numpy(img).cuda(), d).reshape(-1, 2)
            host = np.asarray(peak_local_max(img, min_distance=d)).reshape(-1, 2)
            assert np.array_equal(got, host), f"{name} d={d}: device differs from the host function"
            if str(name) != "quantised":                      # tie order depends on the numpy version (see test_host_logic)
                assert np.array_equal(got, z[f"{name}/peaks_d{d}"]), f"{name} d={d}: differs from scikit-image"
            n += len(got)
    assert n > 4000


@pytest.mark.parametrize("direction", ["negative", "positive"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_peak_filter_device_path_equals_host_path(scene, direction, dtype):
    """get_peak_filter (detection.py:149-168) on a device tensor against the numpy / SciPy path, including a frame with a
    NaN (numpy's min makes the threshold NaN: no peak at all) and a constant frame; a peak-free frame gets the corner
    SciPy's distance transform produces when there is no background."""
    import torch
    from tobac_flow_amd.detection import get_peak_filter
    field = (-scene["bt"]).astype(dtype).copy()
    field[2, 30, 40] = np.nan
    field[4] = 1.5
    for sigma in (2, 0.5):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = get_peak_filter(field, sigma=sigma, direction=direction)
        got = get_peak_filter(torch.from_numpy(field).cuda(), sigma=sigma, direction=direction)
        assert isinstance(got, torch.Tensor) and _same(got.cpu().numpy(), want)
        corner = np.zeros(field.shape[1:], bool)
        yy, xx = np.mgrid[0:field.shape[1], 0:field.shape[2]]
        corner[(yy + 1) ** 2 + xx ** 2 < 25] = True
        assert np.array_equal(want[2].astype(bool), corner) and np.array_equal(want[4].astype(bool), corner)
        assert want[0].sum() > corner.sum()                    # ordinary frames do have peaks


@pytest.mark.parametrize("use_wvd", [True, False])
def test_combined_filters_device_resident_equals_host_recipe(scene, use_wvd):
    """get_combined_filters (detection.py:301-354) with GPU tensors: curvature + peak filters, semi-Lagrangian `any`
    over t+-1, fill holes, opening, SWD ramp -- nothing but the candidate peaks leaves HBM."""
    import torch
    from tobac_flow_amd.detection import get_combined_filters
    bt = scene["bt"].astype(np.float32)
    wvd = ((250.0 - bt) / 8 - 6).astype(np.float32)
    swd = ((bt - 214.0) / 8).astype(np.float32)                     # spans the 2.5 ... 7.5 ramp
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = get_combined_filters(scene["flow"], bt, wvd, swd, use_wvd=use_wvd)
    got = get_combined_filters(scene["flow"], torch.from_numpy(bt).cuda(), torch.from_numpy(wvd).cuda(),
                               torch.from_numpy(swd).cuda(), use_wvd=use_wvd)
    assert isinstance(got, torch.Tensor) and _same(got.cpu().numpy(), np.asarray(want))
    frac = (np.asarray(want) > 0).mean()
    assert 0.01 < frac < 0.9 and len(np.unique(np.asarray(want))) > 10   # a non-trivial, graded filter


def _core_scene(minutes, scale=1.0, T=8):
    """Intensifying cold blobs: BT falls inside them, WVD rises above -5 there, SWD is small there"""
    import tobac_flow_amd.flow as tf
    rng = np.random.default_rng(42)
    bt0 = blob_sequence(rng, T, 96, 120, n_blobs=5, vmax=2.0, noise=0.5)
    flow = tf.create_flow(bt0, smoothing_passes=1, interp_method="cubic")
    ramp = np.linspace(0.5, 1.4, T, dtype=np.float32)[:, None, None]
    cold = np.clip(250.0 - bt0, 0, None)
    bt = FakeDataArray((290.0 - ramp * cold * scale).astype(np.float32), minutes=minutes)
    wvd = FakeDataArray((ramp * cold * scale / 6 - 8).astype(np.float32), minutes=minutes)
    swd = FakeDataArray(np.clip(8 - cold / 8, 0, None).astype(np.float32), minutes=minutes)
    return flow, bt, wvd, swd


@pytest.mark.parametrize("minutes,use_wvd", [(2, True), (5, True), (2, False)])
def test_detect_cores_device_resident_equals_host_glue_and_meets_its_own_criteria(minutes, use_wvd, capsys):
    """detect_cores (detection.py:372-482).  (1) The variant that keeps everything up to the labels in HBM equals the
    variant with the reference's numpy / SciPy glue.  (2) The criteria of the recipe, recomputed independently on the
    result: every core lasts more than min_length steps, touches WVD > -5 and cools by >= 0.5 K / min over some
    min_length-step interval of its per-step mean BT."""
    from tobac_flow_amd.detection import _detect_cores_host, detect_cores
    flow, bt, wvd, swd = _core_scene(minutes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np.asarray(_detect_cores_host(flow, bt, wvd, swd, use_wvd=use_wvd))
        host_log = capsys.readouterr().out
        got = np.asarray(detect_cores(flow, bt, wvd, swd, use_wvd=use_wvd))
        dev_log = capsys.readouterr().out
    assert _same(got, want) and host_log == dev_log               # same labels and the same progress report
    n = int(want.max())
    assert n >= 1 and set(np.unique(want)) == set(range(n + 1))   # dense labels
    btv, wv = np.asarray(bt), np.asarray(wvd)
    for k in range(1, n + 1):
        where = want == k
        steps = np.nonzero(where.any((1, 2)))[0]
        assert steps[-1] - steps[0] + 1 > 3 and (wv[where] > -5).any()
        mean_bt = np.array([np.nanmean(btv[t][where[t]]) for t in steps])
        drop = (mean_bt[:-3] - mean_bt[3:]) / (3.0 * minutes)
        assert np.nanmax(drop) >= 0.5 - 1e-4, (k, drop)
    assert "Initial core count" in host_log
    # device-resident form (round 5): DeviceField in (tensor + time coordinate) -> tensor out, the same labels
    import torch
    from tobac_flow_amd.detection import DeviceField
    tt = np.asarray(bt.t.data)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = detect_cores(flow, *(DeviceField(torch.from_numpy(np.asarray(x)).cuda(), tt) for x in (bt, wvd, swd)), use_wvd=use_wvd)
    capsys.readouterr()
    assert isinstance(dev, torch.Tensor) and _same(dev.cpu().numpy(), want)


def test_core_cooling_statistics_on_the_device_equal_the_host_statistics():
    """The last stage of detect_cores (detection.py:434-482) with its volume passes on the device: per (core, step) label the
    core it belongs to, its mean BT and its time; then the reference's own host reduction over a core's steps.  The labels
    equal the host form's; the per-step means agree with numpy's float32 nanmean to a few float32 ulps (the host value
    depends on the order an unstable argsort leaves the values in; the device value is the correctly rounded mean)."""
    import torch
    from tobac_flow_amd import label as _label
    from tobac_flow_amd.analysis import _label_stats
    from tobac_flow_amd.detection import _core_cooling_filter, _core_cooling_filter_dev
    from tobac_flow_amd.utils import labeled_comprehension, slice_labels
    rng = np.random.default_rng(12)
    T, H, W = 9, 60, 80
    core = np.zeros((T, H, W), np.int32)
    core[0:7, 5:20, 5:25] = 1                      # cools fast
    core[2:9, 30:50, 10:30] = 2                    # cools slowly
    core[1:4, 10:15, 50:60] = 3                    # too short for a min_length-step difference
    core[3:9, 40:55, 50:75] = 4                    # holds NaN values
    core[0:9:2, 25:28, 40:44] = 5                  # present at every other step only
    bt = 250 + rng.normal(size=(T, H, W)).astype(np.float32)
    for k, rate in ((1, 9.0), (2, 1.0), (3, 9.0), (4, 8.0), (5, 7.0)):
        bt -= (core == k) * (rate * np.arange(T, dtype=np.float32)[:, None, None])
    bt[5, 41:44, 51:60] = np.nan
    bt[6][core[6] == 4] = np.nan                   # a whole step of core 4 without a value
    fa = FakeDataArray(bt.astype(np.float32), minutes=5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = _core_cooling_filter(core.copy(), fa, 3)
        got = _core_cooling_filter_dev(torch.from_numpy(core).cuda(), torch.from_numpy(np.asarray(fa)).cuda(), np.asarray(fa.t.data), 3)
        assert np.array_equal(got.cpu().numpy(), want) and 1 <= want.max() < 5
        step = slice_labels(core)
        host_mean = labeled_comprehension(np.asarray(fa), step, np.nanmean, default=np.nan)
    dev_mean = _label_stats(torch.from_numpy(step.astype(np.int32)).cuda(), torch.from_numpy(np.asarray(fa)).cuda(), None, np.float64)[0].astype(np.float32)
    assert np.array_equal(np.isnan(dev_mean), np.isnan(host_mean)) and np.isnan(host_mean).sum() == 1
    ok = ~np.isnan(host_mean)
    assert np.max(np.abs(dev_mean[ok] - host_mean[ok]) / np.abs(host_mean[ok])) < 4 * np.finfo(np.float32).eps


def test_detect_cores_without_candidates_behaves_like_the_reference():
    """Sampled every 15 minutes the same scene grows too slowly per minute: no marker at all.  The reference then hands
    ndi.labeled_comprehension an empty label range in its statistics stage (detection.py:434-446), which this SciPy
    rejects with a ValueError -- a window without growing cloud makes detect_cores raise.  Both variants do the same."""
    from tobac_flow_amd.detection import _detect_cores_host, detect_cores
    flow, bt, wvd, swd = _core_scene(15)
    outcome = []
    for fn in (_detect_cores_host, detect_cores):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                outcome.append(("ok", np.asarray(fn(flow, bt, wvd, swd))))
            except Exception as e:                                   # noqa: BLE001 - the type is what is compared
                outcome.append(("raised", type(e)))
    assert outcome[0][0] == outcome[1][0]
    if outcome[0][0] == "raised":
        assert outcome[0][1] is outcome[1][1] is ValueError
    else:
        assert outcome[0][1].max() == 0 and np.array_equal(outcome[0][1], outcome[1][1])


def test_anvil_seeds_equal_the_scipy_recipe():
    """tools/synth.anvil_seeds (what bench.py computes inside its timed region: SURVEY 8(d)'s marker recipe through
    tf_linearise, tf_field_masks, tf_binary_morph, tf_label, tf_merge_seeds) against the same recipe in numpy / SciPy
    (detection.py:547-561, 590-617): a stack with a NaN patch, erode distances 1 and 2."""
    import torch
    from tobac_flow_amd.utils import linearise_field
    from tools.synth import anvil_seeds
    rng = np.random.default_rng(12)
    bt = (ndi.gaussian_filter(rng.normal(size=(6, 90, 132)), (0.7, 4, 4)) * 120 + 262).astype(np.float32)
    bt[2, 20:31, 40:57] = np.nan
    s = ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None].astype(bool)
    for erode in (1, 2):
        lin, seeds = anvil_seeds(torch.from_numpy(bt).cuda(), 270.0, 250.0, erode_distance=erode)
        want_lin = linearise_field(bt, 270, 250).astype(np.float32)
        assert np.array_equal(lin.cpu().numpy(), want_lin, equal_nan=True)
        want = ndi.label(ndi.binary_erosion(want_lin >= 1, structure=s))[0].astype(np.int32)
        nan = np.isnan(want_lin)
        bg = ndi.binary_erosion(np.logical_or(want_lin <= 0, nan), structure=np.ones([3, 3, 3]), iterations=erode, border_value=1)
        bg[nan] = True
        want[bg] = -1
        assert (want > 0).any() and (want == -1).any() and (want == 0).any()
        assert np.array_equal(seeds.cpu().numpy(), want)
