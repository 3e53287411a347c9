"""GPU parity tests: the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Integer / label work is compared bit-exactly; float32 / float64 stencils that follow the oracle's
operation order are compared bit-exactly too (the library is built with -ffp-contract=off);
Farnebaeck with OpenCV's default parameters is compared bit for bit since round 4 (sequential row sums, k_fb_iter);
other parameter sets take the generic kernels and stay within the north-star tolerance of 1e-4 px.
"""
import numpy as np
import pytest
import scipy.ndimage as ndi

from helpers import _eq, blob_sequence, rand_field, rand_flow, seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tf():
    import tobac_flow_amd.flow as flow
    return flow


# ----------------------------------------------------------------------------- convolve / sobel
@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
@pytest.mark.parametrize("direction", [None, "uphill", "downhill"])
@pytest.mark.parametrize("dtype", [None, np.float32])
def test_sobel_matches_oracle(tf, method, direction, dtype):
    from oracle import np_ops
    rng = np.random.default_rng(7)
    shape = (4, 37, 53)
    data = rand_field(rng, shape, nan_frac=0.01)
    fwd, bwd = rand_flow(rng, shape, 1.5), rand_flow(rng, shape, 1.5)
    got = tf.Flow(fwd, bwd).sobel(data, method=method, dtype=dtype, direction=direction)
    want = np_ops.sobel(data, fwd, bwd, method=method, dtype=dtype, direction=direction)
    _eq(got, want)


def test_sobel_reference_known_answer(tf):
    """reference tests/test_detection.py:36-60 (zero flow, T = 1, cubic, uphill)"""
    field = np.zeros([1, 5, 5], np.float32)
    field[:, 3:] = 1
    z = np.zeros([1, 5, 5, 2], np.float32)
    edges = tf.Flow(z, z).sobel(field, direction="uphill", method="cubic")
    assert edges.dtype == np.float64
    assert np.all(edges[:, 2] > 0) and np.all(edges[:, :2] == 0) and np.all(edges[:, 3:] == 0)


@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
def test_convolve_stack_nanmean_diff(tf, method):
    from oracle import np_ops
    rng = np.random.default_rng(11)
    shape = (5, 33, 41)
    data = rand_field(rng, shape, nan_frac=0.02)
    fwd, bwd = rand_flow(rng, shape, 2.0), rand_flow(rng, shape, 2.0)
    fl = tf.Flow(fwd, bwd)
    for conn in (1, 2):
        st = ndi.generate_binary_structure(3, conn)
        _eq(fl.convolve(data, structure=st, method=method), np_ops.convolve(data, fwd, bwd, st, method))
    import tobac_flow_amd.detection as det
    s_struct = ndi.generate_binary_structure(3, 1)
    s_struct[0] = 0
    s_struct[2] = 0
    got = fl.convolve(data, structure=s_struct, func=det._nanmean0, method=method)
    want = np_ops.convolve(data, fwd, bwd, s_struct, method, func=lambda x: np.nanmean(x, 0))
    _eq(got, want)
    t_struct = np.zeros([3, 3, 3])
    t_struct[:, 1, 1] = 1
    got = fl.convolve(data, structure=t_struct, func=det._nanmean0, method=method)
    with np.errstate(all="ignore"):
        want = np_ops.convolve(data, fwd, bwd, t_struct, method, func=lambda x: np.nanmean(x, 0))
    _eq(got, want)
    _eq(fl.diff(data, method=method), np_ops.diff(data, fwd, bwd, method))


def test_convolve_python_callable_fallback(tf):
    from oracle import np_ops
    rng = np.random.default_rng(12)
    shape = (4, 20, 24)
    data = rand_field(rng, shape)
    fwd, bwd = rand_flow(rng, shape, 1.0), rand_flow(rng, shape, 1.0)
    f = lambda x: np.nanmax(x, 0)  # noqa: E731  (not a tagged function -> host reduction)
    with np.errstate(all="ignore"):
        _eq(tf.Flow(fwd, bwd).convolve(data, func=f), np_ops.convolve(data, fwd, bwd, func=f))


def test_convolve_int_labels_nearest_and_any(tf):
    from functools import partial
    from oracle import np_ops
    rng = np.random.default_rng(13)
    shape = (4, 30, 36)
    labels = ndi.label(rand_field(rng, shape) > 0.05)[0].astype(np.int32)
    fwd, bwd = rand_flow(rng, shape, 2.0), rand_flow(rng, shape, 2.0)
    fl = tf.Flow(fwd, bwd)
    st = ndi.generate_binary_structure(3, 1) * np.array([1, 0, 1])[:, None, None]
    got = fl.convolve(labels, method="nearest", dtype=np.int32, structure=st, fill_value=0)
    want = np_ops.convolve(labels, fwd, bwd, st, "nearest", np.int32, 0)
    _eq(got, want)
    t_struct = np.zeros([3, 3, 3], bool)
    t_struct[:, 1, 1] = True
    m = (labels > 0).astype(int)
    got = fl.convolve(m, structure=t_struct, method="nearest", fill_value=False, dtype=np.int32,
                      func=partial(np.any, axis=0))
    want = np_ops.convolve(m.astype(np.int32), fwd, bwd, t_struct, "nearest", np.int32, False,
                           func=partial(np.any, axis=0))
    _eq(got, want)


# ----------------------------------------------------------------------------- warp / smoothing / to_8bit
def test_warp_flow_reference_known_answers(tf):
    """reference tests/test_flow.py:94-161"""
    arr = np.arange(15, dtype=np.float32).reshape(3, 5)
    fl = np.zeros(arr.shape + (2,), np.float32)
    w = tf.warp_flow(arr, fl)
    ok = ~np.isnan(w)
    assert np.all(w[ok] == arr[ok])
    fl[..., 0] = 0.5
    w = tf.warp_flow(arr, fl)[:, :-1]
    ok = ~np.isnan(w)
    assert np.all(w[ok] == ((arr[:, 1:] + arr[:, :-1])[ok] * 0.5))


@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
def test_warp_and_smooth_match_oracle(tf, method):
    from oracle import np_ops
    rng = np.random.default_rng(3)
    img = rand_field(rng, (1, 45, 57))[0]
    f, b = rand_flow(rng, (1, 45, 57), 2.0)[0], rand_flow(rng, (1, 45, 57), 2.0)[0]
    _eq(tf.warp_flow(img, f, method), np_ops.warp_flow_single(img, f, method))
    gf, gb = tf.smooth_flow_step(f, b, method)
    wf, wb = np_ops.smooth_flow_step(f, b, method)
    _eq(gf, wf)
    _eq(gb, wb)


def test_smooth_flow_reference_known_answers(tf):
    """reference tests/test_flow.py:165-194"""
    z, one = np.zeros([3, 5, 2], np.float32), np.ones([3, 5, 2], np.float32)
    assert np.all(np.stack(list(tf.smooth_flow_step(z, z))) == 0)
    f, b = tf.smooth_flow_step(one, -one)
    assert np.all(f == 1) and np.all(b == -1)
    f, b = tf.smooth_flow_step(one, z)
    assert np.all(f[:1, :3] == 0.5) and np.all(b[:2, :4] == -0.5)


def test_to8bit_pair_matches_oracle(tf):
    from oracle import np_ops
    from tobac_flow_amd import _lib
    from tobac_flow_amd.utils.normalisation_utils import to_8bit_pair_dev
    rng = np.random.default_rng(5)
    for case in range(4):
        pair = blob_sequence(rng, 2, 67, 91)
        if case == 1:
            pair[0, 10:20, 30:50] = np.nan
            pair[1, 15:30, 40:45] = np.nan
        if case == 2:
            pair[:] = 250.0
        if case == 3:
            pair[:] = np.nan
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = np_ops.to_8bit(np_ops.linear_norm(pair.copy()), 0, 1)
        a, b = to_8bit_pair_dev(_lib.to_dev(pair[0]), _lib.to_dev(pair[1]))
        _eq(a.cpu().numpy(), want[0])
        _eq(b.cpu().numpy(), want[1])


# ----------------------------------------------------------------------------- Farnebaeck
def _oracle_farneback(a, b):
    import ctypes
    from oracle import _lib as ol
    L = ol.lib()
    h, w = a.shape
    out = np.zeros((h, w, 2), np.float32)
    L.oracle_farneback.restype = ctypes.c_int
    L.oracle_farneback(ol.ptr(np.ascontiguousarray(a), ctypes.c_uint8), ol.ptr(np.ascontiguousarray(b), ctypes.c_uint8),
                       h, w, ol.ptr(out, ctypes.c_float), 5, ctypes.c_double(0.5), 13, 10, 5, ctypes.c_double(1.1))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (16, 64), (17, 65), (96, 128), (150, 250), (333, 517), (700, 1100)])
def test_farneback_blur_and_polynomial_expansion_are_bit_identical_to_the_oracle(tf, shape):
    """Stage level (tf_farneback_expansion, round 4): the 3 x 3 Gaussian of the uint8 frame and its polynomial expansion
    (cv2 FarnebackPolyExp, n = 5, sigma = 1.1) as the full-resolution pyramid level computes them, against the oracle's
    restatement, every coefficient bit for bit.  (The expansion multiplies by four entries of inv(G): the library inverts G
    by the oracle's elimination -- a closed-form block inverse differed in the last digits and flipped the float rounding of
    one coefficient in ~10^5, which the running column sums of the iteration then carried down the image.)"""
    import ctypes
    import torch
    from oracle import _lib as ol
    from tobac_flow_amd import _lib
    from tobac_flow_amd.utils.flow_utils import FarnebackFlow
    Lo, L = ol.lib(), _lib.lib()
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    img = ndi.gaussian_filter(rng.normal(size=(shape[0] + 8, shape[1] + 8)), 2.0)[4:-4, 4:-4]
    img = np.ascontiguousarray(((img - img.min()) / (np.ptp(img) + 1e-9) * 255).astype(np.uint8))
    h, w = img.shape
    f = img.astype(np.float32)
    want_blur = np.zeros_like(f)
    Lo.oracle_gaussian_blur(ol.ptr(f, ctypes.c_float), h, w, 3, ctypes.c_double(0.0), ol.ptr(want_blur, ctypes.c_float))
    want = np.zeros((h, w, 5), np.float32)
    Lo.oracle_poly_exp(ol.ptr(want_blur, ctypes.c_float), h, w, ol.ptr(want, ctypes.c_float), 5, ctypes.c_double(1.1))
    d_img = torch.from_numpy(img).cuda()
    d_blur = torch.empty((h, w), dtype=torch.float32, device="cuda")
    d_R = torch.empty(5 * h * w, dtype=torch.float32, device="cuda")
    m = FarnebackFlow()
    _lib.check(L.tf_farneback_expansion(_lib.ptr(d_img), h, w, ctypes.byref(m.params), _lib.ptr(d_blur), _lib.ptr(d_R), _lib.stream_ptr()), "tf_farneback_expansion")
    torch.cuda.synchronize()
    R = d_R.cpu().numpy()
    got = np.concatenate([R[:4 * h * w].reshape(h, w, 4), R[4 * h * w:].reshape(h, w, 1)], -1)
    assert np.array_equal(d_blur.cpu().numpy(), want_blur)
    assert np.array_equal(got, want), int((got != want).sum())
    d_R2 = torch.empty_like(d_R)                                        # blur_out = NULL: the library's own temporary
    _lib.check(L.tf_farneback_expansion(_lib.ptr(d_img), h, w, ctypes.byref(m.params), None, _lib.ptr(d_R2), _lib.stream_ptr()), "tf_farneback_expansion")
    assert torch.equal(d_R, d_R2)


@pytest.mark.parametrize("shape", [(96, 128), (150, 250), (333, 517)])
def test_farneback_matches_oracle(tf, shape):
    from oracle import np_ops
    rng = np.random.default_rng(shape[0])
    seq = blob_sequence(rng, 2, *shape, n_blobs=8)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p8 = np_ops.to_8bit(np_ops.linear_norm(seq.copy()), 0, 1)
    model = tf.select_of_model("Farneback")
    f, b = tf.calculate_flow_frame(p8[0], p8[1], model)
    wf, wb = _oracle_farneback(p8[0], p8[1]), _oracle_farneback(p8[1], p8[0])
    assert f.dtype == np.float32 and f.shape == shape + (2,)
    assert np.array_equal(f, wf), (int((f != wf).sum()), np.max(np.abs(f - wf)))          # bit for bit (round 4)
    assert np.array_equal(b, wb), (int((b != wb).sum()), np.max(np.abs(b - wb)))


def test_farneback_recovers_translation(tf):
    rng = np.random.default_rng(0)
    img = ndi.gaussian_filter(rng.normal(size=(200, 260)), 4)
    img = ((img - img.min()) / (img.max() - img.min()) * 255).astype(np.uint8)
    f, b = tf.calculate_flow_frame(img, np.roll(img, (2, -3), (0, 1)), tf.select_of_model("Farneback"))
    c = f[50:150, 60:200].mean((0, 1))
    assert abs(c[0] + 3) < 0.05 and abs(c[1] - 2) < 0.05
    c = b[50:150, 60:200].mean((0, 1))
    assert abs(c[0] - 3) < 0.05 and abs(c[1] + 2) < 0.05


def test_create_flow_matches_oracle_pipeline(tf):
    from oracle import np_ops
    import warnings
    rng = np.random.default_rng(21)
    seq = blob_sequence(rng, 4, 120, 160, n_blobs=6)
    seq[1, 30:40, 50:70] = np.nan
    fl = tf.create_flow(seq, model="Farneback", smoothing_passes=1, interp_method="cubic")
    T = seq.shape[0]
    fw = np.full(seq.shape + (2,), np.nan, np.float32)
    bw = np.full(seq.shape + (2,), np.nan, np.float32)
    for i in range(T - 1):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p8 = np_ops.to_8bit(np_ops.linear_norm(seq[i:i + 2].copy()), 0, 1)
        f, b = _oracle_farneback(p8[0], p8[1]), _oracle_farneback(p8[1], p8[0])
        f, b = np_ops.smooth_flow_step(f, b, "cubic")
        fw[i], bw[i + 1] = f, b
    fw[-1] = -bw[-1]
    bw[0] = -fw[0]
    fw, bw = np.clip(fw, -20, 20), np.clip(bw, -20, 20)
    assert fl.shape == seq.shape
    assert np.array_equal(fl.forward_flow, fw, equal_nan=True)          # every stage bit-identical: so is the composition
    assert np.array_equal(fl.backward_flow, bw, equal_nan=True)


def test_farneback_batch_is_bit_identical_to_single_pairs(tf):
    """tf_farneback_batch (B pairs per launch, strided inputs / outputs) against tf_farneback_pair one pair at a time:
    the same kernels on the same data, so the flows must be identical bit for bit, both directions."""
    import torch
    from tobac_flow_amd.utils.flow_utils import FarnebackFlow
    rng = np.random.default_rng(17)
    B, H, W = 5, 150, 270
    base = ndi.gaussian_filter(rng.normal(size=(H + 2 * B, W + 2 * B)), 2.5)
    base = ((base - base.min()) / np.ptp(base) * 255).astype(np.uint8)
    frames = np.stack([base[i:i + H, 2 * B - i:2 * B - i + W] for i in range(B + 1)])          # drifting content
    fr = torch.from_numpy(frames).cuda()
    model = FarnebackFlow()
    fwd = torch.full((B + 1, H, W, 2), float("nan"), dtype=torch.float32, device="cuda")
    bwd = torch.full_like(fwd, float("nan"))
    model.calc_batch_dev(fr[:-1].contiguous(), fr[1:].contiguous(), fwd[:B], bwd[1:])          # views into bigger arrays
    for i in range(B):
        f1, b1 = model.calc_pair_dev(fr[i], fr[i + 1])
        assert torch.equal(fwd[i], f1) and torch.equal(bwd[i + 1], b1), f"pair {i}"
    assert torch.isnan(fwd[B]).all() and torch.isnan(bwd[0]).all()                              # untouched slots stay untouched
    assert float(fwd[:B].abs().max()) > 0.5


# ----------------------------------------------------------------------------- watershed
EXACT_VS_REFERENCE = ["A_cont_c1", "B_cont_mask_c2", "B_cont_mask_c3", "D_anvil_like_c1", "F_zero_flow_c1", "G_big_flow_c1"]


@pytest.mark.parametrize("name", EXACT_VS_REFERENCE)
def test_watershed_golden_bit_exact(tf, golden_ws, name):
    c = golden_ws[name]
    got = tf.watershed(c["fwd"], c["bwd"], c["field"], c["markers"], mask=c.get("mask"), connectivity=int(c["conn"]))
    assert got.dtype == np.int32
    assert np.array_equal(got, c["labels"]), f"{int((got != c['labels']).sum())} px differ from the reference"


@pytest.mark.parametrize("name,final_depth", [("C_quant4_c1", 3), ("C_quant32_c1", 6), ("E_const_plateau_c1", 3)])
def test_watershed_tie_heavy_goldens(tf, golden_ws, name, final_depth):
    """Tie-heavy inputs in the raster-order mode (on_ambiguous="warn": the opt-out since round 4; the default reproduces the
    reference's heap order, tests/test_gpu_reference_order.py).  The library deepens the chain comparison on its own
    (C_quant32 needs six levels) and REPORTS the pixels whose label hangs on the order of equal-valued markers -- the one
    thing the reference decides by the internal state of its heap.  Checked here: the labels equal the sequential flood under
    the idealised marker order bit for bit; every pixel that differs from the reference's own output is reported; and
    the report is exactly the one the numpy model of the contract computes (tests/ws_parallel_model.py)."""
    import sys, os, warnings
    sys.path.insert(0, os.path.dirname(__file__))
    import ws_parallel_model as M
    from oracle import ws_oracle
    from tobac_flow_amd.watershed import WatershedAmbiguityWarning
    c = golden_ws[name]
    conn = int(c["conn"])
    with pytest.warns(WatershedAmbiguityWarning):
        got, rep = tf.watershed(c["fwd"], c["bwd"], c["field"], c["markers"], mask=c.get("mask"), connectivity=conn,
                                return_ambiguous=True, on_ambiguous="warn")
    ideal = ws_oracle.watershed(c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"), conn, tie_mode=1)
    assert np.array_equal(got, ideal), f"{int((got != ideal).sum())} px differ from the idealised-order oracle"
    differs = got != c["labels"]
    assert not (differs & ((rep & 1) == 0)).any(), "a pixel differs from the reference without being reported"
    assert not (rep & 4).any()                                   # nothing left by the depth cut-off
    want, info = M.run(c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"), conn, depth=final_depth)
    assert np.array_equal(got, want) and np.array_equal(rep, info["report"])
    assert int(differs.sum()) == {"C_quant4_c1": 21, "C_quant32_c1": 0, "E_const_plateau_c1": 37}[name]


def test_watershed_reports_the_depth_it_needed_and_refuses_a_silent_cut_off(tf, golden_ws):
    """Nested exact plateaus (32-level quantised field): three chain levels are not enough.  With room to deepen the
    call ends at depth 6 with the reference's labels; confined to depth 3 it raises instead of returning labels that
    differ from the reference (38 px) with a clean return code -- and `on_ambiguous="ignore"` still warns."""
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import (WatershedAmbiguityWarning, WatershedDepthError, neighbour_offsets,
                                          watershed_dev)
    c = golden_ws["C_quant32_c1"]
    fw, bw = _lib.to_dev(c["fwd"], torch.float32), _lib.to_dev(c["bwd"], torch.float32)
    f, m = _lib.to_dev(c["field"], torch.float32), _lib.to_dev(c["markers"], torch.int32)
    nbr = neighbour_offsets(int(c["conn"]), 3)
    for expect_conflict in (None, True, False):
        st = {}
        lab = watershed_dev(fw, bw, f, m, None, nbr, 3, st, expect_conflict=expect_conflict, on_ambiguous="ignore")
        assert st["chain_depth"] == 6 and st["depth_origins"] == 0
        assert np.array_equal(lab.cpu().numpy(), c["labels"])
    with pytest.raises(WatershedDepthError):
        watershed_dev(fw, bw, f, m, None, nbr, 3, max_chain_depth=3)
    st = {}
    with pytest.warns(WatershedAmbiguityWarning, match="still tie at chain depth 3"):
        lab, rep = watershed_dev(fw, bw, f, m, None, nbr, 3, st, max_chain_depth=3, on_ambiguous="ignore",
                                 return_ambiguous=True)
    lab, rep = lab.cpu().numpy(), rep.cpu().numpy()
    assert st["depth_origins"] > 0 and (rep & 4).any()
    differs = lab != c["labels"]
    assert differs.sum() == 38 and not (differs & ((rep & 1) == 0)).any()
    # the C ABI itself: TF_EDEPTH, never 0, when the cut-off decided a label
    L = _lib.lib()
    T, H, W = c["field"].shape
    ws = torch.empty(L.tf_watershed_workspace_bytes(T, H, W, len(nbr), 3, 0), dtype=torch.uint8, device="cuda")
    out = torch.empty((T, H, W), dtype=torch.int32, device="cuda")
    rc = L.tf_watershed(_lib.ptr(f), _lib.ptr(m), None, _lib.ptr(fw), _lib.ptr(bw), T, H, W, nbr.ctypes.data_as(_lib._P),
                        len(nbr), 3, _lib.ptr(out), _lib.ptr(ws), ws.numel(), None, None)
    assert rc == -5 and b"still tie at chain depth 3" in L.tf_last_error()


@pytest.mark.parametrize("name", ["A_cont_c1", "B_cont_mask_c2", "B_cont_mask_c3", "D_anvil_like_c1", "F_zero_flow_c1",
                                  "G_big_flow_c1"])
def test_watershed_clean_return_means_no_tie_break_mattered(tf, golden_ws, name):
    """TF_OK <=> nothing was decided by a last-resort rule: no warning, an all-zero report, the reference's labels."""
    import warnings
    c = golden_ws[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, rep = tf.watershed(c["fwd"], c["bwd"], c["field"], c["markers"], mask=c.get("mask"),
                                connectivity=int(c["conn"]), return_ambiguous=True, on_ambiguous="raise")
    assert not rep.any() and np.array_equal(got, c["labels"])


@pytest.mark.parametrize("seed", range(6))
def test_watershed_random_vs_oracle(tf, seed):
    from oracle import ws_oracle
    rng = np.random.default_rng(100 + seed)
    shape = (int(rng.integers(1, 7)), int(rng.integers(20, 60)), int(rng.integers(20, 70)))
    field = rand_field(rng, shape)
    if seed % 3 == 2:
        field[rng.random(shape) < 0.02] = np.inf
    markers = seeds(rng, shape, int(rng.integers(1, 15)))
    mask = None if seed % 2 == 0 else ndi.gaussian_filter(rng.normal(size=shape), (0, 2, 2)) > -0.03
    fwd, bwd = rand_flow(rng, shape, 2.5), rand_flow(rng, shape, 2.5)
    conn = [1, 2, 3][seed % 3]
    got = tf.watershed(fwd, bwd, field, markers, mask=mask, connectivity=conn)
    want = ws_oracle.watershed(fwd, bwd, field, markers, mask, conn)
    assert np.array_equal(got, want), f"{int((got != want).sum())} px differ"


def _ws_both_paths(c_fwd, c_bwd, field, markers, mask, conn, depth):
    """Run the HIP flood with the speculative root phase (probe) and without it (TF_WS_SKIP_FAST_PATH)."""
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import neighbour_offsets, watershed_dev
    fw, bw = _lib.to_dev(c_fwd, torch.float32), _lib.to_dev(c_bwd, torch.float32)
    f, m = _lib.to_dev(field, torch.float32), _lib.to_dev(markers, torch.int32)
    k = None if mask is None else _lib.to_dev(mask).to(torch.int8)
    nbr = neighbour_offsets(conn, 3)
    out = []
    for skip in (False, True):
        st = {}
        lab = watershed_dev(fw, bw, f, m, k, nbr, depth, st, expect_conflict=skip).cpu().numpy()
        out.append((lab, st["sweeps"]))
    return out


GOLDEN_DEPTH = {"C_quant32_c1": 6}


@pytest.mark.parametrize("name", EXACT_VS_REFERENCE + ["C_quant4_c1", "C_quant32_c1", "E_const_plateau_c1"])
def test_watershed_skip_fast_path_gives_identical_labels_golden(tf, golden_ws, name):
    """The scheduling hint must never change a label: chain phases alone == root-phase fast path
    (when it is accepted) == fast path + chain phases (when it is rejected)."""
    c = golden_ws[name]
    (probe, st_p), (skip, st_s) = _ws_both_paths(c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"),
                                                 int(c["conn"]), GOLDEN_DEPTH.get(name, 3))
    assert st_p[5] in (0, 1) and st_p[1] > 0              # probed: root phase ran, conflict flag evaluated
    assert st_s[5] == -1 and st_s[1] == 0 and st_s[2] > 0  # skipped: no root phase, chain phases ran
    assert np.array_equal(probe, skip), f"{int((probe != skip).sum())} px depend on the scheduling hint"


@pytest.mark.parametrize("seed", range(6))
def test_watershed_skip_fast_path_gives_identical_labels_random(tf, seed):
    rng = np.random.default_rng(100 + seed)
    shape = (int(rng.integers(1, 7)), int(rng.integers(20, 60)), int(rng.integers(20, 70)))
    field = rand_field(rng, shape)
    if seed % 2 == 1:
        field = np.round(field * 8) / 8                    # exact plateaus: conflicts, deep chains
    markers = seeds(rng, shape, int(rng.integers(1, 15)))
    mask = None if seed % 2 == 0 else ndi.gaussian_filter(rng.normal(size=shape), (0, 2, 2)) > -0.03
    fwd, bwd = rand_flow(rng, shape, 2.5), rand_flow(rng, shape, 2.5)
    (probe, st_p), (skip, st_s) = _ws_both_paths(fwd, bwd, field, markers, mask, [1, 2, 3][seed % 3], 3)
    assert st_s[5] == -1 and st_s[1] == 0
    assert np.array_equal(probe, skip), f"{int((probe != skip).sum())} px depend on the scheduling hint"


def test_watershed_conflict_memo_schedules_but_never_changes_labels(tf, golden_ws):
    """Default path (expect_conflict=None): a shape whose probe conflicted skips the root phase on the
    following calls and probes again after _REPROBE calls."""
    import torch
    from tobac_flow_amd import _lib, watershed as wsmod
    c = golden_ws["E_const_plateau_c1"]
    fw, bw = _lib.to_dev(c["fwd"], torch.float32), _lib.to_dev(c["bwd"], torch.float32)
    f, m = _lib.to_dev(c["field"], torch.float32), _lib.to_dev(c["markers"], torch.int32)
    nbr = wsmod.neighbour_offsets(int(c["conn"]), 3)
    wsmod._conflict_memo.clear()
    flags, first = [], None
    for _ in range(wsmod._REPROBE + 3):
        st = {}
        lab = wsmod.watershed_dev(fw, bw, f, m, None, nbr, 3, st).cpu().numpy()
        first = lab if first is None else first
        assert np.array_equal(lab, first)
        flags.append(st["sweeps"][5])
    assert flags[0] == 1                                   # probe: the plateau field conflicts
    assert flags[1:1 + wsmod._REPROBE] == [-1] * wsmod._REPROBE
    assert flags[1 + wsmod._REPROBE] == 1                  # probed again


def test_watershed_errors(tf):
    z = np.zeros((2, 5, 5, 2), np.float32)
    f = np.zeros((2, 5, 5), np.float32)
    with pytest.raises(ValueError):
        tf.watershed(z, z, f, np.zeros((2, 5, 4), np.int32))
    with pytest.raises(ValueError):
        tf.watershed(z, z, f, np.zeros((2, 5, 5), np.int32), mask=np.ones((1, 5, 5), bool))
    out = tf.watershed(z, z, f, np.zeros((2, 5, 5), np.int32))       # no markers: nothing flooded
    assert out.dtype == np.int32 and not out.any()


def test_combined_edge_field_device_path_equals_numpy_path(tf):
    """detection.get_combined_edge_field: fused device kernel == the reference's numpy tail"""
    import torch
    from tobac_flow_amd.detection import get_combined_edge_field
    rng = np.random.default_rng(31)
    shape = (3, 40, 52)
    field = np.clip(rand_field(rng, shape, nan_frac=0.01) * 3, 0, 1).astype(np.float32)
    fwd, bwd = rand_flow(rng, shape, 1.5), rand_flow(rng, shape, 1.5)
    fl = tf.Flow(fwd, bwd)
    want = get_combined_edge_field(fl, field)
    assert want.dtype == np.float64
    dev = get_combined_edge_field(fl, torch.from_numpy(field).cuda())
    assert dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), want)
    dev32 = get_combined_edge_field(fl, torch.from_numpy(field).cuda(), dtype=np.float32)
    assert np.array_equal(dev32.cpu().numpy(), want.astype(np.float32))


# ----------------------------------------------------------------------------- flow-aware labelling
@pytest.mark.parametrize("overlap,absolute_overlap", [(0.0, 0), (0.5, 4), (0.9, 1), (0.2, 12)])
def test_flow_label_matches_oracle(tf, overlap, absolute_overlap):
    from oracle import np_label
    rng = np.random.default_rng(int(overlap * 10) + absolute_overlap)
    shape = (6, 48, 60)
    mask = ndi.gaussian_filter(rng.normal(size=shape), (0.5, 1.5, 1.5)) > 0.12
    fwd, bwd = rand_flow(rng, shape, 2.0), rand_flow(rng, shape, 2.0)
    fl = tf.Flow(fwd, bwd)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = fl.label(mask, overlap=overlap, absolute_overlap=absolute_overlap)
    want = np_label.flow_label(fwd, bwd, mask, overlap=overlap, absolute_overlap=absolute_overlap)
    assert got.dtype == np.int32 and np.array_equal(got, want), f"{int((got != want).sum())} px differ"


def test_flow_link_overlap_matches_oracle(tf):
    from oracle import np_label
    from tobac_flow_amd.utils.label_utils import make_step_labels
    rng = np.random.default_rng(77)
    shape = (5, 40, 44)
    lab3 = ndi.label(ndi.gaussian_filter(rng.normal(size=shape), (1, 2, 2)) > 0.05)[0].astype(np.int32)
    step = make_step_labels(lab3).astype(np.int32)
    fwd, bwd = rand_flow(rng, shape, 1.5), rand_flow(rng, shape, 1.5)
    got = tf.Flow(fwd, bwd).link_overlap(step, overlap=0.5, absolute_overlap=5)
    want = np_label.flow_link_overlap(fwd, bwd, step, overlap=0.5, absolute_overlap=5)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- flow API scenarios of the reference's tests
def _reference_blob(tf):
    xx, yy = np.meshgrid(np.arange(15), np.arange(10))
    return tf.to_8bit((7 ** 2 - (xx - 7) ** 2) * (4.5 ** 2 - (yy - 4.5) ** 2))


def test_calculate_flow_and_create_flow_agree_like_in_the_reference_tests(tf):
    """tests/test_flow.py:298-361 with the model that exists here: calculate_flow returns (forward, backward) for the
    stack, create_flow wraps the same vectors (clipped to +-20) in a Flow, identical frames give the flow the oracle
    gives for identical frames (close to zero)."""
    blob = _reference_blob(tf).astype(np.float32)
    stack = np.stack([np.roll(blob, -1, (0, 1)), blob, np.roll(blob, 1, (0, 1))])
    fwd, bwd = tf.calculate_flow(stack, "Farneback")
    obj = tf.create_flow(stack, "Farneback")
    assert isinstance(obj, tf.Flow) and obj.shape == stack.shape
    assert fwd.shape == stack.shape + (2,) and fwd.dtype == np.float32
    assert np.array_equal(np.clip(fwd, -20, 20), obj.forward_flow) and np.array_equal(np.clip(bwd, -20, 20), obj.backward_flow)
    assert np.array_equal(fwd[-1], -bwd[-1]) and np.array_equal(bwd[0], -fwd[0])        # mirrored end frames (flow.py:425-426)
    for i in range(2):                                                                  # pair i against the oracle
        a, b = (np_ops_to8(stack[i], stack[i + 1]))
        assert np.array_equal(fwd[i], _oracle_farneback(a, b))
        assert np.array_equal(bwd[i + 1], _oracle_farneback(b, a))
    same = tf.calculate_flow(np.stack([blob] * 3), "Farneback")
    assert np.allclose(same[0], 0, atol=0.05) and np.allclose(same[1], 0, atol=0.05)


def np_ops_to8(x, y):
    from oracle import np_ops
    pair = np_ops.to_8bit(np_ops.linear_norm(np.stack([x, y])), 0, 1)
    return np.ascontiguousarray(pair[0]), np.ascontiguousarray(pair[1])


def test_calculate_flow_2_pairs_two_stacks(tf):
    """calculate_flow_2 (flow.py:431-496): flow from a[i] to b[i] on the jointly normalised pair -- with the
    reference's own indexing, which it shares with calculate_flow: only the first T - 1 pairs are computed, the forward
    flow of pair i is stored at i and its BACKWARD flow at i + 1, then forward[-1] = -backward[-1] and
    backward[0] = -forward[0]."""
    rng = np.random.default_rng(21)
    a = ndi.gaussian_filter(rng.normal(size=(3, 60, 90)), (0, 3, 3)).astype(np.float32)
    b = np.roll(a, (1, -2), (1, 2))
    fwd, bwd = tf.calculate_flow_2(a, b, "Farneback")
    T = a.shape[0]
    assert fwd.shape == a.shape + (2,) and bwd.shape == a.shape + (2,)
    for i in range(T - 1):
        p, n = np_ops_to8(a[i], b[i])
        f, bk = tf.calculate_flow_frame(p, n, tf.select_of_model("Farneback"))
        assert np.array_equal(fwd[i], f) and np.array_equal(bwd[i + 1], bk)
        assert np.array_equal(f, _oracle_farneback(p, n))
    assert np.array_equal(fwd[T - 1], -bwd[T - 1]) and np.array_equal(bwd[0], -fwd[0])


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (7, 64), (65, 17), (84, 108), (85, 109), (96, 128), (129, 257), (168, 216), (333, 517)])
def test_variational_refinement_bit_exact_vs_oracle(tf, shape):
    """tf_varref (cv2.VariationalRefinement, flow.py:359, 513-519) against the oracle's C restatement: every float
    expression is evaluated in the same order, so the refined flow is IDENTICAL -- tile seams, odd sizes and images
    smaller than a tile included.  (Both restate OpenCV: parity with cv2 itself is unpinned, DESIGN.md.)"""
    from oracle import np_ops
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    H, W = shape
    a = ndi.gaussian_filter(rng.normal(size=(H + 8, W + 8)), 2.0)
    a = ((a - a.min()) / max(np.ptp(a), 1e-9) * 255)
    i0, i1 = a[4:-4, 4:-4].astype(np.uint8), a[3:-5, 6:-2].astype(np.uint8)
    flow = (rng.normal(size=(H, W, 2)) * 1.5).astype(np.float32)
    flow[rng.random((H, W)) < 0.02] = 25.0                     # far out of the image: replicated border taps
    want = np_ops.variational_refinement(i0, i1, flow)
    vr = tf.VariationalRefinement.create()
    given = flow.copy()
    got = vr.calc(i0, i1, given)
    assert got is given and got.dtype == np.float32            # refined in place like OpenCV's InputOutputArray
    assert np.array_equal(got, want), f"max abs diff {np.abs(got - want).max()}"
    vr.fixedPointIterations, vr.sorIterations, vr.alpha, vr.omega = 2, 3, 5.0, 1.2
    assert np.array_equal(vr.calc(i0, i1, flow.copy()),
                          np_ops.variational_refinement(i0, i1, flow, 2, 3, alpha=5.0, omega=1.2))
    # more sweeps than the fused SOR kernel's halo covers: one launch per half sweep, same arithmetic
    vr.fixedPointIterations, vr.sorIterations = 2, 7
    assert np.array_equal(vr.calc(i0, i1, flow.copy()),
                          np_ops.variational_refinement(i0, i1, flow, 2, 7, alpha=5.0, omega=1.2))
    vr.sorIterations = 0
    assert np.array_equal(vr.calc(i0, i1, flow.copy()), flow + np.float32(0))


@pytest.mark.parametrize("shape", [(37, 53), (90, 120), (200, 333)])
def test_variational_refinement_batch_equals_the_oracle_image_for_image(tf, shape):
    """tf_varref_batch (round 6): B images per set of launches, the grid's z dimension = the image -- every image's refined flow
    is the oracle's bit for bit (and so tf_varref's), with the flows as views into a larger (T, H, W, 2) array (a stride
    between images that is not H * W * 2), in groups smaller than the batch, with more sweeps than the fused kernel covers
    (per-image fallback inside the library) and with a workspace sized for one image only."""
    import ctypes
    import torch
    from oracle import np_ops
    from tobac_flow_amd import _lib
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    H, W = shape
    B = 5
    a = ndi.gaussian_filter(rng.normal(size=(B + 1, H + 8, W + 8)), (0, 2.0, 2.0))
    a = ((a - a.min()) / max(np.ptp(a), 1e-9) * 255)
    i0 = np.ascontiguousarray(a[:B, 4:-4, 4:-4]).astype(np.uint8)
    i1 = np.ascontiguousarray(a[1:, 3:-5, 6:-2]).astype(np.uint8)
    flow = (rng.normal(size=(B + 2, H, W, 2)) * 1.5).astype(np.float32)
    flow[rng.random((B + 2, H, W)) < 0.02] = 25.0
    want = [np_ops.variational_refinement(i0[b], i1[b], flow[1 + b]) for b in range(B)]
    vr = tf.VariationalRefinement.create()
    d0, d1 = torch.from_numpy(i0).cuda(), torch.from_numpy(i1).cuda()
    for rounds in (32, 0):                                   # all images in one group / one image per group
        big = torch.from_numpy(flow).cuda()
        view = big[1:1 + B]                                  # frames 1 .. B of a larger array
        vr.calc_batch_dev(d0, d1, view, rounds=rounds)
        got = big.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[1 + b], want[b]), (rounds, b, float(np.abs(got[1 + b] - want[b]).max()))
        assert np.array_equal(got[0], flow[0]) and np.array_equal(got[-1], flow[-1])       # the neighbours are untouched
    # a stride between the images that is larger than a frame: every second frame of the array
    big = torch.from_numpy(np.repeat(flow[1:1 + B], 2, axis=0)).cuda()
    L = _lib.lib()
    p = vr._params()
    ws = _lib.workspace(L.tf_varref_workspace_bytes_batch(B, H, W), "varref_test")
    _lib.check(L.tf_varref_batch(_lib.ptr(d0), _lib.ptr(d1), B, H * W, H, W, ctypes.byref(p), _lib.ptr(big), 2 * H * W * 2, 0,
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_varref_batch")
    got = big.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[2 * b], want[b]) and np.array_equal(got[2 * b + 1], flow[1 + b])
    # a workspace for ONE image: the library refines the images one after the other
    big = torch.from_numpy(flow[1:1 + B].copy()).cuda()
    one = L.tf_varref_workspace_bytes(H, W)
    _lib.check(L.tf_varref_batch(_lib.ptr(d0), _lib.ptr(d1), B, H * W, H, W, ctypes.byref(p), _lib.ptr(big), H * W * 2, 0,
                                 _lib.ptr(ws), one, _lib.stream_ptr()), "tf_varref_batch")
    assert all(np.array_equal(big[b].cpu().numpy(), want[b]) for b in range(B))
    assert L.tf_varref_batch(_lib.ptr(d0), _lib.ptr(d1), B, H * W, H, W, ctypes.byref(p), _lib.ptr(big), H * W * 2, 0, _lib.ptr(ws), one - 4096 - 1024, _lib.stream_ptr()) == -1
    assert L.tf_varref_batch(_lib.ptr(d0), _lib.ptr(d1), B, H * W - 1, H, W, ctypes.byref(p), _lib.ptr(big), H * W * 2, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    # parameters the fused SOR kernel does not cover (7 sweeps > its halo): per-image fallback inside the library, same bits
    vr.fixedPointIterations, vr.sorIterations, vr.alpha, vr.omega = 2, 7, 5.0, 1.2
    big = torch.from_numpy(flow[1:1 + B].copy()).cuda()
    vr.calc_batch_dev(d0, d1, big)
    for b in range(B):
        assert np.array_equal(big[b].cpu().numpy(), np_ops.variational_refinement(i0[b], i1[b], flow[1 + b], 2, 7, alpha=5.0, omega=1.2))


def test_vr_steps_refine_once_per_direction_like_the_reference(tf):
    """flow.py:513-519: any vr_steps > 0 runs exactly ONE VariationalRefinement.calc per direction, before the
    smoothing; create_flow / calculate_flow / calculate_flow_frame agree with each other and with the oracle pipeline
    (tests/test_flow.py:265-279, 323-333 are the reference's scenarios)."""
    from oracle import np_ops
    blob = _reference_blob(tf)
    nxt = np.roll(blob, -1, [0, 1])
    model = tf.select_of_model("Farneback")
    plain = tf.calculate_flow_frame(blob, nxt, model)
    refined = tf.calculate_flow_frame(blob, nxt, model, vr_steps=1)
    assert np.array_equal(refined[0], np_ops.variational_refinement(blob, nxt, plain[0]))
    assert np.array_equal(refined[1], np_ops.variational_refinement(nxt, blob, plain[1]))
    many = tf.calculate_flow_frame(blob, nxt, model, vr_steps=3)
    assert np.array_equal(many[0], refined[0]) and np.array_equal(many[1], refined[1])
    sm = tf.calculate_flow_frame(blob, nxt, model, vr_steps=1, smoothing_steps=1, interp_method="cubic")
    want = np_ops.smooth_flow_step(refined[0], refined[1], "cubic")
    assert np.array_equal(sm[0], want[0], equal_nan=True) and np.array_equal(sm[1], want[1], equal_nan=True)
    rng = np.random.default_rng(12)
    stack = (ndi.gaussian_filter(rng.normal(size=(4, 60, 72)), (0.5, 2, 2)) * 40 + 250).astype(np.float32)
    for kw in ({}, {"smoothing_passes": 1, "interp_method": "cubic"}):
        fwd, bwd = tf.calculate_flow(stack, "Farneback", vr_steps=1, **kw)
        for i in range(3):
            p8 = np_ops.to_8bit(np_ops.linear_norm(stack[i:i + 2].copy()), 0, 1)
            f, b = tf.calculate_flow_frame(p8[0], p8[1], model, vr_steps=1, smoothing_steps=kw.get("smoothing_passes", 0),
                                           interp_method=kw.get("interp_method", "linear"))
            assert np.array_equal(fwd[i], f, equal_nan=True) and np.array_equal(bwd[i + 1], b, equal_nan=True)
    fl = tf.create_flow(stack, vr_steps=1, smoothing_passes=1, interp_method="cubic")     # scripts/dcc_detect_goes.py:164-166
    fwd, bwd = tf.calculate_flow(stack, "Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")
    assert np.array_equal(fl.forward_flow, np.clip(fwd, -20, 20)) and np.array_equal(fl.backward_flow, np.clip(bwd, -20, 20))


def test_calculate_flow_frame_smoothing_steps_match_oracle(tf):
    """smoothing_steps of calculate_flow_frame (flow.py:519-525) = that many smooth_flow_step passes"""
    from oracle import np_ops
    rng = np.random.default_rng(5)
    a = ndi.gaussian_filter(rng.normal(size=(70, 100)), 3)
    a = ((a - a.min()) / np.ptp(a) * 255).astype(np.uint8)
    b = np.roll(a, (2, -1), (0, 1))
    model = tf.select_of_model("Farneback")
    f0, b0 = tf.calculate_flow_frame(a, b, model)
    for steps, method in [(1, "linear"), (2, "cubic")]:
        f, bk = tf.calculate_flow_frame(a, b, model, smoothing_steps=steps, interp_method=method)
        wf, wb = f0, b0
        for _ in range(steps):
            wf, wb = np_ops.smooth_flow_step(wf, wb, method)
        assert np.max(np.abs(f - wf)) <= 1e-5 and np.max(np.abs(bk - wb)) <= 1e-5


@pytest.mark.parametrize("method,kwargs", [("inverse_log", {}), ("z_score", {"max_std": 2}), ("uniform", {"quantiles": 64}),
                                           ("local_linear", {"size": 25}), ("log", {})])
def test_calculate_flow_with_other_normalisation_methods(tf, method, kwargs):
    """calculate_flow(normalisation_method=...) (flow.py:362-428): the pair is normalised jointly by the chosen method,
    quantised with to_8bit(., 0, 1) and handed to the flow model; equal to doing exactly that by hand per pair."""
    from tobac_flow_amd.utils.normalisation_utils import select_normalisation_method
    rng = np.random.default_rng(9)
    base = ndi.gaussian_filter(rng.normal(size=(64, 96)), 3) * 30 + 250
    stack = np.stack([np.roll(base, (i, -i), (0, 1)) for i in range(3)]).astype(np.float32)
    fwd, bwd = tf.calculate_flow(stack, "Farneback", normalisation_method=method, **kwargs)
    norm = select_normalisation_method(method)
    model = tf.select_of_model("Farneback")
    for i in range(2):
        p8 = tf.to_8bit(norm(np.stack([stack[i], stack[i + 1]], 0), **kwargs), 0, 1)
        f, b = tf.calculate_flow_frame(np.ascontiguousarray(p8[0]), np.ascontiguousarray(p8[1]), model)
        assert np.array_equal(fwd[i], f) and np.array_equal(bwd[i + 1], b), (method, i)
    # for a brightness-temperature-like field the reference's log_norm gives all zeros and its inverse_log_norm a
    # range of ~5 / 300 (two bits after to_8bit): no or almost no flow signal survives (see test_host_logic)
    if method == "log":
        assert not fwd.any()
    elif method == "inverse_log":
        assert np.abs(fwd).max() < 0.1
    else:
        assert np.abs(fwd[0]).max() > 0.3
    with pytest.raises(ValueError):
        tf.calculate_flow(stack, "Farneback", normalisation_method="quadratic")


@pytest.mark.parametrize("interp", ["nearest", "linear", "cubic"])
def test_sobel_edge_field_fused_is_bit_identical_to_the_two_kernel_form(tf, interp):
    """tf_sobel_edge_field against tf_convolve(SOBEL_UPHILL, float64) + tf_edge_field (the two-kernel form of
    detection.py:620-642), float32 and float64 outputs, NaNs in the field, first / last frame (missing neighbours)."""
    import torch
    from tobac_flow_amd import _lib
    rng = np.random.default_rng(12)
    shape = (4, 45, 70)
    field = rand_field(rng, shape).astype(np.float32)
    field[rng.random(shape) < 0.03] = np.nan
    fwd, bwd = rand_flow(rng, shape, 2.5), rand_flow(rng, shape, 2.5)
    T, H, W = shape
    L = _lib.lib()
    f = torch.from_numpy(field).cuda()
    fw, bw = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    code = _lib.INTERP[interp]
    struct = np.ones(27, np.uint8)
    sob = torch.empty(shape, dtype=torch.float64, device="cuda")
    _lib.check(L.tf_convolve(_lib.ptr(f), _lib.TF_F32, T, H, W, _lib.ptr(fw), _lib.ptr(bw), struct.ctypes.data_as(_lib._P), code,
                             float("nan"), 2, _lib.ptr(sob), _lib.TF_F64, 0, T, _lib.stream_ptr()), "tf_convolve")
    for dt, ty in ((torch.float64, _lib.TF_F64), (torch.float32, _lib.TF_F32)):
        two = torch.empty(shape, dtype=dt, device="cuda")
        one = torch.empty(shape, dtype=dt, device="cuda")
        _lib.check(L.tf_edge_field(_lib.ptr(sob), _lib.ptr(f), sob.numel(), _lib.ptr(two), ty, _lib.stream_ptr()), "tf_edge_field")
        _lib.check(L.tf_sobel_edge_field(_lib.ptr(f), T, H, W, _lib.ptr(fw), _lib.ptr(bw), code, _lib.ptr(one), ty,
                                         _lib.stream_ptr()), "tf_sobel_edge_field")
        a, b = one.cpu().numpy(), two.cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), f"{interp} {dt}: {int((a != b).sum())} differ"
        assert np.isposinf(a[np.isnan(field)]).all() and np.isfinite(a).any()


# ----------------------------------------------------------------------------- OpenCV itself, where it exists
def test_farneback_and_remap_against_opencv_when_it_is_installed(tf):
    """SURVEY.md section 7 hard part 2: the cv2-backed stages are pinned only on a box that has OpenCV with the contrib
    `optflow` module.  There this asserts the north-star tolerance (1e-4 abs on the flow; remap: NaN masks equal and
    values within float32 rounding of OpenCV's fixed-point weights); elsewhere it skips with the reason -- the same
    probe bench.py reports as `cv2_parity`."""
    cv2 = pytest.importorskip("cv2", reason="parity unpinned: OpenCV is not installed on this box")
    if not hasattr(cv2, "optflow"):
        pytest.skip("parity unpinned: this OpenCV build has no optflow (contrib) module")
    import bench
    res = bench.cv2_parity()
    assert res["status"] == "pinned"
    assert res["farneback_max_abs_diff"] <= 1e-4
    for name in ("nearest", "linear", "cubic", "lanczos"):
        assert res[f"remap_{name}_nan_mask_equal"]
        assert res[f"remap_{name}_max_abs_diff"] <= (0 if name == "nearest" else 1e-3)
    if res["varref_max_abs_diff"] is not None:                # cv2.VariationalRefinement on the same input flow
        assert res["varref_max_abs_diff"] <= 1e-4


@pytest.mark.parametrize("kw", [dict(win_size=9), dict(win_size=15, num_iters=3), dict(poly_n=7, poly_sigma=1.5),
                                dict(num_levels=2, pyr_scale=0.6, win_size=13)])
def test_farneback_non_default_parameters_match_oracle(tf, kw):
    """Parameters other than OpenCV's defaults take other kernels: window sizes != 13 the unfused pair
    k_fb_update_matrices + k_fb_blur_solve, polyN != 5 the generic expansion kernel, other pyramid scales the generic
    resize -- each against the oracle's restatement with the same parameters."""
    import ctypes
    from oracle import _lib as ol
    from tobac_flow_amd.utils.flow_utils import FarnebackFlow
    rng = np.random.default_rng(17)
    a = ndi.gaussian_filter(rng.normal(size=(141, 203)), 2.5)
    a = ((a - a.min()) / np.ptp(a) * 255).astype(np.uint8)
    b = np.roll(a, (1, -2), (0, 1))
    p = dict(num_levels=5, pyr_scale=0.5, win_size=13, num_iters=10, poly_n=5, poly_sigma=1.1)
    p.update(kw)
    got = FarnebackFlow(**p).calc(a, b, None)
    L = ol.lib()
    L.oracle_farneback.restype = ctypes.c_int
    want = np.zeros(a.shape + (2,), np.float32)
    L.oracle_farneback(ol.ptr(a, ctypes.c_uint8), ol.ptr(b, ctypes.c_uint8), a.shape[0], a.shape[1], ol.ptr(want, ctypes.c_float),
                       p["num_levels"], ctypes.c_double(p["pyr_scale"]), p["win_size"], p["num_iters"], p["poly_n"],
                       ctypes.c_double(p["poly_sigma"]))
    assert np.abs(got - want).max() <= 1e-4, np.abs(got - want).max()
    assert np.abs(np.median(got[20:-20, 20:-20].reshape(-1, 2), 0) - np.array([-2, 1])).max() < 0.2


def test_lanczos_interpolation_matches_oracle_everywhere_it_is_accepted(tf):
    """method="lanczos" (cv2.INTER_LANCZOS4, convolve.py:47-54 / flow_utils.py:22-34): single-image warp, the smoothing
    step, the generic convolve (raw stack and nanmean) and the 27-tap Sobel, bit for bit against the oracle; borders,
    far-out flows and NaN samples included."""
    from oracle import np_ops
    rng = np.random.default_rng(23)
    shape = (3, 41, 57)
    data = rand_field(rng, shape, nan_frac=0.005)
    fwd, bwd = rand_flow(rng, shape, 2.5), rand_flow(rng, shape, 2.5)
    fwd[0, 5, 5] = (60.0, -70.0)                                   # far outside
    _eq(tf.warp_flow(data[0], fwd[0], method="lanczos"), np_ops.warp_flow_single(data[0], fwd[0], "lanczos"))
    gf, gb = tf.smooth_flow_step(fwd[1], bwd[1], "lanczos")
    wf, wb = np_ops.smooth_flow_step(fwd[1], bwd[1], "lanczos")
    _eq(gf, wf)
    _eq(gb, wb)
    fl = tf.Flow(fwd, bwd)
    s = ndi.generate_binary_structure(3, 1)
    _eq(fl.convolve(data, structure=s, method="lanczos"), np_ops.convolve(data, fwd, bwd, s, "lanczos", np.float32, np.nan, None))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np_ops.convolve(data, fwd, bwd, s, "lanczos", np.float32, np.nan, lambda x: np.nanmean(x, 0))
    _eq(fl.convolve(data, structure=s, method="lanczos", func=lambda x: np.nanmean(x, 0)), want)
    for direction in (None, "uphill"):
        _eq(fl.sobel(data, method="lanczos", direction=direction), np_ops.sobel(data, fwd, bwd, "lanczos", None, np.nan, direction))


@pytest.mark.parametrize("name", EXACT_VS_REFERENCE + ["C_quant4_c1", "E_const_plateau_c1"])
def test_watershed_raveled_twin_takes_the_references_own_arguments(tf, golden_ws, name):
    """tobac_flow_amd._watershed.watershed_raveled = the reference's native seam (_watershed.pyx:222-233), same twelve
    arguments, `output` mutated in place: fed with exactly what watershed.py:59-149 prepares (oracle/ws_oracle.prepare:
    padding, raveled neighbourhood, raveled int32 flow offsets) it returns the reference's golden labels -- on the
    tie-heavy goldens too (default since round 4: the reference heap's own order of equal-valued markers); with
    reference_order=False those two give the idealised-order labels with a warning."""
    import warnings
    from oracle import ws_oracle
    from tobac_flow_amd._watershed import watershed_raveled
    from tobac_flow_amd.watershed import WatershedAmbiguityWarning
    c = golden_ws[name]
    conn = int(c["conn"])
    p = ws_oracle.prepare(c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"), conn)
    out = p["out"].ravel().copy()
    args = (np.ascontiguousarray(p["field"].ravel()), p["markers"].astype(np.intp), p["nbr"].astype(np.intp), p["fwd_off"],
            p["bwd_off"], p["fwd_loc"], p["bwd_loc"], p["mask"], p["strides"].astype(np.int32), 0.0, out, False)
    pd = p["pad"]
    tie_heavy = name in ("C_quant4_c1", "E_const_plateau_c1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # the default: nothing left to warn about
        assert watershed_raveled(*args) is None
    o = out.reshape(p["out"].shape)
    assert np.array_equal(o[pd[0]:o.shape[0] - pd[0], pd[1]:o.shape[1] - pd[1], pd[2]:o.shape[2] - pd[2]], c["labels"])
    assert not o[:pd[0]].any() and not o[:, :pd[1]].any() and not o[:, :, :pd[2]].any()          # the padding ring stays 0
    out[...] = p["out"].ravel()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert watershed_raveled(*args, reference_order=False) is None
    got = o[pd[0]:o.shape[0] - pd[0], pd[1]:o.shape[1] - pd[1], pd[2]:o.shape[2] - pd[2]]
    want = ws_oracle.watershed(c["fwd"], c["bwd"], c["field"], c["markers"], c.get("mask"), conn, tie_mode=1) if tie_heavy else c["labels"]
    assert np.array_equal(got, want)
    assert any(issubclass(w.category, WatershedAmbiguityWarning) for w in rec) == tie_heavy


def test_watershed_raveled_argument_checks(tf):
    from tobac_flow_amd._watershed import watershed_raveled
    img = np.zeros(27, np.float32)
    out = np.zeros(27, np.int32)
    out[13] = 1
    i32, z8 = np.zeros(27, np.int32), np.ones(27, np.int8)
    ok = [img, np.array([13], np.intp), np.array([-1, 1], np.intp), i32, i32, np.zeros(2, np.int32), np.zeros(2, np.int32), z8,
          np.array([9, 3, 1], np.int32), 0.0, out, False]
    assert watershed_raveled(*ok) is None and out.tolist() == [1] * 27               # a 1-D chain floods end to end
    for k, bad in ((0, img.astype(np.float64)), (10, out.astype(np.int64)), (7, z8.astype(bool)), (3, i32.reshape(3, 9))):
        args = list(ok)
        args[k] = bad
        with pytest.raises(ValueError):
            watershed_raveled(*args)
    for k, bad in ((9, 0.5), (11, True)):                                            # compact watershed / watershed lines
        args = list(ok)
        args[k] = bad
        with pytest.raises(ValueError):
            watershed_raveled(*args)
    args = list(ok)
    args[1] = np.array([13, 5], np.intp)                                             # not np.flatnonzero order
    with pytest.raises(ValueError):
        watershed_raveled(*args)


def test_shared_reciprocal_division_equals_the_hardware_division():
    """k_vr_system divides fifteen products of derivative values by three denominators through one refined reciprocal
    each; in the operands' range that is the IEEE division bit for bit (varref.hip, vr_div_shared)."""
    import ctypes
    from tobac_flow_amd import _lib
    L = _lib.lib()
    for seed in (1, 2, 3):
        bad = ctypes.c_uint64(123)
        _lib.check(L.tf_selftest_shared_divide(1 << 26, seed, ctypes.byref(bad), _lib.stream_ptr()), "selftest")
        assert bad.value == 0


def test_variational_refinement_random_shapes_and_parameters(tf):
    """a sweep over shapes around the tile kernel's geometry (108 x 84 tiles, 128 x 104 regions, 10-pixel halo) with
    random iteration counts and weights: identical to the oracle every time"""
    from oracle import np_ops
    rng = np.random.default_rng(2024)
    shapes = [(int(rng.integers(1, 260)), int(rng.integers(1, 330))) for _ in range(10)] + [(83, 107), (94, 118), (104, 128), (105, 129)]
    for H, W in shapes:
        a = ndi.gaussian_filter(rng.normal(size=(H + 8, W + 8)), 1.5)
        a = ((a - a.min()) / max(np.ptp(a), 1e-9) * 255)
        i0, i1 = a[4:-4, 4:-4].astype(np.uint8), a[5:-3, 3:-5].astype(np.uint8)
        flow = (rng.normal(size=(H, W, 2)) * 2).astype(np.float32)
        fp, sor = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        alpha, delta, gamma, omega = float(rng.uniform(5, 30)), float(rng.uniform(1, 8)), float(rng.uniform(2, 15)), float(rng.uniform(1.0, 1.9))
        vr = tf.VariationalRefinement.create()
        vr.fixedPointIterations, vr.sorIterations, vr.alpha, vr.delta, vr.gamma, vr.omega = fp, sor, alpha, delta, gamma, omega
        got = vr.calc(i0, i1, flow.copy())
        want = np_ops.variational_refinement(i0, i1, flow, fp, sor, alpha=alpha, delta=delta, gamma=gamma, omega=omega)
        assert np.array_equal(got, want), ((H, W), fp, sor, np.abs(got - want).max())


@pytest.mark.parametrize("shape", [(84, 108), (333, 517)])
def test_variational_refinement_fast_divide_stays_within_the_flow_tolerance(tf, shape):
    """TF_VR_FAST_DIVIDE (opt-in, VariationalRefinement.fastDivide): hardware reciprocals instead of correctly rounded
    divisions -- no longer the oracle's bits, but within the north star's 1e-4 px of it on identical input flows
    (VERDICT r2 next-round 5a).  The default stays bit-identical (test_variational_refinement_bit_exact_vs_oracle)."""
    from oracle import np_ops
    rng = np.random.default_rng(shape[0] + 1)
    H, W = shape
    a = ndi.gaussian_filter(rng.normal(size=(H + 8, W + 8)), 2.0)
    a = ((a - a.min()) / np.ptp(a) * 255).astype(np.uint8)
    i0, i1 = np.ascontiguousarray(a[4:4 + H, 4:4 + W]), np.ascontiguousarray(a[3:3 + H, 6:6 + W])
    flow0 = (ndi.gaussian_filter(rng.normal(size=(H, W, 2)), (3, 3, 0)) * 4 + np.array([2.0, -1.0])).astype(np.float32)
    want = np_ops.variational_refinement(i0, i1, flow0.copy())
    vr = tf.VariationalRefinement.create()
    assert vr.fastDivide is False
    exact = vr.calc(i0, i1, flow0.copy())
    assert np.array_equal(exact, want)
    vr.fastDivide = True
    fast = vr.calc(i0, i1, flow0.copy())
    d = np.abs(fast - want)
    print("fast divide vs oracle: max %.3g, mean %.3g, identical %.1f %%" % (d.max(), d.mean(), 100.0 * (d == 0).mean()))
    assert d.max() <= 1e-4 and d.max() > 0
