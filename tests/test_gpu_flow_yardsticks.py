"""The device's flow core judged by the float64 yardsticks of tests/flow_yardsticks.py (bounds derived in its docstring): the
full-resolution blur and polynomial expansion (tf_farneback_expansion), the remap behind tf_warp_flow and the four warps of
tf_smooth_flow_step, and two exact identities of the refinement (tf_varref, tf_varref_ex, tf_varref_batch).  The bounds are
the twin's, without a margin for the device: the kernels are bit-identical to the twin, so an excess here is a finding.

Only the library and the yardstick module are used.  Every test prints its error / bound before it asserts."""
import ctypes

import numpy as np
import pytest

import flow_yardsticks as Y

pytestmark = pytest.mark.gpu

_ids = lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)        # noqa: E731


def _lib():
    from tobac_flow_amd import _lib as lib
    return lib


def _torch():
    import torch
    return torch


def device_expansion(img_u8, n, sigma):
    """(blur (h, w), R (h, w, 5)) of tf_farneback_expansion; the entry honours poly_n / poly_sigma (n != 5: k_fb_polyexp)"""
    from tobac_flow_amd.utils.flow_utils import FarnebackFlow
    t, lib = _torch(), _lib()
    L = lib.lib()
    h, w = img_u8.shape
    d_img = t.from_numpy(np.array(img_u8, np.uint8, order="C")).cuda()            # a copy: the shared reference is read-only
    d_blur = t.empty((h, w), dtype=t.float32, device="cuda")
    d_R = t.empty(5 * h * w, dtype=t.float32, device="cuda")
    m = FarnebackFlow(poly_n=n, poly_sigma=sigma)
    lib.check(L.tf_farneback_expansion(lib.ptr(d_img), h, w, ctypes.byref(m.params), lib.ptr(d_blur), lib.ptr(d_R),
                                       lib.stream_ptr()), "tf_farneback_expansion")
    t.cuda.synchronize()
    R = d_R.cpu().numpy()
    return d_blur.cpu().numpy(), np.concatenate([R[:4 * h * w].reshape(h, w, 4), R[4 * h * w:].reshape(h, w, 1)], -1)


# ---- 1. blur of the full-resolution level, polynomial expansion --------------------------------------------------------------
@pytest.mark.parametrize("n,sigma,content,shape", Y.expansion_cases(), ids=_ids)
def test_blur_is_the_exact_binomial_and_the_expansion_the_least_squares_fit(n, sigma, content, shape):
    img, blur, value, bound = Y.expansion_reference(shape, content, n, sigma)
    got_blur, got = device_expansion(img, n, sigma)
    assert np.array_equal(got_blur, blur)
    ratio = Y.worst_ratio(got, value, bound)
    print(f"expansion_n{n} {content} {shape}: error / bound = {ratio:.4f}")
    assert ratio <= 1


def test_expansion_returns_the_coefficients_of_a_quadratic_in_the_interior():
    """x^2 + y^2 - x y + 2 x + 3 y + 60 about (7, 6) on 14 x 16: the binomial blur adds a constant to a quadratic away from the
    border, so from n + 1 pixels inside the expansion is (r_y, r_x, 1, 1, -1) -- (4, 3, 1, 1, -1) at the pixel (8, 7)"""
    n, sigma = Y.DEFAULT_POLY
    img = Y.quadratic_frame()
    assert img.min() >= 0 and img.max() <= 255 and np.array_equal(img, np.rint(img))
    got_blur, got = device_expansion(img.astype(np.uint8), n, sigma)
    want = Y.quadratic_coefficients()
    _, bound = Y.expansion_yardstick(Y.blur3_yardstick(img.astype(np.uint8)), n, sigma)
    inner = (slice(n + 1, -n - 1), slice(n + 1, -n - 1))
    assert want[inner].shape[:2] == (2, 4) and want[7, 8].tolist() == [4, 3, 1, 1, -1]
    assert np.array_equal(got_blur[1:-1, 1:-1], (img + 1.0)[1:-1, 1:-1])       # (f'' / 4 per axis) = 1/2 + 1/2
    ratio = Y.worst_ratio(got[inner], want[inner], bound[inner])
    print(f"expansion_n{n} quadratic: error / bound = {ratio:.4f}")
    assert ratio <= 1


# ---- 3. remap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,shape,kind", Y.remap_cases(), ids=_ids)
def test_warp_flow(method, shape, kind):
    from tobac_flow_amd.utils.flow_utils import warp_flow
    img, flow, value, bound = Y.remap_reference(shape, kind, method)
    got = warp_flow(img.copy(), flow.copy(), method)
    assert got.dtype == np.float32
    ratio = Y.worst_ratio(got, value, bound)                                    # NaN placement: exact, asserted inside
    print(f"remap_{method} {shape} {kind}: error / bound = {ratio:.4f}")
    assert ratio <= 1


@pytest.mark.parametrize("method", Y.REMAP_METHODS)
@pytest.mark.parametrize("shape", Y.SMOOTH_SHAPES, ids=_ids)
def test_smooth_flow_step_through_its_four_warps(shape, method):
    import tobac_flow_amd.flow as tf
    fwd, bwd, (fv, fb), (bv, bb) = Y.smooth_reference(shape, method)
    f2, b2 = tf.smooth_flow_step(fwd.copy(), bwd.copy(), method)
    ratio = max(Y.worst_ratio(f2, fv, fb), Y.worst_ratio(b2, bv, bb))
    print(f"smooth_{method} {shape}: error / bound = {ratio:.4f}")
    assert ratio <= 1


# ---- 4. refinement identities --------------------------------------------------------------------------------------------------
def _workspace(nbytes):
    t = _torch()
    return t.empty((int(nbytes) + 255) // 256 * 256, dtype=t.uint8, device="cuda")


def _refine(i0, i1, flow, flags):
    """flags None: tf_varref; otherwise tf_varref_ex with these flags"""
    t, lib = _torch(), _lib()
    L = lib.lib()
    H, W = flow.shape[:2]
    p = lib.VarRefParams()
    L.tf_varref_default_params(ctypes.byref(p))
    assert (p.fixed_point_iterations, p.sor_iterations) == (5, 5)
    ws = _workspace(L.tf_varref_workspace_bytes(H, W))
    d0, d1, f = t.from_numpy(i0.copy()).cuda(), t.from_numpy(i1.copy()).cuda(), t.from_numpy(flow.copy()).cuda()
    if flags is None:
        lib.check(L.tf_varref(lib.ptr(d0), lib.ptr(d1), H, W, ctypes.byref(p), lib.ptr(f), lib.ptr(ws), ws.numel(),
                              lib.stream_ptr()), "tf_varref")
    else:
        lib.check(L.tf_varref_ex(lib.ptr(d0), lib.ptr(d1), H, W, ctypes.byref(p), lib.ptr(f), flags, lib.ptr(ws), ws.numel(),
                                 lib.stream_ptr()), "tf_varref_ex")
    return f.cpu().numpy()


def _refine_batch(i0, i1, flow, B=3):
    """tf_varref_batch on B copies of the case; the flows are frames 1 .. B of a (B + 2, H, W + 1, 2) array: a padded stride,
    whose other words must stay as they were"""
    t, lib = _torch(), _lib()
    L = lib.lib()
    H, W = flow.shape[:2]
    p = lib.VarRefParams()
    L.tf_varref_default_params(ctypes.byref(p))
    stride = 2 * H * (W + 1)
    host = np.full((B + 2) * stride, 1234.5, np.float32)
    for b in range(B):
        host[(1 + b) * stride:(1 + b) * stride + 2 * H * W] = flow.ravel()
    big = t.from_numpy(host).cuda()
    d0 = t.from_numpy(np.ascontiguousarray(np.stack([i0] * B))).cuda()
    d1 = t.from_numpy(np.ascontiguousarray(np.stack([i1] * B))).cuda()
    ws = _workspace(L.tf_varref_workspace_bytes_batch(B, H, W))
    lib.check(L.tf_varref_batch(lib.ptr(d0), lib.ptr(d1), B, H * W, H, W, ctypes.byref(p),
                                ctypes.c_void_p(big.data_ptr() + 4 * stride), stride, 0, lib.ptr(ws), ws.numel(),
                                lib.stream_ptr()), "tf_varref_batch")
    out = big.cpu().numpy()
    inside = np.zeros(out.size, bool)
    for b in range(B):
        inside[(1 + b) * stride:(1 + b) * stride + 2 * H * W] = True
    assert (out[~inside] == np.float32(1234.5)).all(), "words outside the output frames changed"
    return [out[(1 + b) * stride:(1 + b) * stride + 2 * H * W].reshape(H, W, 2) for b in range(B)]


@pytest.mark.parametrize("entry", ["tf_varref", "ex-0", "ex-fast-divide", "ex-fast-sor", "ex-both", "batch"])
@pytest.mark.parametrize("identity", ["identical", "constant"])
@pytest.mark.parametrize("shape", Y.VARREF_SHAPES, ids=_ids)
def test_refinement_identities(shape, identity, entry):
    """identical frames with a zero flow return zeros; constant frames (two greys) with the constant flow (0.3125, -1.7) return
    the flow's bits"""
    i0, i1, flow = Y.varref_frames(shape, identity)
    if entry == "batch":
        outs = _refine_batch(i0, i1, flow)
    else:
        outs = [_refine(i0, i1, flow, {"tf_varref": None, "ex-0": 0, "ex-fast-divide": 1, "ex-fast-sor": 2, "ex-both": 3}[entry])]
    for out in outs:
        if identity == "identical":
            assert np.array_equal(out, np.zeros_like(out))
        else:
            assert out.tobytes() == flow.tobytes()
