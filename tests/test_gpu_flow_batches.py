"""The batched flow entry points -- tf_varref_batch, tf_farneback_batch, tf_farneback_batch_split and
tf_farneback_batch_phase -- across parameters, strides, one-sided calls and workspace contents.

create_flow, the detection scripts and bench.py compute every flow through these calls.  What a batch adds to the
single-image code is per-image offsets (grid z times a batch stride, varref planes padded to 64 floats, hand-over words
per pair), and those offsets are checked here where the single-image tests cannot see them:
  - every image of a batch equals the single-image call on that image (same kernels, same data: bit for bit), and the
    single image equals the oracle at the parameters (bit for bit, or within the stated 1e-4 px where a generic kernel
    sums in another order);
  - odd image strides (unaligned frames), flow strides larger than a frame (the gaps stay untouched), NULL for one direction;
  - the output does not depend on what the workspace held before the call.
Inputs are smooth seeded uint8 frames whose content drifts by a pixel per frame.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

pytestmark = pytest.mark.gpu

TF_VR_FAST_DIVIDE, TF_VR_FAST_SOR = 1, 2
SENTINEL = 1234.5                     # flow-buffer words outside the output frames (finite: a stray read is a wrong number)
POISON = (0.75, -3.0)                 # workspace fills of the poisoned-scratch tests (finite: see section 4)


# ----------------------------------------------------------------------------- helpers
def _lib():
    from tobac_flow_amd import _lib as lib
    return lib


def _torch():
    import torch
    return torch


def _frames(rng, n, H, W):
    """n smooth uint8 frames; the content drifts by one pixel per frame down and to the left"""
    base = ndi.gaussian_filter(rng.normal(size=(H + 2 * n, W + 2 * n)), 2.5)
    base = ((base - base.min()) / max(np.ptp(base), 1e-9) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([base[i:i + H, 2 * n - i:2 * n - i + W] for i in range(n)]))


def _at(t, offset):
    """pointer to element `offset` of the device tensor t"""
    return ctypes.c_void_p(t.data_ptr() + offset * t.element_size())


def _dev_frames(frames, stride):
    """frames (n, H, W) in one device byte buffer, frame i at byte i * stride (the gaps hold other bytes)"""
    n, H, W = frames.shape
    buf = np.full(n * stride + 64, 77, np.uint8)
    for i in range(n):
        buf[i * stride:i * stride + H * W] = frames[i].ravel()
    return _torch().from_numpy(buf).cuda()


def _workspace(nbytes, fill=None):
    """a workspace of the test's own (not _lib.workspace's shared one), optionally filled with one float value"""
    t = _torch()
    ws = t.empty((int(nbytes) + 255) // 256 * 256, dtype=t.uint8, device="cuda")
    if fill is not None:
        ws.view(t.float32).fill_(fill)
    return ws


class _FlowBuffer:
    """B output frames of H x W x 2 floats, frame b at float (1 + b) * stride of a buffer of (B + 2) * stride floats: a
    guard frame in front, the gap after each frame and a guard frame behind hold SENTINEL and must keep it"""

    def __init__(self, B, H, W, stride, frames=None):
        self.B, self.H, self.W, self.stride = B, H, W, stride
        host = np.full((B + 2) * stride, SENTINEL, np.float32)
        if frames is not None:
            for b in range(B):
                host[(1 + b) * stride:(1 + b) * stride + 2 * H * W] = frames[b].ravel()
        self.dev = _torch().from_numpy(host).cuda()

    def ptr(self, b=0):
        return _at(self.dev, (1 + b) * self.stride)

    def frames(self):
        host = self.dev.cpu().numpy()
        n = 2 * self.H * self.W
        inside = np.zeros(host.size, bool)
        for b in range(self.B):
            inside[(1 + b) * self.stride:(1 + b) * self.stride + n] = True
        outside = host[~inside]
        assert (outside == np.float32(SENTINEL)).all(), f"{int((outside != np.float32(SENTINEL)).sum())} words outside the output frames changed"
        return np.stack([host[(1 + b) * self.stride:(1 + b) * self.stride + n].reshape(self.H, self.W, 2) for b in range(self.B)])


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, max abs {np.nanmax(d) if np.isfinite(d).any() else d.max()}")


def _max_dev(got, want):
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())


# ----------------------------------------------------------------------------- 1. tf_varref_batch
VR_DEFAULTS = dict(alpha=20.0, delta=5.0, gamma=10.0, omega=1.6)
# (fixed_point_iterations, sor_iterations, weights away from the defaults).  The first seven run the fused SOR tile kernel
# for the whole batch (2 * sor <= VRT_HALO = 10); (2, 6) and (3, 0) fall back to one image at a time inside the library
VR_CASES = [(0, 1, {}), (0, 5, dict(alpha=7.5, omega=1.3)), (1, 1, {}), (1, 5, dict(delta=2.0, gamma=4.0)),
            (2, 3, dict(alpha=35.0, delta=8.0, gamma=15.0, omega=1.9)), (3, 4, {}), (5, 5, dict(omega=1.1)),
            (2, 6, dict(alpha=12.0)), (3, 0, {})]
# around the tile geometry (108 x 84 tiles); 2 x 3, 37 x 53 and 85 x 109 have H * W no multiple of 64: padded planes
VR_SHAPES = [(2, 3), (37, 53), (84, 108), (85, 109), (129, 257)]
VR_BATCHES = [2, 3, 7]
# every (fp, sor) pair on two shapes, each with a batch of more than one image
VR_PARAMS = [pytest.param(fp, sor, kw, VR_SHAPES[(i + 2 * j) % 5], VR_BATCHES[(i + j) % 3], id=f"fp{fp}-sor{sor}-{VR_SHAPES[(i + 2 * j) % 5][0]}x{VR_SHAPES[(i + 2 * j) % 5][1]}-B{VR_BATCHES[(i + j) % 3]}")
             for i, (fp, sor, kw) in enumerate(VR_CASES) for j in range(2)]


def _vr_params(fp, sor, kw):
    w = dict(VR_DEFAULTS, **kw)
    return _lib().VarRefParams(fp, sor, w["alpha"], w["delta"], w["gamma"], w["omega"]), w


def _vr_inputs(H, W, B, seed):
    rng = np.random.default_rng(seed)
    fr = _frames(rng, B + 1, H, W)                      # image b refines frame b -> frame b + 1
    flow = (rng.normal(size=(B, H, W, 2)) * 1.5).astype(np.float32)
    flow[rng.random((B, H, W)) < 0.02] = 25.0           # far out of the image: replicated border taps
    flow[rng.random((B, H, W)) < 0.02] = -0.0           # W + 0 turns these into +0 where nothing is refined
    return fr, flow


def _vr_single(fr, flow, p, flags, fill=None):
    """tf_varref_ex image by image on contiguous copies"""
    t, lib = _torch(), _lib()
    L = lib.lib()
    B, H, W = flow.shape[:3]
    ws = _workspace(L.tf_varref_workspace_bytes(H, W), fill)
    out = []
    for b in range(B):
        d0, d1 = t.from_numpy(fr[b].copy()).cuda(), t.from_numpy(fr[b + 1].copy()).cuda()
        f = t.from_numpy(flow[b].copy()).cuda()
        lib.check(L.tf_varref_ex(lib.ptr(d0), lib.ptr(d1), H, W, ctypes.byref(p), lib.ptr(f), flags, lib.ptr(ws), ws.numel(),
                                 lib.stream_ptr()), "tf_varref_ex")
        out.append(f.cpu().numpy())
    return np.stack(out)


def _vr_batch(fr, flow, p, flags, img_stride, flow_stride, fill=None):
    """tf_varref_batch on frames img_stride bytes apart and flows flow_stride floats apart (guard words checked)"""
    lib = _lib()
    L = lib.lib()
    B, H, W = flow.shape[:3]
    dimg = _dev_frames(fr, img_stride)
    fb = _FlowBuffer(B, H, W, flow_stride, flow)
    ws = _workspace(L.tf_varref_workspace_bytes_batch(B, H, W), fill)
    lib.check(L.tf_varref_batch(_at(dimg, 0), _at(dimg, img_stride), B, img_stride, H, W, ctypes.byref(p), fb.ptr(), flow_stride,
                                flags, lib.ptr(ws), ws.numel(), lib.stream_ptr()), "tf_varref_batch")
    return fb.frames()


@pytest.mark.parametrize("fp,sor,kw,shape,B", VR_PARAMS)
def test_varref_batch_equals_the_single_image_and_the_oracle(fp, sor, kw, shape, B):
    """Every image of tf_varref_batch equals tf_varref_ex on that image, bit for bit: with flags 0 (and then the oracle
    too, up to the sign of a zero flow where no fixed-point iteration runs), TF_VR_FAST_SOR and TF_VR_FAST_DIVIDE (no
    oracle for those).  The frames sit at an odd byte stride > H * W in one
    buffer, the flows at a stride > 2 * H * W in a larger array whose other words stay untouched."""
    from oracle import np_ops
    H, W = shape
    fr, flow = _vr_inputs(H, W, B, H * 7919 + W * 31 + B * 7 + fp * 3 + sor)
    p, w = _vr_params(fp, sor, kw)
    img_stride = H * W + (1 if H * W % 2 == 0 else 2)   # odd
    flow_stride = 2 * H * W + 6
    for flags in (0, TF_VR_FAST_SOR, TF_VR_FAST_DIVIDE):
        single = _vr_single(fr, flow, p, flags)
        got = _vr_batch(fr, flow, p, flags, img_stride, flow_stride)
        for b in range(B):
            _same_bits(got[b], single[b], f"flags {flags}: image {b} of the batch against tf_varref_ex")
        if flags == 0:
            for b in range(B):
                want = np_ops.variational_refinement(fr[b], fr[b + 1], flow[b], fp, sor, **w)
                if fp == 0:
                    # no fixed-point iteration: the oracle hands back its copy of W, the library W + dW with dW = 0 --
                    # the same values, but -0 becomes +0
                    want = want + np.float32(0)
                _same_bits(single[b], want, f"image {b}: tf_varref_ex against the oracle")


@pytest.mark.parametrize("shape", [(37, 53), (85, 109)])
def test_varref_python_batch_without_fixed_point_iterations(shape):
    """VariationalRefinement.calc_batch_dev with fixedPointIterations = 0 (the tile path with no iteration: the refined
    flow is W + 0, -0 becomes +0) for every grouping: all images per launch (rounds 32 and 1 at these sizes) and one
    (rounds 0); the flows are a view into a larger array whose other frames stay untouched."""
    import tobac_flow_amd.flow as tf
    from oracle import np_ops
    t = _torch()
    H, W = shape
    B = 7
    fr, flow = _vr_inputs(H, W, B, H + W)
    vr = tf.VariationalRefinement.create()
    vr.fixedPointIterations, vr.sorIterations = 0, 3
    want = flow + np.float32(0)
    assert (np.signbit(flow) & (flow == 0)).any() and not (np.signbit(want) & (want == 0)).any()
    for b in range(B):                                   # (the oracle hands back its copy of W: -0 stays -0)
        _same_bits(np_ops.variational_refinement(fr[b], fr[b + 1], flow[b], 0, 3), flow[b], f"oracle, image {b}")
    d0, d1 = t.from_numpy(fr[:-1].copy()).cuda(), t.from_numpy(fr[1:].copy()).cuda()
    outer = np.full((B + 2, H, W, 2), SENTINEL, np.float32)
    for rounds in (32, 1, 0):
        outer[1:1 + B] = flow
        big = t.from_numpy(outer).cuda()
        vr.calc_batch_dev(d0, d1, big[1:1 + B], rounds=rounds)
        got = big.cpu().numpy()
        for b in range(B):
            _same_bits(got[1 + b], want[b], f"rounds {rounds}, image {b}")
        assert (got[0] == np.float32(SENTINEL)).all() and (got[-1] == np.float32(SENTINEL)).all()


# ----------------------------------------------------------------------------- 2. tf_farneback_batch
FB_DEFAULTS = dict(num_levels=5, pyr_scale=0.5, win_size=13, num_iters=10, poly_n=5, poly_sigma=1.1)
FB_SETS = {
    "default": {},
    "iters1": dict(num_iters=1), "iters2": dict(num_iters=2), "iters3": dict(num_iters=3), "iters7": dict(num_iters=7),
    "win9": dict(win_size=9), "win15": dict(win_size=15),
    "poly7": dict(poly_n=7, poly_sigma=1.5),
    "scale06": dict(pyr_scale=0.6), "scale08": dict(pyr_scale=0.8, num_levels=8),
    "levels0": dict(num_levels=0), "levels1": dict(num_levels=1),
}
# the pair against oracle_farneback: 0 = bit for bit, else the largest deviation allowed (the module contract of
# tests/test_gpu_parity.py: generic kernels within 1e-4 px; measured on these inputs: win 9 1.3e-5, win 15 7.2e-6 px)
FB_ORACLE_TOL = {
    "default": 0.0, "iters1": 0.0, "iters2": 0.0, "iters3": 0.0, "iters7": 0.0, "levels0": 0.0, "levels1": 0.0,
    "poly7": 0.0, "scale06": 0.0, "scale08": 0.0, "win9": 1e-4, "win15": 1e-4,
}
FB_SHAPES = [((203, 331), 5), ((96, 128), 2), ((31, 45), 4)]      # odd H * W; aligned; a single level (< 32 px at scale 0.5)
FB_LARGE = ((515, 777), 3)                                         # odd H * W, deep enough for pyramid level 4
FB_LARGE_SETS = ["default", "scale06"]
FB_CASES = [pytest.param(name, shape, B, id=f"{name}-{shape[0]}x{shape[1]}-B{B}") for name in FB_SETS for shape, B in FB_SHAPES] + \
           [pytest.param(name, FB_LARGE[0], FB_LARGE[1], id=f"{name}-{FB_LARGE[0][0]}x{FB_LARGE[0][1]}-B{FB_LARGE[1]}") for name in FB_LARGE_SETS]


def _fb_kw(name):
    return dict(FB_DEFAULTS, **FB_SETS[name])


def _fb_params(name):
    kw = _fb_kw(name)
    lib = _lib()
    return lib.FarnebackParams(kw["num_levels"], kw["pyr_scale"], kw["win_size"], kw["num_iters"], kw["poly_n"], kw["poly_sigma"],
                               lib.FB_CHAIN_DEFAULT, 0)


def _fb_levels(H, W, kw):
    """farneback.hip fb_levels"""
    k, scale = 0, 1.0
    while k < kw["num_levels"]:
        scale *= kw["pyr_scale"]
        if W * scale < 32 or H * scale < 32:
            break
        k += 1
    return k


def _fb_can_split(H, W, kw):
    """farneback.hip tf_farneback_can_split"""
    return _fb_levels(H, W, kw) >= 2 and kw["pyr_scale"] == 0.5


def _fb_lds_levels(H, W, kw):
    """the pyramid levels whose row blur takes k_fb_blur_rows_sampled_lds (farneback.hip fb_run_levels: a level that is
    neither full size nor an exact 2 x 2 area reduction, a blur longer than 5 taps, a source stride >= 12 and a source
    segment of <= FBL_ROW_BYTES = 4096 bytes per 64 outputs)"""
    out = []
    for k in range(_fb_levels(H, W, kw), -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= kw["pyr_scale"]
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(3, int(np.rint(sigma * 5)) | 1)
        w, h = int(np.rint(W * scale)), int(np.rint(H * scale))
        rsx, rsy = 1.0 / (w / W), 1.0 / (h / H)
        irx, iry = int(rsx + 0.5), int(rsy + 0.5)
        same = w == W and h == H
        eps = np.finfo(np.float64).eps
        area2 = not same and abs(rsx - irx) < eps and abs(rsy - iry) < eps and irx == 2 and iry == 2
        if same or area2:
            continue
        if ksize > 5 and rsx >= 12 and int(64 * rsx) + ksize + 8 <= 4096 and W >= ksize:
            out.append(k)
    return out


def _oracle_fb(a, b, kw):
    from oracle import _lib as ol
    Lo = ol.lib()
    Lo.oracle_farneback.restype = ctypes.c_int
    out = np.zeros(a.shape + (2,), np.float32)
    rc = Lo.oracle_farneback(ol.ptr(np.ascontiguousarray(a), ctypes.c_uint8), ol.ptr(np.ascontiguousarray(b), ctypes.c_uint8),
                             a.shape[0], a.shape[1], ol.ptr(out, ctypes.c_float), kw["num_levels"], ctypes.c_double(kw["pyr_scale"]),
                             kw["win_size"], kw["num_iters"], kw["poly_n"], ctypes.c_double(kw["poly_sigma"]))
    assert rc >= 0
    return out


def _fb_status_ok():
    """no row-sum chain of the iteration kernel starved in the launches so far (they would have left NaN rows)"""
    _torch().cuda.synchronize()
    assert _lib().lib().tf_farneback_check() == 0


@functools.lru_cache(maxsize=None)
def _fb_expected(name, H, W, B):
    """the frames of a (H, W, B) case and tf_farneback_pair on each of its pairs (forward, backward)"""
    t, lib = _torch(), _lib()
    L = lib.lib()
    fr = _frames(np.random.default_rng(H * 1000 + W), B + 1, H, W)
    fr.setflags(write=False)
    p = _fb_params(name)
    ws = _workspace(L.tf_farneback_workspace_bytes(H, W, ctypes.byref(p)))
    fwd, bwd = [], []
    for b in range(B):
        d0, d1 = t.from_numpy(fr[b].copy()).cuda(), t.from_numpy(fr[b + 1].copy()).cuda()
        f, k = (t.empty((H, W, 2), dtype=t.float32, device="cuda") for _ in range(2))
        lib.check(L.tf_farneback_pair(lib.ptr(d0), lib.ptr(d1), H, W, ctypes.byref(p), lib.ptr(f), lib.ptr(k), lib.ptr(ws), ws.numel(),
                                      lib.stream_ptr()), "tf_farneback_pair")
        fwd.append(f.cpu().numpy())
        bwd.append(k.cpu().numpy())
    _fb_status_ok()
    return fr, np.stack(fwd), np.stack(bwd)


def _fb_run(name, fr, B, img_stride, flow_stride, kind="batch", dirs=(True, True), parts=1, groups=None, fill=None):
    """one batched Farneback entry point on frames img_stride bytes apart (pair b: frames b and b + 1) into guarded flow
    buffers.  kind: "batch" (tf_farneback_batch), "split" (tf_farneback_batch_split, `parts`), "phase" (phase 1 for all
    pairs, then phase 2 for each (b0, b1) of `groups`).  Returns (fwd, bwd) host arrays, None for a direction not asked for."""
    lib = _lib()
    L = lib.lib()
    H, W = fr.shape[1:]
    p = _fb_params(name)
    if kind == "batch":
        nbytes = L.tf_farneback_workspace_bytes_batch(B, H, W, ctypes.byref(p))
    elif kind == "split":
        nbytes = L.tf_farneback_workspace_bytes_split(B, parts, H, W, ctypes.byref(p))
    else:
        nbytes = max(L.tf_farneback_workspace_bytes_phase(B, H, W, ctypes.byref(p), 1),
                     max(L.tf_farneback_workspace_bytes_phase(b1 - b0, H, W, ctypes.byref(p), 2) for b0, b1 in groups))
    assert nbytes > 0
    ws = _workspace(nbytes, fill)
    dimg = _dev_frames(fr, img_stride)
    out = [_FlowBuffer(B, H, W, flow_stride) if want else None for want in dirs]

    def optr(d, b):
        return out[d].ptr(b) if out[d] is not None else None

    common = (lib.ptr(ws), ws.numel(), lib.stream_ptr())
    if kind == "batch":
        lib.check(L.tf_farneback_batch(_at(dimg, 0), _at(dimg, img_stride), B, img_stride, H, W, ctypes.byref(p), optr(0, 0), optr(1, 0),
                                       flow_stride, *common), "tf_farneback_batch")
    elif kind == "split":
        lib.check(L.tf_farneback_batch_split(_at(dimg, 0), _at(dimg, img_stride), B, parts, img_stride, H, W, ctypes.byref(p), optr(0, 0),
                                             optr(1, 0), flow_stride, *common), "tf_farneback_batch_split")
    else:
        lib.check(L.tf_farneback_batch_phase(_at(dimg, 0), _at(dimg, img_stride), B, img_stride, H, W, ctypes.byref(p), optr(0, 0),
                                             optr(1, 0), flow_stride, *common, 1), "tf_farneback_batch_phase 1")
        for b0, b1 in groups:
            lib.check(L.tf_farneback_batch_phase(_at(dimg, b0 * img_stride), _at(dimg, (b0 + 1) * img_stride), b1 - b0, img_stride, H, W,
                                                 ctypes.byref(p), optr(0, b0), optr(1, b0), flow_stride, *common, 2), "tf_farneback_batch_phase 2")
    res = tuple(o.frames() if o is not None else None for o in out)
    _fb_status_ok()
    return res


def _fb_same_as_pairs(got, name, H, W, B, what):
    _, fwd, bwd = _fb_expected(name, H, W, B)
    for d, want in enumerate((fwd, bwd)):
        if got[d] is None:
            continue
        for b in range(B):
            _same_bits(got[d][b], want[b], f"{what}: {('forward', 'backward')[d]} flow of pair {b}")


@pytest.mark.parametrize("name,shape,B", FB_CASES)
def test_farneback_pair_against_the_oracle(name, shape, B):
    """tf_farneback_pair against oracle_farneback at the same parameters, both directions of every pair.  Bit for bit
    wherever the iteration is k_fb_iter (win_size 13), whatever num_iters and num_levels, and also through the generic
    expansion (poly_n 7) and the sampled blur + resize of pyr_scale 0.6 / 0.8 (k_fb_blur_rows_sampled*,
    k_fb_blur_cols_resize, with the LDS form at 515 x 777).  Within 1e-4 px (FB_ORACLE_TOL) for win_size 9 and 15: those
    run the unfused k_fb_update_matrices + k_fb_blur_solve, whose box filter sums the window in another order than
    OpenCV's running column sums."""
    H, W = shape
    kw = _fb_kw(name)
    fr, fwd, bwd = _fb_expected(name, H, W, B)
    tol = FB_ORACLE_TOL[name]
    for b in range(B):
        for got, (a, c), what in ((fwd[b], (fr[b], fr[b + 1]), "forward"), (bwd[b], (fr[b + 1], fr[b]), "backward")):
            want = _oracle_fb(a, c, kw)
            if tol == 0:
                _same_bits(got, want, f"{what} flow of pair {b} against the oracle")
            else:
                d = _max_dev(got, want)
                assert d <= tol, f"{what} flow of pair {b}: max abs {d} > {tol}"
    assert np.abs(fwd).max() > 0.5                         # the frames do move


@pytest.mark.parametrize("name,shape,B", FB_CASES)
def test_farneback_batch_equals_the_pairs(name, shape, B):
    """Every pair of tf_farneback_batch equals tf_farneback_pair, bit for bit, both directions: frames back to back
    (img_stride = H * W, odd at 203 x 331 and 515 x 777: pairs 1 .. B - 1 start at unaligned addresses) and at a stride
    of H * W + 3 into flow frames 2 * H * W + 6 floats apart (the gaps stay untouched); then with NULL for one direction,
    the other one equals that of the two-direction call."""
    H, W = shape
    fr = _fb_expected(name, H, W, B)[0]
    _fb_same_as_pairs(_fb_run(name, fr, B, H * W, 2 * H * W), name, H, W, B, "back to back")
    _fb_same_as_pairs(_fb_run(name, fr, B, H * W + 3, 2 * H * W + 6), name, H, W, B, "strided")
    for dirs in ((True, False), (False, True)):
        got = _fb_run(name, fr, B, H * W + 3, 2 * H * W + 6, dirs=dirs)
        assert (got[0] is None) != (got[1] is None)
        _fb_same_as_pairs(got, name, H, W, B, f"one direction {dirs}")


def test_farneback_large_batch_reaches_the_lds_blur_with_unaligned_frames():
    """515 x 777: pyramid level 4 (scale 0.5) and level 5 (scale 0.6) have a source stride >= 12, where the row blur stages
    its rows in LDS (k_fb_blur_rows_sampled_lds): aligned 32-bit words where the image base, the batch stride and W are
    multiples of four, bytes with reflected borders otherwise.  H * W is odd and W is no multiple of four, so in a batch of
    back-to-back frames every pair after the first takes the byte staging from an unaligned base.  The batch through the
    model's calc_batch_dev gives the pairs' bits (and so the oracle's, test_farneback_pair_against_the_oracle)."""
    t = _torch()
    from tobac_flow_amd.utils.flow_utils import FarnebackFlow
    (H, W), B = FB_LARGE
    assert (H * W) % 4 and W % 4
    for name in FB_LARGE_SETS:
        assert _fb_lds_levels(H, W, _fb_kw(name)), name
    assert not _fb_lds_levels(272, 544, _fb_kw("default"))          # (the largest shape of the chain-form test)
    fr = t.from_numpy(_fb_expected(FB_LARGE_SETS[0], H, W, B)[0].copy()).cuda()
    for name in FB_LARGE_SETS:
        m = FarnebackFlow(**_fb_kw(name))
        f, b = (t.empty((B, H, W, 2), dtype=t.float32, device="cuda") for _ in range(2))
        m.calc_batch_dev(fr[:-1], fr[1:], f, b)
        m.check_launches()
        _, fwd, bwd = _fb_expected(name, H, W, B)
        _same_bits(f.cpu().numpy(), fwd, f"{name}: forward flows of the batch")
        _same_bits(b.cpu().numpy(), bwd, f"{name}: backward flows of the batch")


# ----------------------------------------------------------------------------- 3. split and phase
SPLIT_CASES = [c for c in FB_CASES if _fb_can_split(*c.values[1], _fb_kw(c.values[0]))]


@pytest.mark.parametrize("name,shape,B", SPLIT_CASES)
def test_farneback_split_and_phase_equal_the_batch(name, shape, B):
    """tf_farneback_batch_split with parts 2 and B, and tf_farneback_batch_phase (phase 1 for all pairs, then phase 2 in two
    uneven groups, as create_flow does) give the pairs' flows bit for bit -- and so tf_farneback_batch's
    (test_farneback_batch_equals_the_pairs).  The split level's flow reaches phase 2 in the caller's frames whatever
    the parity of num_iters."""
    H, W = shape
    assert _lib().lib().tf_farneback_can_split(H, W, ctypes.byref(_fb_params(name))) == 1
    fr = _fb_expected(name, H, W, B)[0]
    for parts in (2, B):
        _fb_same_as_pairs(_fb_run(name, fr, B, H * W, 2 * H * W + 6, kind="split", parts=parts), name, H, W, B, f"split, parts {parts}")
    cut = B // 2
    _fb_same_as_pairs(_fb_run(name, fr, B, H * W, 2 * H * W + 6, kind="phase", groups=((0, cut), (cut, B))), name, H, W, B, "phase 1 + 2")


def test_farneback_split_of_other_pyramid_scales_is_the_unsplit_batch():
    """pyr_scale != 0.5 does not split (every coarse level is then not a sampled blur of the full-size frame): parts > 1 is
    accepted and silently gives the unsplit result, and the phase calls are refused"""
    (H, W), B = FB_SHAPES[0]
    lib = _lib()
    L = lib.lib()
    for name in ("scale06", "scale08"):
        assert _fb_levels(H, W, _fb_kw(name)) >= 2 and not _fb_can_split(H, W, _fb_kw(name))
        p = _fb_params(name)
        assert L.tf_farneback_can_split(H, W, ctypes.byref(p)) == 0
        assert L.tf_farneback_workspace_bytes_phase(B, H, W, ctypes.byref(p), 1) == 0
        fr = _fb_expected(name, H, W, B)[0]
        for parts in (2, B):
            _fb_same_as_pairs(_fb_run(name, fr, B, H * W, 2 * H * W, kind="split", parts=parts), name, H, W, B, f"split, parts {parts}")
        ws = _workspace(1 << 20)
        d = _torch().zeros(B * H * W * 4, dtype=_torch().float32, device="cuda")
        assert L.tf_farneback_batch_phase(lib.ptr(d), lib.ptr(d), B, H * W, H, W, ctypes.byref(p), lib.ptr(d), None, 2 * H * W,
                                          lib.ptr(ws), ws.numel(), lib.stream_ptr(), 1) == -1


# ----------------------------------------------------------------------------- 4. workspace contents
# Read before the first run of these tests: every workspace word that the library uses as an index, a ticket or a spin
# condition is written by the call before it is read, so a poisoned start can give wrong numbers but not a hang or a stray
# address.  tf_varref_batch: the workspace holds float planes only (D1, D2, S, A12, weights, dW and its partner).
# tf_farneback_batch / _split / _phase: the iteration kernel's ticket counters (the first FBI_HDR bytes of the blur scratch)
# and every pair's hand-over words are zeroed per level before its first launch (fb_run_levels, hipMemsetAsync); the rest
# is float planes, and the flows read from them are remapped with bounds checks (fb_matrix_at).  The status word of the
# starved-chain report is host memory, not workspace.
@pytest.mark.parametrize("fp", [0, 1, 3])
def test_varref_batch_output_does_not_depend_on_the_workspace(fp):
    """tf_varref_batch (3 images, tile path) with its workspace filled with 0.75, then with -3.0, before the call: both
    outputs equal tf_varref_ex image by image.  With fixed_point_iterations = 0 no iteration writes the update dW, and the
    call must zero it in every image's plane, not in the first one only."""
    H, W, B = 37, 53, 3
    fr, flow = _vr_inputs(H, W, B, 99 + fp)
    p, _ = _vr_params(fp, 3, {})
    want = _vr_single(fr, flow, p, 0, fill=POISON[0])
    if fp == 0:
        _same_bits(want, flow + np.float32(0), "tf_varref_ex without iterations")
    for fill in POISON:
        got = _vr_batch(fr, flow, p, 0, H * W, 2 * H * W, fill=fill)
        for b in range(B):
            _same_bits(got[b], want[b], f"workspace filled with {fill}: image {b}")


@pytest.mark.parametrize("kind", ["batch", "split", "phase"])
@pytest.mark.parametrize("name", ["default", "win9"])
def test_farneback_output_does_not_depend_on_the_workspace(kind, name):
    """tf_farneback_batch, _split (parts 2) and _phase (groups 2 + 3) on 5 pairs with the workspace filled with 0.75,
    then with -3.0, before the call: both give the pairs' flows bit for bit"""
    (H, W), B = FB_SHAPES[0]
    fr = _fb_expected(name, H, W, B)[0]
    for fill in POISON:
        got = _fb_run(name, fr, B, H * W, 2 * H * W, kind=kind, parts=2, groups=((0, 2), (2, B)), fill=fill)
        _fb_same_as_pairs(got, name, H, W, B, f"{kind}, workspace filled with {fill}")


# ----------------------------------------------------------------------------- 5. the reported workspace size is enough
GUARD = 4096
# (H, W, B, parameters away from the defaults)
EXACT_CASES = [pytest.param(131, 140, 3, {}, id="131x140-B3-default"),                          # two pyramid levels, parts 2 + 1, fused
               pytest.param(40, 47, 2, dict(pyr_scale=0.6, win_size=9), id="40x47-B2-scale06-win9"),   # no split; generic iteration with the M plane
               # (47 * 0.6 < 32 px: 40 x 47 has level 0 only.  This one has a level 1 of 36 x 42, whose sampled blur rows -- 2 * 60 * 42
               # floats -- are larger than the 60 * 70 plane)
               pytest.param(60, 70, 2, dict(pyr_scale=0.6, win_size=9), id="60x70-B2-scale06-win9"),
               pytest.param(33, 70, 1, {}, id="33x70-B1-default")]                              # one level


class _GuardedWorkspace:
    """`nbytes` of workspace with GUARD bytes of 0xA5 in front of it and behind it, in one allocation of the test's own: a
    library that writes beyond the size it reported hits a guard band, not somebody else's memory"""

    def __init__(self, nbytes, generous=False):
        t = _torch()
        self.nbytes = int(nbytes) * (4 if generous else 1)
        self.buf = t.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=t.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0

    def args(self):
        return _at(self.buf, GUARD), self.nbytes

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xA5).all())


def _fb_guarded_run(p, fr, B, kind, generous=False):
    """tf_farneback_batch / _split (parts 2) / _phase (1, then 2 for pairs 0 .. 1 and 2 .. B - 1) with, for every call, a
    workspace of exactly the bytes its size function reports (four times that: generous).  Returns the flows and the workspaces."""
    lib = _lib()
    L = lib.lib()
    H, W = fr.shape[1:]
    dimg = _dev_frames(fr, H * W)
    out = [_FlowBuffer(B, H, W, 2 * H * W) for _ in range(2)]
    used = []

    def call(fn, what, nbytes, b0, nb, *extra, parts=()):
        assert nbytes > 0, what
        used.append(_GuardedWorkspace(nbytes, generous))
        lib.check(fn(_at(dimg, b0 * H * W), _at(dimg, (b0 + 1) * H * W), nb, *parts, H * W, H, W, ctypes.byref(p), out[0].ptr(b0), out[1].ptr(b0),
                     2 * H * W, *used[-1].args(), lib.stream_ptr(), *extra), what)

    if kind == "batch":
        call(L.tf_farneback_batch, "tf_farneback_batch", L.tf_farneback_workspace_bytes_batch(B, H, W, ctypes.byref(p)), 0, B)
    elif kind == "split":
        call(L.tf_farneback_batch_split, "tf_farneback_batch_split", L.tf_farneback_workspace_bytes_split(B, 2, H, W, ctypes.byref(p)), 0, B, parts=(2,))
    else:
        call(L.tf_farneback_batch_phase, "tf_farneback_batch_phase 1", L.tf_farneback_workspace_bytes_phase(B, H, W, ctypes.byref(p), 1), 0, B, 1)
        for b0, b1 in ((0, 2), (2, B)):
            call(L.tf_farneback_batch_phase, "tf_farneback_batch_phase 2", L.tf_farneback_workspace_bytes_phase(b1 - b0, H, W, ctypes.byref(p), 2),
                 b0, b1 - b0, 2)
    res = out[0].frames(), out[1].frames()
    _fb_status_ok()
    return res, used


@pytest.mark.parametrize("H,W,B,over", EXACT_CASES)
def test_farneback_stays_inside_the_workspace_it_asks_for(H, W, B, over):
    """Every entry point gets a workspace of exactly the bytes its size function reports, 4096 bytes inside an allocation
    whose first and last 4096 bytes hold 0xA5: after the calls both guard bands are intact and the flows are those of
    the same batch on a workspace four times as large.  A geometry that does not split runs the unsplit batch for parts 2
    and reports no size for the phases."""
    lib = _lib()
    kw = dict(FB_DEFAULTS, **over)
    p = lib.FarnebackParams(kw["num_levels"], kw["pyr_scale"], kw["win_size"], kw["num_iters"], kw["poly_n"], kw["poly_sigma"], lib.FB_CHAIN_DEFAULT, 0)
    fr = _frames(np.random.default_rng(H * 1000 + W), B + 1, H, W)
    want, _ = _fb_guarded_run(p, fr, B, "batch", generous=True)
    assert np.abs(want[0]).max() > 0.1
    splits = bool(lib.lib().tf_farneback_can_split(H, W, ctypes.byref(p)))
    assert splits == _fb_can_split(H, W, kw) and (B >= 3 or not splits)
    if not splits:
        assert lib.lib().tf_farneback_workspace_bytes_phase(B, H, W, ctypes.byref(p), 1) == 0
    for kind in ("batch", "split") + (("phase",) if splits else ()):
        got, used = _fb_guarded_run(p, fr, B, kind)
        _torch().cuda.synchronize()
        for i, ws in enumerate(used):
            assert ws.intact(), f"{kind}: call {i} wrote outside the {ws.nbytes} bytes it asked for"
        for d in range(2):
            _same_bits(got[d], want[d], f"{kind} on an exact workspace: {('forward', 'backward')[d]} flows")
