"""k_vr_system forms the seven derivative planes itself from the {avg, Iz} plane k_vr_prepare writes (csrc/varref.hip).

Every case asserts array_equal against the oracle's C restatement (oracle.np_ops.variational_refinement), no tolerances:
  - image borders, where the clamp acts twice in the second differences (shapes down to 1 x 1);
  - the seams of the system kernel's 128 x 8 tile, its interior-column path (tiles whose columns lie two pixels inside the
    image: W >= 258) next to the clamped one, and one shape that also crosses a seam of the 108 x 84 SOR tile;
  - frames with 0 / 255 checkerboards (the largest derivative magnitudes) and flat regions (exact zeros), flows of a few
    pixels that push warps out of the image;
  - 1, 2 and 5 fixed-point iterations (the first runs without dW), the fused and the per-half-sweep SOR path, and none;
  - a batch of three images on padded planes with a strided flow array, and workspaces filled with NaN / 0x5a bytes.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TW, TH = 128, 8                                         # VRS_TW, VRS_TH of csrc/varref.hip
BORDER_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (4, 5), (5, 4), (5, 5)]
SEAM_SHAPES = [(h, w) for w in (TW - 1, TW, TW + 1, 2 * TW + 1) for h in (TH - 1, TH, TH + 1, 2 * TH + 1)]
# 85 x 109 crosses the SOR tile's seams too; from W = 2 TW + 2 on, tile column 1 takes the interior-column path
OTHER_SHAPES = [(85, 109), (TH + 1, 2 * TW + 2), (2 * TH + 3, 3 * TW + 3)]
SHAPES = BORDER_SHAPES + SEAM_SHAPES + OTHER_SHAPES
# (fixed_point_iterations, sor_iterations): (2, 6) takes one launch per half sweep, which reads the same S / A12 / wt
ITERATIONS = [(1, 5), (2, 5), (5, 5), (2, 6), (0, 5)]


def _lib():
    from tobac_flow_amd import _lib as lib
    return lib


def _torch():
    import torch
    return torch


def _inputs(H, W, B, seed):
    """B + 1 uint8 frames (image b refines frame b -> b + 1) of noise with a 0 / 255 checkerboard whose phase flips from
    frame to frame, a region that is flat and equal in all frames, one flat 0 and one flat 255; flows of a few pixels"""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, size=(B + 1, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    h2, w2, h4, w4 = (H + 1) // 2, (W + 1) // 2, (H + 3) // 4, (W + 3) // 4
    for i in range(B + 1):
        fr[i, :h2, :w2] = (((yy + xx + i) & 1) * 255)[:h2, :w2]
        fr[i, h2:, w2:] = 93
        fr[i, h2:h2 + h4, :w4] = 0 if i % 2 == 0 else 255
        fr[i, :h4, w2:w2 + w4] = 255
    flow = (rng.normal(size=(B, H, W, 2)) * 3.0).astype(np.float32)
    flow[rng.random((B, H, W)) < 0.02] = 0.0
    return np.ascontiguousarray(fr), flow


def _params(fp, sor):
    return _lib().VarRefParams(fp, sor, 20.0, 5.0, 10.0, 1.6)


def _workspace(nbytes, fill=None):
    t = _torch()
    ws = t.empty((int(nbytes) + 255) // 256 * 256, dtype=t.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill) if isinstance(fill, int) else ws.view(t.float32).fill_(fill)
    return ws


def _single(i0, i1, flow, fp, sor):
    t, lib = _torch(), _lib()
    L = lib.lib()
    H, W = flow.shape[:2]
    p = _params(fp, sor)
    ws = _workspace(L.tf_varref_workspace_bytes(H, W))
    d0, d1, f = t.from_numpy(i0.copy()).cuda(), t.from_numpy(i1.copy()).cuda(), t.from_numpy(flow.copy()).cuda()
    lib.check(L.tf_varref_ex(lib.ptr(d0), lib.ptr(d1), H, W, ctypes.byref(p), lib.ptr(f), 0, lib.ptr(ws), ws.numel(),
                             lib.stream_ptr()), "tf_varref_ex")
    return f.cpu().numpy()


def _batch(fr, flow, fp, sor, fill=None):
    """tf_varref_batch on B images at once; the flows are frames 1 .. B of a (B + 2, H, W + 1, 2) array, so the flow stride
    exceeds 2 H W and the other words must stay as they were"""
    t, lib = _torch(), _lib()
    L = lib.lib()
    B, H, W = flow.shape[:3]
    p = _params(fp, sor)
    stride = 2 * H * (W + 1)
    host = np.full((B + 2) * stride, 1234.5, np.float32)
    for b in range(B):
        host[(1 + b) * stride:(1 + b) * stride + 2 * H * W] = flow[b].ravel()
    big = t.from_numpy(host).cuda()
    d0, d1 = t.from_numpy(fr[:-1].copy()).cuda(), t.from_numpy(fr[1:].copy()).cuda()
    nbytes = L.tf_varref_workspace_bytes_batch(B, H, W)
    plane = (H * W + 63) // 64 * 64 if B > 1 else H * W
    assert nbytes <= 48 * plane * B + 6 * 256 + 4096, "more than 48 B of workspace per pixel and image"
    ws = _workspace(nbytes, fill)
    lib.check(L.tf_varref_batch(lib.ptr(d0), lib.ptr(d1), B, H * W, H, W, ctypes.byref(p),
                                ctypes.c_void_p(big.data_ptr() + 4 * stride), stride, 0, lib.ptr(ws), ws.numel(),
                                lib.stream_ptr()), "tf_varref_batch")
    out = big.cpu().numpy()
    inside = np.zeros(out.size, bool)
    for b in range(B):
        inside[(1 + b) * stride:(1 + b) * stride + 2 * H * W] = True
    assert (out[~inside] == np.float32(1234.5)).all(), "words outside the output frames changed"
    return np.stack([out[(1 + b) * stride:(1 + b) * stride + 2 * H * W].reshape(H, W, 2) for b in range(B)])


@pytest.mark.parametrize("fp,sor", ITERATIONS, ids=[f"fp{a}-sor{b}" for a, b in ITERATIONS])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_system_from_sources_equals_the_oracle(shape, fp, sor):
    from oracle import np_ops
    H, W = shape
    fr, flow = _inputs(H, W, 1, 1000 * H + W)
    got = _single(fr[0], fr[1], flow[0], fp, sor)
    want = np_ops.variational_refinement(fr[0], fr[1], flow[0], fp, sor)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} values differ"


@pytest.mark.parametrize("fp", [1, 5])
@pytest.mark.parametrize("shape", [(85, 109), (2 * TH + 1, 2 * TW + 3)], ids=["85x109", "17x259"])
def test_batch_on_padded_planes_equals_the_single_image_and_the_oracle(shape, fp):
    from oracle import np_ops
    H, W = shape
    B = 3
    assert (H * W) % 64 != 0
    fr, flow = _inputs(H, W, B, 77 * H + W)
    got = _batch(fr, flow, fp, 5)
    for b in range(B):
        one = _single(fr[b], fr[b + 1], flow[b], fp, 5)
        want = np_ops.variational_refinement(fr[b], fr[b + 1], flow[b], fp, 5)
        assert np.array_equal(got[b], one), f"image {b}: batch against the single-image call"
        assert np.array_equal(got[b], want), f"image {b}: batch against the oracle"


@pytest.mark.parametrize("B", [1, 3])
def test_output_does_not_depend_on_the_workspace(B):
    from oracle import np_ops
    H, W = 2 * TH + 1, 2 * TW + 3
    fr, flow = _inputs(H, W, B, 5 + B)
    a = _batch(fr, flow, 5, 5, fill=float("nan"))
    b = _batch(fr, flow, 5, 5, fill=0x5a)
    assert np.array_equal(a, b)
    for i in range(B):
        assert np.array_equal(a[i], np_ops.variational_refinement(fr[i], fr[i + 1], flow[i], 5, 5)), f"image {i}"
