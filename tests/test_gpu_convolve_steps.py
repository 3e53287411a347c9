"""The step-level convolve API (warp_flow, convolve_same_step, convolve_step: tf_warp_offsets / tf_gather_offsets /
tf_convolve_step of csrc/convolve.hip) on the GPU, bit for bit against the numpy oracle (oracle/np_ops.py over
oracle/c/remap.c).  Shapes are small and deliberately no multiple of the 64 x 4 block; every comparison is
helpers._eq (array_equal with NaNs equal, dtype and shape included)."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

from helpers import _eq, rand_field, rand_flow

pytestmark = pytest.mark.gpu

METHODS = ("nearest", "linear", "cubic", "lanczos")
TAP_CAP = 32                            # TF_STEP_TAP_CAP of csrc/convolve.hip: taps per launch
H, W = 37, 53
NINE = np.stack(np.meshgrid(np.arange(-1, 2), np.arange(-1, 2)), -1).reshape(-1, 2)
FRACTIONAL = np.array([[0.5, -1.25], [2.75, 0.03125]])


def _grid(h, w, x0=0, y0=0):
    return np.stack(np.meshgrid(np.arange(w) + x0, np.arange(h) + y0), -1)


def _flow(rng, h, w, amp):
    return rand_flow(rng, (1, h, w), amp)[0]


def _field(rng, h, w, nan_frac=0.015):
    f = rand_field(rng, (h, w), smooth=(1.5, 1.5))
    f.ravel()[rng.choice(h * w, int(round(nan_frac * h * w)), replace=False)] = np.nan      # 1.5 % NaNs, exactly
    return f


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _quiet(f, *a, **k):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return f(*a, **k)


@pytest.fixture(scope="module")
def cv():
    import tobac_flow_amd.convolve as c
    return c


@pytest.fixture(scope="module")
def ops():
    from oracle import np_ops
    return np_ops


@pytest.fixture(scope="module")
def base():
    rng = np.random.default_rng(20)
    long = rng.integers(-96, 97, (2 * TAP_CAP + 3, 2)) / 32.0          # more than two launches' worth, on the 1/32 px raster
    assert len(long) > TAP_CAP
    img = _field(rng, H, W)
    assert 0.01 < np.isnan(img).mean() < 0.02
    return {
        "img": img,
        "flow": {2: _flow(rng, H, W, 2), 80: _flow(rng, H, W, 80)},
        "offsets": {"default": None, "nine": NINE, "fractional": FRACTIONAL, "long": long},
        "labels": rng.integers(0, 6, (H, W)).astype(np.int32),
    }


# ---- warp_flow ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", ["default", "nine", "fractional", "long"])
@pytest.mark.parametrize("amp", [2, 80])
@pytest.mark.parametrize("method", METHODS)
def test_warp_flow_matches_oracle(cv, ops, base, method, amp, offsets):
    img, flow, offs = base["img"], base["flow"][amp], base["offsets"][offsets]
    kw = {} if offs is None else {"offsets": offs}
    for fill in (np.nan, -7.5):
        want = ops.warp_flow_multi(img, flow, method, fill, grid_locs=_grid(H, W), **kw)
        if amp == 80 and method != "lanczos":
            outside = (want == fill) if fill == fill else np.isnan(want)
            assert outside.mean() > 0.25                               # many taps leave the image
        got = cv.warp_flow(img, flow, method=method, fill_value=fill, **kw)
        assert got.shape == ((1 if offs is None else len(offs)), H, W)
        _eq(got, want)
        _eq(cv.warp_flow(img, flow, method=method, fill_value=fill, grid_locs=_grid(H, W), **kw), want)


@pytest.mark.parametrize("shape", [(2, 3), (3, 9), (7, 7)])
@pytest.mark.parametrize("method", METHODS)
def test_warp_flow_images_smaller_than_the_footprint(cv, ops, method, shape):
    """smaller than the cubic (4 x 4) / Lanczos (8 x 8) footprint: every sample takes the border path"""
    rng = np.random.default_rng(21)
    h, w = shape
    img, flow = _field(rng, h, w, nan_frac=0.0), _flow(rng, h, w, 1)
    offs = np.concatenate([NINE, FRACTIONAL])
    for fill in (np.nan, -7.5):
        want = ops.warp_flow_multi(img, flow, method, fill, offs, _grid(h, w))
        _eq(cv.warp_flow(img, flow, method=method, fill_value=fill, offsets=offs), want)


@pytest.fixture(scope="module")
def crop():
    """a (20, 24) cut at (x0, y0) = (11, 5) of the (37, 53) frame; for the full-frame run the frame is the bottom right
    corner of a large image, so that its pixel (0, 0) sits at (X0, Y0) = (5000, 5000) of that image"""
    import torch
    rng = np.random.default_rng(22)
    frame = _field(rng, H, W)
    X0 = Y0 = 5000
    big = np.zeros((Y0 + H, X0 + W), np.float32)
    big[Y0:, X0:] = frame
    return {"frame": frame, "x0": 11, "y0": 5, "h": 20, "w": 24, "flow": _flow(rng, 20, 24, 2), "X0": X0, "Y0": Y0,
            "big": big, "big_dev": torch.from_numpy(big).cuda(),
            "offsets": np.concatenate([NINE, FRACTIONAL, [[22.5, 16.25], [-3.0, 2.0]]])}


@pytest.mark.parametrize("method", METHODS)
def test_warp_flow_crop_with_local_grid(cv, ops, crop, method):
    c = crop
    cut = np.ascontiguousarray(c["frame"][c["y0"]:c["y0"] + c["h"], c["x0"]:c["x0"] + c["w"]])
    grid = _grid(c["h"], c["w"])
    want = ops.warp_flow_multi(cut, c["flow"], method, np.nan, c["offsets"], grid)
    _eq(cv.warp_flow(cut, c["flow"], method=method, offsets=c["offsets"], grid_locs=grid), want)
    _eq(cv.warp_flow(cut, c["flow"], method=method, offsets=c["offsets"], grid_locs=grid.astype(np.float64)), want)


@pytest.mark.parametrize("method", METHODS)
def test_warp_flow_crop_with_full_frame_grid(cv, ops, crop, method):
    """grid_locs in the coordinates of the large image (around 5000): the coordinate is rounded to float32 at that
    magnitude.  The oracle gets the region of the large image from `halo` pixels before the frame to the image's end and
    that region's origin: right and bottom are the image's true border, and no footprint reaches the region's left or top
    edge (asserted), so the two must agree everywhere."""
    c = crop
    halo = 16
    ox, oy = c["X0"] - halo, c["Y0"] - halo
    region = np.ascontiguousarray(c["big"][oy:, ox:])
    reach = float(np.abs(c["flow"]).max()) + 3 + 4                     # flow + most negative offset + Lanczos footprint
    assert reach < min(c["x0"], c["y0"]) + halo
    grid = _grid(c["h"], c["w"], c["X0"] + c["x0"], c["Y0"] + c["y0"])
    want = ops.warp_flow_multi(region, c["flow"], method, np.nan, c["offsets"], grid, origin=(ox, oy))
    assert np.isnan(want[-2]).mean() > 0.2                             # the far offset leaves the image
    got = cv.warp_flow(c["big_dev"], c["flow"], method=method, offsets=c["offsets"], grid_locs=grid)
    _eq(_host(got), want)
    # the rounding at 5000 is not the rounding at 0: the same cut with local coordinates differs somewhere
    local = ops.warp_flow_multi(c["frame"], c["flow"], method, np.nan, c["offsets"], _grid(c["h"], c["w"], c["x0"], c["y0"]))
    if method != "nearest":
        assert not np.array_equal(np.nan_to_num(local), np.nan_to_num(want))


@pytest.mark.parametrize("method", METHODS)
def test_warp_flow_image_larger_than_the_flow(cv, ops, method):
    rng = np.random.default_rng(23)
    img, flow = _field(rng, 40, 60), _flow(rng, 16, 70, 2)
    want = ops.warp_flow_multi(img, flow, method, np.nan, NINE, None)
    got = cv.warp_flow(img, flow, method=method, offsets=NINE)
    assert got.shape == (9, 16, 70)
    _eq(got, want)


def test_warp_flow_integer_labels(cv, ops, base):
    lab = base["labels"]
    for amp in (2, 80):
        want = ops.warp_flow_multi(lab, base["flow"][amp], "nearest", 0, NINE, _grid(H, W))
        got = cv.warp_flow(lab, base["flow"][amp], method="nearest", fill_value=0, offsets=NINE)
        assert got.dtype == np.int32
        _eq(got, want)
    _eq(cv.warp_flow(lab.astype(np.int64), base["flow"][2], method="nearest", fill_value=0, offsets=NINE),
        ops.warp_flow_multi(lab, base["flow"][2], "nearest", 0, NINE, _grid(H, W)))
    with pytest.raises(ValueError):
        cv.warp_flow(lab, base["flow"][2], method="linear", fill_value=0)


# ---- convolve_same_step ------------------------------------------------------------------------------
SEVEN = np.stack(np.meshgrid(np.arange(-3, 4), np.arange(-3, 4)), -1).reshape(-1, 2)     # 49 offsets: two launches


@pytest.mark.parametrize("kind", ["float32", "int32"])
def test_convolve_same_step_matches_oracle(cv, ops, base, kind):
    img = base["img"] if kind == "float32" else base["labels"]
    fills = (np.nan, -7.5) if kind == "float32" else (0, -1)
    assert len(SEVEN) > TAP_CAP
    cut_grid = _grid(20, 24, 11, 5)
    edge_grid = _grid(9, 70, -8, 30)                                   # hangs over the image on three sides
    for fill in fills:
        for grid in (None, cut_grid, edge_grid):
            vals, oob = ops.convolve_same_step(img, SEVEN, fill, _grid(H, W) if grid is None else grid)
            assert not oob.all() and (oob.any() or grid is cut_grid)      # the cut lies inside the image, the others do not
            want = vals.copy()
            want[oob] = fill
            got = cv.convolve_same_step(img, SEVEN, fill_value=fill, grid_locs=grid)
            assert got.shape == (49,) + ((H, W) if grid is None else grid.shape[:2])
            _eq(got, want)
    _eq(cv.convolve_same_step(img, SEVEN.astype(np.float64), fill_value=fills[1]),      # integral floats are accepted
        cv.convolve_same_step(img, SEVEN, fill_value=fills[1]))


# ---- convolve_step -----------------------------------------------------------------------------------
def _structures():
    out = {f"connectivity{k}": ndi.generate_binary_structure(3, k) for k in (1, 2, 3)}
    s = ndi.generate_binary_structure(3, 2)
    out["no_backward"] = s * np.array([0, 1, 1], bool)[:, None, None]
    out["no_forward"] = s * np.array([1, 1, 0], bool)[:, None, None]
    out["column"] = np.ones((3, 1, 1), bool)
    out["ones_3x5"] = np.ones((3, 3, 5), bool)
    out["ones_5x3"] = np.ones((3, 5, 3), bool)
    return out


STRUCTURES = _structures()
STEP_CASES = [(m, s) for s in STRUCTURES for m in ("nearest", "linear", "cubic")] + [("lanczos", "connectivity1")]
SH, SW = 33, 41


@pytest.fixture(scope="module")
def frames():
    """three independently allocated frames (no views of one volume) and the two flows of the middle one"""
    rng = np.random.default_rng(24)
    f = {k: _field(rng, SH, SW) for k in ("prev", "same", "next")}
    assert f["prev"].base is None and f["same"].base is None and f["next"].base is None
    f["fwd"], f["bwd"] = _flow(rng, SH, SW, 2), _flow(rng, SH, SW, 2)
    f["labels"] = [rng.integers(0, 5, (SH, SW)).astype(np.int32) for _ in range(3)]
    return f


@pytest.mark.parametrize("method,structure", STEP_CASES)
def test_convolve_step_matches_oracle(cv, ops, frames, method, structure):
    f, s = frames, STRUCTURES[structure]
    grid = _grid(SH, SW)
    for dtype in (np.float32, np.float64):
        for fill in (np.nan, -7.5):
            want = ops.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], s, method, dtype, fill, grid)
            got = cv.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], structure=s, method=method,
                                   dtype=dtype, fill_value=fill)
            assert got.shape == (np.count_nonzero(s), SH, SW)
            _eq(got, want)
    got = cv.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], structure=s, method=method, grid_locs=grid)
    _eq(got, ops.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], s, method, np.float32, np.nan, grid))


@pytest.mark.parametrize("end", ["prev", "next"])
@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
def test_convolve_step_with_an_all_fill_end_frame(cv, ops, frames, method, end):
    """the reference's loop hands an all-fill frame of the OUTPUT dtype to the step at either end of the sequence
    (convolve.py:307-314); a finite fill is interpolated like any other constant image"""
    f, s = frames, ndi.generate_binary_structure(3, 3)
    for dtype in (np.float32, np.float64):
        for fill in (np.nan, -7.5):
            fr = dict(f)
            fr[end] = np.full((SH, SW), fill, dtype=dtype)
            want = ops.convolve_step(fr["prev"], fr["same"], fr["next"], f["fwd"], f["bwd"], s, method, dtype, fill, _grid(SH, SW))
            got = cv.convolve_step(fr["prev"], fr["same"], fr["next"], f["fwd"], f["bwd"], structure=s, method=method,
                                   dtype=dtype, fill_value=fill)
            _eq(got, want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_convolve_step_integer_labels(cv, ops, frames, k):
    p, c, n = frames["labels"]
    s = ndi.generate_binary_structure(3, k)
    want = ops.convolve_step(p, c, n, frames["fwd"], frames["bwd"], s, "nearest", np.int32, 0, _grid(SH, SW))
    got = cv.convolve_step(p, c, n, frames["fwd"], frames["bwd"], structure=s, method="nearest", dtype=np.int32, fill_value=0)
    assert got.dtype == np.int32
    _eq(got, want)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_stacked_steps_equal_convolve(cv, method, k):
    """the reference's own loop (convolve.py:305-345) over convolve_step == the fused convolve(func=None)"""
    rng = np.random.default_rng(25)
    T, h, w = 4, 33, 41
    data = rand_field(rng, (T, h, w), nan_frac=0.01)
    fwd, bwd = rand_flow(rng, (T, h, w), 2), rand_flow(rng, (T, h, w), 2)
    s = ndi.generate_binary_structure(3, k)
    for fill in (np.nan, -7.5):
        want = cv.convolve(data, fwd, bwd, structure=s, method=method, dtype=np.float32, fill_value=fill, func=None)
        got = np.empty_like(want)
        blank = np.full((h, w), fill, dtype=np.float32)
        for i in range(T):
            out = cv.convolve_step(blank if i == 0 else data[i - 1], data[i], blank if i == T - 1 else data[i + 1],
                                   fwd[i], bwd[i], structure=s, method=method, dtype=np.float32, fill_value=fill,
                                   res=got[:, i], grid_locs=_grid(h, w))
            assert out.shape == (np.count_nonzero(s), h, w)
        _eq(got, want)


# ---- containers --------------------------------------------------------------------------------------
def test_res_is_written_and_returned(cv, ops, base, frames):
    img, flow = base["img"], base["flow"][2]
    want = ops.warp_flow_multi(img, flow, "cubic", np.nan, NINE, _grid(H, W))
    res = np.zeros((9, H, W), np.float64)
    assert cv.warp_flow(img, flow, method="cubic", offsets=NINE, res=res) is res
    _eq(res, want.astype(np.float64))
    vals, oob = ops.convolve_same_step(img, NINE, -7.5, _grid(H, W))
    vals[oob] = -7.5
    res = np.zeros((9, H, W), np.float32)
    assert cv.convolve_same_step(img, NINE, fill_value=-7.5, res=res) is res
    _eq(res, vals)
    f = frames
    s = ndi.generate_binary_structure(3, 2)
    want = ops.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], s, "linear", np.float64, np.nan, _grid(SH, SW))
    res = np.zeros(want.shape, np.float64)
    out = cv.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], structure=s, method="linear", res=res)
    assert out is res                                                   # res' dtype stands in for dtype=
    _eq(res, want)


def test_device_tensors_in_device_tensors_out(cv, base, frames):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    img, flow = base["img"], base["flow"][80]
    host = cv.warp_flow(img, flow, method="cubic", offsets=FRACTIONAL, fill_value=-7.5)
    got = cv.warp_flow(dev(img), dev(flow), method="cubic", offsets=FRACTIONAL, fill_value=-7.5)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    _eq(_host(got), host)
    host = cv.convolve_same_step(img, NINE, grid_locs=_grid(20, 24, 40, 30))
    got = cv.convolve_same_step(dev(img), NINE, grid_locs=dev(_grid(20, 24, 40, 30)))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    _eq(_host(got), host)
    f = frames
    s = ndi.generate_binary_structure(3, 3)
    host = cv.convolve_step(f["prev"], f["same"], f["next"], f["fwd"], f["bwd"], structure=s, method="cubic", dtype=np.float64)
    args = [dev(f[k]) for k in ("prev", "same", "next", "fwd", "bwd")]
    got = cv.convolve_step(*args, structure=s, method="cubic", dtype=np.float64)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    _eq(_host(got), host)
    res = torch.zeros((27, SH, SW), dtype=torch.float64, device="cuda")
    where = res.data_ptr()
    out = cv.convolve_step(*args, structure=s, method="cubic", res=res)
    assert out is res and res.data_ptr() == where
    _eq(_host(res), host)


def test_abi_argument_checks():
    """the checks of tf_convolve, ahead of any launch: null pointers, extents < 2^15, int32 data needs nearest, empty
    structure.  Every buffer is large enough for the shape the call names."""
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    n = 1 << 15
    buf = [torch.zeros(n * 4 * 2, dtype=torch.float32, device="cuda") for _ in range(5)]
    a, b, c, fl, out = (_lib.ptr(x) for x in buf)
    offs = np.zeros((1, 2), np.float32)
    ioffs = np.zeros((1, 2), np.int32)
    o, io = offs.ctypes.data_as(ctypes.c_void_p), ioffs.ctypes.data_as(ctypes.c_void_p)
    struct = np.zeros(27, np.uint8)
    st = struct.ctypes.data_as(ctypes.c_void_p)
    err = lambda: L.tf_last_error().decode()   # noqa: E731
    EINVAL = -1
    assert L.tf_warp_offsets(None, 0, 4, 4, fl, None, 4, 4, o, 1, 1, 0.0, out, 0, None) == EINVAL and "null pointer" in err()
    assert L.tf_warp_offsets(a, 0, 4, 4, fl, None, 4, 4, o, 1, 1, 0.0, None, 0, None) == EINVAL and "null pointer" in err()
    assert L.tf_warp_offsets(a, 0, 4, n, fl, None, 4, 4, o, 1, 1, 0.0, out, 0, None) == EINVAL and "bad shape" in err()
    assert L.tf_warp_offsets(a, 0, 4, 4, fl, None, n, 4, o, 1, 1, 0.0, out, 0, None) == EINVAL and "bad shape" in err()
    assert L.tf_warp_offsets(a, 0, 4, 4, fl, None, 0, 4, o, 1, 1, 0.0, out, 0, None) == EINVAL and "bad shape" in err()
    assert L.tf_warp_offsets(a, 2, 4, 4, fl, None, 4, 4, o, 1, 1, 0.0, out, 2, None) == EINVAL and "int32 data needs nearest" in err()
    assert L.tf_warp_offsets(a, 0, 4, 4, fl, None, 4, 4, o, 0, 1, 0.0, out, 0, None) == EINVAL
    assert L.tf_gather_offsets(None, 0, 4, 4, None, 4, 4, io, 1, 0.0, out, 0, None) == EINVAL and "null pointer" in err()
    assert L.tf_gather_offsets(a, 0, 4, 4, None, 4, n, io, 1, 0.0, out, 0, None) == EINVAL and "bad shape" in err()
    assert L.tf_convolve_step(a, b, c, 0, 4, 4, fl, fl, None, st, 3, 3, 1, 0.0, out, 0, None) == EINVAL and "empty structure" in err()
    struct[4] = 1                              # one backward tap: prev and bwd are needed, next and fwd are not
    assert L.tf_convolve_step(None, b, c, 0, 4, 4, fl, fl, None, st, 3, 3, 1, 0.0, out, 0, None) == EINVAL and "null pointer" in err()
    assert L.tf_convolve_step(a, b, c, 0, 4, 4, fl, None, None, st, 3, 3, 1, 0.0, out, 0, None) == EINVAL and "null pointer" in err()
    assert L.tf_convolve_step(a, b, c, 2, 4, 4, fl, fl, None, st, 3, 3, 2, 0.0, out, 2, None) == EINVAL and "int32 data needs nearest" in err()
    assert L.tf_convolve_step(a, b, c, 0, n, 4, fl, fl, None, st, 3, 3, 1, 0.0, out, 0, None) == EINVAL and "bad shape" in err()
    assert L.tf_convolve_step(a, None, None, 0, 4, 4, None, fl, None, st, 3, 3, 1, 0.0, out, 0, None) == 0
    torch.cuda.synchronize()
