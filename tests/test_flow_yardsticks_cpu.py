"""The C twins of the flow core (oracle/c/farneback.c, remap.c, varref.c) judged by the float64 yardsticks of
tests/flow_yardsticks.py, whose docstring derives every bound; the device is held to the same bounds in
tests/test_gpu_flow_yardsticks.py.  Three guards keep the yardsticks honest: each one, evaluated with one wrong parameter,
must refuse the twin on the same cases; the twin must use between 1/16 and all of every bound over the case set; and
profiles/flow_yardsticks.txt must record the ratios this file computes."""
import ctypes
import functools
import os

import numpy as np
import pytest

import flow_yardsticks as Y

F = ctypes.c_float
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flow_yardsticks.txt")


def _lib():
    from oracle import _lib as ol
    return ol, ol.lib()


# ---- the twin's stages ----------------------------------------------------------------------------------------------------
def twin_blur(img32, ksize, sigma):
    ol, L = _lib()
    img32 = np.ascontiguousarray(img32, np.float32)
    out = np.zeros_like(img32)
    L.oracle_gaussian_blur(ol.ptr(img32, F), img32.shape[0], img32.shape[1], int(ksize), ctypes.c_double(sigma), ol.ptr(out, F))
    return out


def twin_expansion(blur32, n, sigma):
    ol, L = _lib()
    blur32 = np.ascontiguousarray(blur32, np.float32)
    h, w = blur32.shape
    out = np.zeros((h, w, 5), np.float32)
    L.oracle_poly_exp(ol.ptr(blur32, F), h, w, ol.ptr(out, F), int(n), ctypes.c_double(sigma))
    return out


def twin_resize(src, dshape):
    ol, L = _lib()
    src = np.ascontiguousarray(src, np.float32)
    sh, sw, cn = src.shape
    out = np.zeros(tuple(dshape) + (cn,), np.float32)
    L.oracle_resize_linear(ol.ptr(src, F), sh, sw, cn, ol.ptr(out, F), int(dshape[0]), int(dshape[1]))
    return out


def twin_remap(img, flow, method):
    from oracle import np_ops
    return np_ops.warp_flow_single(np.ascontiguousarray(img), np.array(flow), method)


def _resize_source(sshape, cn):
    """cn = 1: a blurred frame (what the pyramid resizes); cn = 2: a flow field of a few pixels"""
    if cn == 1:
        return twin_blur(Y.frame(sshape, "noise", 5).astype(np.float32), 9, 1.5)[..., None]
    return Y.remap_flow(sshape, "amp6", 4)


@functools.lru_cache(maxsize=None)
def _blur_case(level, shape, content):
    ksize, sigma = Y.pyramid_blur_params(level)
    img = Y.frame(shape, content).astype(np.float32)
    value, bound = Y.blur_yardstick(img, ksize, sigma)
    return twin_blur(img, ksize, sigma), value, bound


# ---- 1. blur of the full-resolution level, polynomial expansion --------------------------------------------------------------
@pytest.mark.parametrize("content", Y.EXPANSION_CONTENTS)
@pytest.mark.parametrize("shape", Y.EXPANSION_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_resolution_blur_is_the_exact_binomial(shape, content):
    img = Y.frame(shape, content)
    assert np.array_equal(twin_blur(img.astype(np.float32), 3, 0.0), Y.blur3_yardstick(img))


def test_the_expansion_yardstick_returns_the_coefficients_of_a_quadratic():
    """the yardstick itself against the analytic answer, channel order included: (4, 3, 1, 1, -1) where r_y = 4, r_x = 3"""
    for n, sigma in (Y.DEFAULT_POLY, Y.OTHER_POLY):
        shape = (2 * n + 4, 2 * n + 6)
        q = dict(Y.QUADRATIC, c=0.3, xx=0.125, yy=-0.375, xy=0.0625)
        img, want = Y.quadratic_frame(shape, q), Y.quadratic_coefficients(shape, q)
        value, _ = Y.expansion_yardstick(img, n, sigma)
        inner = (slice(n, shape[0] - n), slice(n, shape[1] - n))
        assert np.abs(value - want)[inner].max() < 1e-10
    want = Y.quadratic_coefficients()
    y, x = np.argwhere((want[..., 0] == 4) & (want[..., 1] == 3))[0]
    assert want[y, x].tolist() == [4, 3, 1, 1, -1]


@pytest.mark.parametrize("n,sigma,content,shape", Y.expansion_cases(),
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_expansion_of_the_twin_is_the_least_squares_fit(n, sigma, content, shape):
    _, blur, value, bound = Y.expansion_reference(shape, content, n, sigma)
    ratio = Y.worst_ratio(twin_expansion(blur, n, sigma), value, bound)
    print(f"expansion n={n} {content} {shape}: error / bound = {ratio:.3f}")
    assert ratio <= 1


def test_expansion_of_the_twin_returns_the_quadratic_in_the_interior():
    n, sigma = Y.DEFAULT_POLY
    img = Y.quadratic_frame()
    assert img.min() >= 0 and img.max() <= 255 and np.array_equal(img, np.rint(img))
    img = img.astype(np.float32)                                # as an image in its own right: no blur here
    value, bound = Y.expansion_yardstick(img, n, sigma)
    want = Y.quadratic_coefficients()
    inner = (slice(n + 1, -n - 1), slice(n + 1, -n - 1))
    assert want[inner].size > 0
    assert Y.worst_ratio(twin_expansion(img, n, sigma)[inner], want[inner], bound[inner]) <= 1


# ---- 2. pyramid blur and resize ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ("noise", "checker"))
@pytest.mark.parametrize("shape", Y.BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("level", Y.PYRAMID_LEVELS)
def test_pyramid_blur_of_the_twin_is_the_gaussian_correlation(level, shape, content):
    got, value, bound = _blur_case(level, shape, content)
    ratio = Y.worst_ratio(got, value, bound)
    print(f"blur level {level} {content} {shape}: error / bound = {ratio:.3f}")
    assert ratio <= 1


def test_pyramid_blur_parameters():
    assert [Y.pyramid_blur_params(k) for k in Y.PYRAMID_LEVELS] == [(3, 0.5), (9, 1.5), (19, 3.5), (39, 7.5)]


@pytest.mark.parametrize("sshape,dshape,cn", Y.RESIZE_HALVINGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"cn{v}")
def test_halving_of_the_twin_is_the_block_mean(sshape, dshape, cn):
    src = _resize_source(sshape, cn)
    value, bound = Y.halving_yardstick(src)
    ratio = Y.worst_ratio(twin_resize(src, dshape), value, bound)
    print(f"halving {sshape} cn={cn}: error / bound = {ratio:.3f}")
    assert ratio <= 1


@pytest.mark.parametrize("sshape,dshape,cn", Y.RESIZE_BILINEAR, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"cn{v}")
def test_resize_of_the_twin_is_bilinear_at_pixel_centres(sshape, dshape, cn):
    src = _resize_source(sshape, cn)
    value, bound = Y.bilinear_yardstick(src, dshape)
    ratio = Y.worst_ratio(twin_resize(src, dshape), value, bound)
    print(f"bilinear {sshape} -> {dshape} cn={cn}: error / bound = {ratio:.3f}")
    assert ratio <= 1


# ---- 3. remap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,shape,kind", Y.remap_cases(), ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_remap_of_the_twin(method, shape, kind):
    img, flow, value, bound = Y.remap_reference(shape, kind, method)
    ratio = Y.worst_ratio(twin_remap(img, flow, method), value, bound)                  # NaN placement: exact, asserted inside
    print(f"remap {method} {shape} {kind}: error / bound = {ratio:.3f}")
    assert ratio <= 1


def test_the_remap_cases_hold_what_they_claim():
    """ties: 32 * coordinate ends in .5 everywhere, and rounds up about as often as down; last: integer coordinates on the last
    row and column, whose zero-weight tap beyond the image makes the linear result NaN; amp80: finite and NaN results both"""
    shape = (37, 53)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    f = Y.remap_flow(shape, "ties")
    c = (xx + f[..., 0].astype(np.float64)) * 32
    assert np.all(c - np.floor(c) == 0.5)
    up = np.rint(c) > c
    assert 0.3 < up.mean() < 0.7
    f = Y.remap_flow(shape, "last")
    on_last = (xx + f[..., 0] == shape[1] - 1) | (yy + f[..., 1] == shape[0] - 1)
    value = Y.remap_reference(shape, "last", "linear")[2]
    assert on_last.sum() > shape[0] * shape[1] // 2 and np.isnan(value[on_last]).all()
    inside = (xx + f[..., 0] < shape[1] - 1) & (yy + f[..., 1] < shape[0] - 1)
    assert inside.sum() >= 32 and np.isfinite(value[inside]).all()
    for method in Y.REMAP_METHODS:
        for kind in ("amp0.3", "amp6", "amp80", "ties"):
            value = Y.remap_reference(shape, kind, method)[2]
            assert np.isnan(value).any() and np.isfinite(value).sum() >= 32, (method, kind)


@pytest.mark.parametrize("method", Y.REMAP_METHODS)
@pytest.mark.parametrize("shape", Y.SMOOTH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_smooth_flow_step_of_the_twin(shape, method):
    from oracle import np_ops
    fwd, bwd, (fv, fb), (bv, bb) = Y.smooth_reference(shape, method)
    f2, b2 = np_ops.smooth_flow_step(fwd.copy(), bwd.copy(), method)
    ratio = max(Y.worst_ratio(f2, fv, fb), Y.worst_ratio(b2, bv, bb))
    print(f"smooth_flow_step {method} {shape}: error / bound = {ratio:.3f}")
    assert ratio <= 1


# ---- 4. refinement identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Y.VARREF_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_refinement_identities_of_the_twin(shape):
    from oracle import np_ops
    i0, i1, flow = Y.varref_frames(shape, "identical")
    out = np_ops.variational_refinement(i0, i1, flow)
    assert np.array_equal(out, np.zeros_like(out))
    i0, i1, flow = Y.varref_frames(shape, "constant")
    out = np_ops.variational_refinement(i0, i1, flow)
    assert out.tobytes() == flow.tobytes()


# ---- 5. guards -----------------------------------------------------------------------------------------------------------------
SENS_SHAPE = (40, 50)


def test_the_expansion_yardstick_refuses_a_wrong_sigma():
    n, sigma = Y.DEFAULT_POLY
    _, blur, value, bound = Y.expansion_reference(SENS_SHAPE, "noise", n, sigma)
    got = twin_expansion(blur, n, sigma)
    assert not Y.rejects(got, value, bound)
    assert Y.rejects(got, Y.expansion_yardstick(blur, n, 1.15)[0], bound)


def test_the_expansion_yardstick_refuses_a_reflected_border():
    n, sigma = Y.DEFAULT_POLY
    _, blur, value, bound = Y.expansion_reference(SENS_SHAPE, "noise", n, sigma)
    got = twin_expansion(blur, n, sigma)
    wrong = Y.expansion_yardstick(blur, n, sigma, border="reflect")[0]
    assert Y.rejects(got, wrong, bound)
    inner = (slice(n, -n), slice(n, -n))
    assert not Y.rejects(got[inner], wrong[inner], bound[inner])      # ... and only at the border: the interior is the same fit


@pytest.mark.parametrize("wrong", [dict(a=-0.5), dict(quantise="trunc"), dict(bins=64)], ids=["a=-0.5", "truncation", "64-bins"])
def test_the_remap_yardstick_refuses(wrong):
    methods = ("cubic",) if "a" in wrong else Y.REMAP_METHODS
    for method in methods:
        for kind in ("amp0.3", "amp6"):
            img, flow, value, bound = Y.remap_reference((37, 53), kind, method)
            got = twin_remap(img, flow, method)
            assert not Y.rejects(got, value, bound)
            assert Y.rejects(got, Y.remap_yardstick(img, flow, method, **wrong)[0], bound), (method, kind)


def test_the_resize_yardstick_refuses_pixel_corner_coordinates():
    for sshape, dshape, cn in (((333, 37), (166, 18), 1), ((21, 32), (41, 63), 2)):
        src = _resize_source(sshape, cn)
        value, bound = Y.bilinear_yardstick(src, dshape)
        got = twin_resize(src, dshape)
        assert not Y.rejects(got, value, bound)
        assert Y.rejects(got, Y.bilinear_yardstick(src, dshape, corner=True)[0], bound)


@functools.lru_cache(maxsize=None)
def twin_ratios():
    """{bound: the twin's worst error / bound over the case set}"""
    out = {}

    def note(name, ratio):
        out[name] = max(out.get(name, 0.0), ratio)
    for n, sigma, content, shape in Y.expansion_cases():
        _, blur, value, bound = Y.expansion_reference(shape, content, n, sigma)
        note(f"expansion_n{n}", Y.worst_ratio(twin_expansion(blur, n, sigma), value, bound))
    for level in Y.PYRAMID_LEVELS:
        for shape in Y.BLUR_SHAPES:
            for content in ("noise", "checker"):
                got, value, bound = _blur_case(level, shape, content)
                note(f"blur_k{Y.pyramid_blur_params(level)[0]}", Y.worst_ratio(got, value, bound))
    for sshape, dshape, cn in Y.RESIZE_HALVINGS:
        src = _resize_source(sshape, cn)
        note("resize_mean", Y.worst_ratio(twin_resize(src, dshape), *Y.halving_yardstick(src)))
    for sshape, dshape, cn in Y.RESIZE_BILINEAR:
        src = _resize_source(sshape, cn)
        note("resize_bilinear", Y.worst_ratio(twin_resize(src, dshape), *Y.bilinear_yardstick(src, dshape)))
    for method, shape, kind in Y.remap_cases():
        img, flow, value, bound = Y.remap_reference(shape, kind, method)
        note(f"remap_{method}", Y.worst_ratio(twin_remap(img, flow, method), value, bound))
    from oracle import np_ops
    for method in Y.REMAP_METHODS:
        for shape in Y.SMOOTH_SHAPES:
            fwd, bwd, (fv, fb), (bv, bb) = Y.smooth_reference(shape, method)
            f2, b2 = np_ops.smooth_flow_step(fwd.copy(), bwd.copy(), method)
            note(f"smooth_{method}", max(Y.worst_ratio(f2, fv, fb), Y.worst_ratio(b2, bv, bb)))
    return out


def derived_K():
    K = {f"expansion_n{n}": Y.expansion_K(n) for n, _ in (Y.DEFAULT_POLY, Y.OTHER_POLY)}
    K.update({f"blur_k{Y.pyramid_blur_params(k)[0]}": Y.blur_K(Y.pyramid_blur_params(k)[0]) for k in Y.PYRAMID_LEVELS})
    K.update(resize_mean=Y.RESIZE_K_MEAN, resize_bilinear=Y.RESIZE_K_BILINEAR)
    K.update({f"remap_{m}": Y.remap_K(m) for m in Y.REMAP_METHODS})
    K.update({f"smooth_{m}": Y.remap_K(m) / 2 + 1 for m in Y.REMAP_METHODS})
    return K


def read_profile():
    """{bound: (K, twin ratio, device ratio or None)} from the lines `name K twin device` of profiles/flow_yardsticks.txt"""
    rows = {}
    with open(PROFILE) as fh:
        for line in fh:
            p = line.split()
            if len(p) == 4 and p[0] in derived_K():
                rows[p[0]] = (float(p[1]), float(p[2]), None if p[3] == "-" else float(p[3]))
    return rows


@pytest.mark.parametrize("name", sorted(derived_K()))
def test_the_twin_uses_between_a_sixteenth_and_all_of_the_bound(name):
    ratio = twin_ratios()[name]
    print(f"{name}: K = {derived_K()[name]}, twin's worst error / bound = {ratio:.4f}")
    assert 1 / 16 <= ratio <= 1


@pytest.mark.parametrize("name", sorted(derived_K()))
def test_the_profile_records_these_figures(name):
    K, twin, device = read_profile()[name]
    assert abs(K - derived_K()[name]) < 0.06
    assert abs(twin - twin_ratios()[name]) <= 0.1 * twin_ratios()[name]
    assert device is None or device <= 1
