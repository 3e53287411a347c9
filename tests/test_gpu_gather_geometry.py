"""The semi-Lagrangian gather (csrc/convolve.hip + remap_dev.h) where its paths switch.

Every comparison is bit-exact against the numpy oracle (oracle/np_ops.py over oracle/c/remap.c), never against the
library.  The inputs come from tests/gather_cases.py; before anything is compared each test asserts with the classifier
of that module that its input reaches the classes it is there for (shared-patch path / per-tap path at each of the four
limits / taps that do not line up; inside / straddling / outside taps) with at least 32 pixels each -- the same
condition tests/test_gather_cases_cpu.py checks and prints without a GPU.

Each Sobel case is computed three ways which must all agree: the oracle, the dedicated 27-tap kernel (k_sobel27) and
the generic kernel (k_convolve, TF_SOBEL_GENERIC=1).  Volumes handed to the library are the middle slice of a tensor
with one spare frame at each end, so that a kernel that mistakes a border pixel for an interior one reads a wrong VALUE.
"""
import warnings
from functools import partial

import numpy as np
import pytest

import gather_cases as gc
from helpers import _eq

pytestmark = pytest.mark.gpu

METHODS = ("nearest", "linear", "cubic", "lanczos")
FILLS = (np.nan, -3.5, 0.0)
COMBOS = [(d, dt, fv) for d in (None, "uphill", "downhill") for dt in (None, np.float32) for fv in FILLS]
SPARE = 123.25                        # content of the spare frames: finite, unlike any field value


@pytest.fixture(scope="module")
def tf():
    import tobac_flow_amd.flow as flow
    return flow


def _quiet(f, *a, **k):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return f(*a, **k)


def _dev(a, spare=SPARE):
    """`a` on the device as the middle slice big[1:-1] of a tensor with one spare frame at each end"""
    import torch
    a = np.ascontiguousarray(a)
    big = torch.full((a.shape[0] + 2,) + a.shape[1:], spare if a.dtype.kind == "f" else int(spare),
                     dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    big[1:-1] = torch.from_numpy(a).cuda()
    return big[1:-1]


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _sobel3(tf, monkeypatch, case, method, direction, dtype, fill):
    """oracle == k_sobel27 == k_convolve for one Sobel case"""
    from oracle import np_ops
    data, fwd, bwd = case["data"], case["fwd"], case["bwd"]
    want = _quiet(np_ops.sobel, data, fwd, bwd, method=method, dtype=dtype, fill_value=fill, direction=direction)
    fl = tf.Flow(fwd, bwd)
    what = f"{case['name']} {method} {direction} {np.dtype(dtype or np.float64).name} fill={fill}"
    monkeypatch.delenv("TF_SOBEL_GENERIC", raising=False)
    got = _host(fl.sobel(_dev(data), method=method, dtype=dtype, fill_value=fill, direction=direction))
    monkeypatch.setenv("TF_SOBEL_GENERIC", "1")
    gen = _host(fl.sobel(_dev(data), method=method, dtype=dtype, fill_value=fill, direction=direction))
    monkeypatch.delenv("TF_SOBEL_GENERIC", raising=False)
    for name, g in (("k_sobel27", got), ("k_convolve", gen)):
        try:
            _eq(g, want)
        except AssertionError as e:
            raise AssertionError(f"{name} vs oracle, {what}: {e}") from None


def _tap_keys(fam, method):
    """the border branches of the per-tap remap a family reaches: an 8 x 8 lanczos footprint is outside only with the
    far flows and never inside a 6-pixel strip; nearest has no straddling taps"""
    if method == "nearest":
        return ("inside", "outside")
    if method == "lanczos":
        return {"far_outside": ("inside", "straddle", "outside"), "large_coordinates": ("straddle",)}.get(fam, ("inside", "straddle"))
    return ("inside", "straddle", "outside")


def _require(fam, method, plane_keys=()):
    """the coverage condition of this module: at least 32 pixels in every class the test is there for"""
    keys = _tap_keys(fam, method)
    if fam in ("border_sweep", "far_outside", "nearest_ties"):
        keys += tuple("miss_" + k for k in keys)                          # ... on the planes that read the all-fill frame too
    gc.require(gc.family_counts(fam, method), (plane_keys if method in ("linear", "cubic") else ()) + keys,
               f"{fam}, {method}")


# ----------------------------------------------------------------------------- Sobel
@pytest.mark.parametrize("method", METHODS)
def test_sobel_border_sweep_every_direction_dtype_and_fill(tf, monkeypatch, method):
    """(a): 5 shapes x 16 sets of k / 32 flows; every (direction, dtype, fill) occurs at least four times per method."""
    cases = gc.family("border_sweep")
    _require("border_sweep", method, gc.PLANE_KEYS)
    used = set()
    for i, case in enumerate(cases):
        combo = COMBOS[(i + 5 * METHODS.index(method)) % len(COMBOS)]
        used.add(combo)
        _sobel3(tf, monkeypatch, case, method, *combo)
    assert len(used) == len(COMBOS)


@pytest.mark.parametrize("method", METHODS)
def test_sobel_bin_ties(tf, monkeypatch, method):
    """(b): exact 1/32-px ties (half to even) and their neighbours; most pixels' taps do not line up."""
    cases = gc.family("bin_ties")
    _require("bin_ties", method, gc.PLANE_KEYS + ("unaligned",))
    for i, case in enumerate(cases):
        for combo in ((None, None, np.nan), ("uphill", np.float32, -3.5)) if i == 0 else (("downhill", None, 0.0),):
            _sobel3(tf, monkeypatch, case, method, *combo)


@pytest.mark.parametrize("method", METHODS)
def test_sobel_large_coordinates(tf, monkeypatch, method):
    """(c): x and y up to the ABI limit 32767, where the three taps' coordinates are rounded apart."""
    cases = gc.family("large_coordinates")
    _require("large_coordinates", method, gc.PLANE_KEYS + ("unaligned",))
    for i, case in enumerate(cases):
        _sobel3(tf, monkeypatch, case, method, *(("uphill", None, np.nan) if i == 0 else (None, np.float32, -3.5)))


@pytest.mark.parametrize("method", METHODS)
def test_sobel_nearest_ties_and_far_outside(tf, monkeypatch, method):
    """(d), (e): flows on exact halves; flows up to 1e6 px beside ordinary ones."""
    for fam in ("nearest_ties", "far_outside"):
        cases = gc.family(fam)
        _require(fam, method)
        for i, case in enumerate(cases):
            for j in range(3):
                _sobel3(tf, monkeypatch, case, method, *COMBOS[(7 * i + 5 * j + METHODS.index(method)) % len(COMBOS)])


@pytest.mark.parametrize("method", METHODS)
def test_sobel_field_values(tf, monkeypatch, method):
    """(f): plateaus and exact zeros, +-inf (inf - inf included), NaN blocks, 1e-30 / 1e30 / 3e38; every kind of field
    meets all three directions."""
    cases = gc.family("field_values")
    _require("field_values", method, gc.PLANE_KEYS)
    for i, case in enumerate(cases):
        kind = i % 6
        for j, direction in enumerate((None, "uphill", "downhill")):
            dtype = (None, np.float32)[(i // 6 + j + kind) % 2]
            fill = FILLS[(i // 6 + j + METHODS.index(method)) % 3]
            _sobel3(tf, monkeypatch, case, method, direction, dtype, fill)


@pytest.mark.parametrize("method", ["linear", "cubic"])
@pytest.mark.parametrize("fam", ["border_sweep", "bin_ties", "field_values"])
def test_fused_edge_field_against_the_oracle(tf, fam, method):
    """tf_sobel_edge_field against the oracle's uphill float64 Sobel followed by the reference's three elementwise lines
    (detection.py:638-642) in numpy float64, for float64 and float32 output."""
    import torch
    from oracle import np_ops
    from tobac_flow_amd import _lib
    L = _lib.lib()
    cases = gc.family(fam)
    _require(fam, method, gc.PLANE_KEYS + (("unaligned",) if fam == "bin_ties" else ()))
    for case in cases[::2] if fam == "border_sweep" else cases:
        field, fwd, bwd = case["data"], case["fwd"], case["bwd"]
        T, H, W = field.shape
        edges = _quiet(np_ops.sobel, field, fwd, bwd, method=method, dtype=None, fill_value=np.nan, direction="uphill")
        with np.errstate(all="ignore"):
            edges[edges > 0] += 1
            edges = edges - field
            edges[np.isnan(field)] = np.inf
        f, fw, bw = _dev(field), torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
        for dt, ty, ndt in ((torch.float64, _lib.TF_F64, np.float64), (torch.float32, _lib.TF_F32, np.float32)):
            out = torch.full(field.shape, SPARE, dtype=dt, device="cuda")
            _lib.check(L.tf_sobel_edge_field(_lib.ptr(f), T, H, W, _lib.ptr(fw), _lib.ptr(bw), _lib.INTERP[method],
                                             _lib.ptr(out), ty, _lib.stream_ptr()), "tf_sobel_edge_field")
            with np.errstate(all="ignore"):
                _eq(out.cpu().numpy(), edges.astype(ndt))


# ----------------------------------------------------------------------------- convolve
def _structures():
    """12 seeded 3 x 3 x 3 structures: five directed ones, seven random"""
    rng = np.random.default_rng(909)
    out = [np.zeros((3, 3, 3), bool) for _ in range(3)]
    out[0][0] = rng.random((3, 3)) < 0.6                    # plane 0 only
    out[0][0, 1, 1] = True
    out[1][2] = rng.random((3, 3)) < 0.6                    # plane 2 only
    out[1][2, 0, 2] = True
    out[2][0, 2, 0] = True                                  # a single tap
    s = rng.random((3, 3, 3)) < 0.5                         # centre absent
    s[1, 1, 1], s[0, 0, 0] = False, True
    out += [s, np.ones((3, 3, 3), bool)]                    # ... and all 27
    while len(out) < 12:
        s = rng.random((3, 3, 3)) < rng.uniform(0.15, 0.8)
        if s.any():
            out.append(s)
    return out


def _convolve_cases():
    sweep, fv = gc.family("border_sweep"), gc.family("field_values")
    first = [sweep[i * gc.SWEEP_VARIANTS + 3] for i in range(len(gc.SWEEP_SHAPES))]
    nan_inf = [c for c in fv if c["name"] in ("nan9x130", "nan70x7", "inf5x65", "plateau6x6")]
    return first + nan_inf + [gc.family("far_outside")[0], gc.family("nearest_ties")[1]]


@pytest.mark.parametrize("seed", range(12))
def test_convolve_structures_stack_nanmean_nanmax(tf, seed):
    """Random structures: the raw stack, nanmean (detection._nanmean0) and nanmax (TF_FUNC_NANMAX through convolve_dev)
    against the oracle's convolve with the numpy function, NaN and numeric fill, float32 and float64 stacks."""
    import torch
    import tobac_flow_amd.detection as det
    from oracle import np_ops
    from tobac_flow_amd import _lib
    from tobac_flow_amd.convolve import convolve_dev
    st = _structures()[seed]
    for ci, case in enumerate(_convolve_cases()):
        data, fwd, bwd = case["data"], case["fwd"], case["bwd"]
        method = METHODS[(seed + ci) % 4]
        fill = (np.nan, -3.5)[(seed // 4 + ci) % 2]
        dtype = (np.float32, np.float64)[(seed // 2 + ci) % 2]
        fl = tf.Flow(fwd, bwd)
        what = f"{case['name']} structure {seed} {method} fill={fill} {np.dtype(dtype).name}"
        try:
            _eq(_host(fl.convolve(_dev(data), structure=st, method=method, fill_value=fill, dtype=dtype)),
                np_ops.convolve(data, fwd, bwd, st, method, dtype, fill))
            want = _quiet(np_ops.convolve, data, fwd, bwd, st, method, dtype, fill, func=lambda x: np.nanmean(x, 0))
            _eq(_host(fl.convolve(_dev(data), structure=st, method=method, fill_value=fill, dtype=dtype, func=det._nanmean0)), want)
            want = _quiet(np_ops.convolve, data, fwd, bwd, st, method, dtype, fill, func=lambda x: np.nanmax(x, 0))
            fw, bw = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
            _eq(_host(convolve_dev(_dev(data), fw, bw, st, method, dtype, fill, func_code=_lib.FUNC_NANMAX)), want)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None


def test_nanmax_of_an_all_nan_stack_is_nan(tf):
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.convolve import convolve_dev
    shape = (3, 9, 70)
    data = np.ones(shape, np.float32)
    data[1] = np.nan
    data[1, 4, 30:40] = 2.0                                  # finite centres whose in-plane neighbours are all NaN
    st = np.zeros((3, 3, 3), bool)
    st[1, 0, 1] = st[1, 2, 1] = True                         # the pixel above and the pixel below
    z = torch.zeros(shape + (2,), device="cuda")
    got = _host(convolve_dev(_dev(data), z, z, st, "linear", np.float32, -1.0, func_code=_lib.FUNC_NANMAX))
    assert np.isnan(got[1, 4, 30:40]).all()                  # all-NaN stack -> NaN (np.nanmax), not the fill
    assert (got[1][np.isnan(data[1])] == -1.0).all() and (got[0] == 1.0).all() and (got[2] == 1.0).all()


@pytest.mark.parametrize("method", METHODS)
def test_diff_and_label_warps(tf, method):
    """Flow.diff on every family but the large one; int32 labels through nearest (stack and np.any) on (d), (e), (a)."""
    from oracle import np_ops
    for fam in ("border_sweep", "bin_ties", "nearest_ties", "far_outside", "field_values"):
        cases = gc.family(fam)
        for case in cases[METHODS.index(method)::4]:
            fl = tf.Flow(case["fwd"], case["bwd"])
            for dtype in (np.float32, np.float64):
                _eq(_host(fl.diff(_dev(case["data"]), method=method, dtype=dtype)),
                    _quiet(np_ops.diff, case["data"], case["fwd"], case["bwd"], method, dtype))
    if method != "nearest":
        return
    st = np.ones((3, 3, 3), bool)
    t_struct = np.zeros((3, 3, 3), bool)
    t_struct[:, 1, 1] = True
    for case in gc.family("nearest_ties") + gc.family("far_outside") + gc.family("border_sweep")[::8]:
        lab = gc.labels_of(case)
        fl = tf.Flow(case["fwd"], case["bwd"])
        _eq(_host(fl.convolve(_dev(lab), method="nearest", dtype=np.int32, structure=st, fill_value=0)),
            np_ops.convolve(lab, case["fwd"], case["bwd"], st, "nearest", np.int32, 0))
        m = (lab > 500).astype(np.int32)
        _eq(_host(fl.convolve(_dev(m), structure=t_struct, method="nearest", fill_value=False, dtype=np.int32,
                              func=partial(np.any, axis=0))),
            np_ops.convolve(m, case["fwd"], case["bwd"], t_struct, "nearest", np.int32, False, func=partial(np.any, axis=0)))


# ----------------------------------------------------------------------------- frame ranges
@pytest.mark.parametrize("generic", [False, True])
def test_frame_ranges_compose_to_the_whole_call(tf, monkeypatch, generic):
    """tf_convolve's [t0, t1): [0, k) and [k, T) into one sentinel-filled output equal the whole-range call (which equals
    the oracle) for every k of a T = 5 volume; t0 == t1 writes nothing.  Sobel (both kernels), nanmean, raw stack."""
    import torch
    from oracle import np_ops
    from tobac_flow_amd import _lib
    from tobac_flow_amd.convolve import convolve_dev
    from helpers import rand_field, rand_flow
    rng = np.random.default_rng(77)
    shape = (5, 9, 70)
    T = shape[0]
    data = rand_field(rng, shape, smooth=(0.5, 1, 1), nan_frac=0.02)
    fwd, bwd = rand_flow(rng, shape, 1.5), rand_flow(rng, shape, 1.5)
    fw, bw = torch.from_numpy(fwd).cuda(), torch.from_numpy(bwd).cuda()
    full = np.ones((3, 3, 3), bool)
    cross = np.zeros((3, 3, 3), bool)
    cross[:, 1, 1] = cross[1, :, 1] = cross[1, 1, :] = True
    if generic:
        monkeypatch.setenv("TF_SOBEL_GENERIC", "1")
    else:
        monkeypatch.delenv("TF_SOBEL_GENERIC", raising=False)
    sentinel = -777.0
    runs = [(full, _lib.FUNC_SOBEL_UPHILL, np.float64, "cubic",
             lambda: np_ops.sobel(data, fwd, bwd, "cubic", None, np.nan, "uphill")),
            (full, _lib.FUNC_SOBEL, np.float32, "linear",
             lambda: np_ops.sobel(data, fwd, bwd, "linear", np.float32, np.nan, None))]
    if not generic:
        runs += [(cross, _lib.FUNC_NANMEAN, np.float32, "linear",
                  lambda: np_ops.convolve(data, fwd, bwd, cross, "linear", np.float32, np.nan, func=lambda x: np.nanmean(x, 0))),
                 (cross, _lib.FUNC_STACK, np.float32, "cubic",
                  lambda: np_ops.convolve(data, fwd, bwd, cross, "cubic", np.float32, np.nan))]
    for st, code, dtype, method, oracle in runs:
        whole = _host(convolve_dev(_dev(data), fw, bw, st, method, dtype, np.nan, code))
        _eq(whole, _quiet(oracle))
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        for k in range(T + 1):
            out = torch.full(whole.shape, sentinel, dtype=tdt, device="cuda")
            convolve_dev(_dev(data), fw, bw, st, method, dtype, np.nan, code, t0=k, t1=k, out=out)
            assert (out == sentinel).all(), f"t0 == t1 == {k} wrote something"
            convolve_dev(_dev(data), fw, bw, st, method, dtype, np.nan, code, t0=0, t1=k, out=out)
            part = _host(out)
            frames = part if code != _lib.FUNC_STACK else np.moveaxis(part, 1, 0)
            assert (frames[k:] == sentinel).all(), f"[0, {k}) wrote beyond frame {k}"
            convolve_dev(_dev(data), fw, bw, st, method, dtype, np.nan, code, t0=k, t1=T, out=out)
            _eq(_host(out), whole)


# ----------------------------------------------------------------------------- warp_flow / smooth_flow_step
def _frames(fam):
    cases = gc.family(fam)
    if fam == "border_sweep":
        cases = cases[::3]
    for case in cases:
        for t in range(case["data"].shape[0]):
            yield f"{case['name']}[{t}]", case["data"][t], case["fwd"][t], case["bwd"][t]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fam", ["border_sweep", "bin_ties", "large_coordinates", "nearest_ties", "far_outside"])
def test_warp_and_smooth_single_frames(tf, fam, method):
    """k_warp and k_smooth (sample_flow2) on the frames of (a) - (e): in the smoothing step the sampled image is the other
    flow, so both flows carry the directed values; tf_smooth_flow_step_clip equals the clip of the unclipped result."""
    import torch
    from oracle import np_ops
    from tobac_flow_amd import _lib
    L = _lib.lib()
    _require(fam, method)
    maxv = 1.25
    for name, img, f, b in _frames(fam):
        try:
            _eq(tf.warp_flow(img, f, method), np_ops.warp_flow_single(img, f, method))
            _eq(tf.warp_flow(img, b, method), np_ops.warp_flow_single(img, b, method))
            gf, gb = tf.smooth_flow_step(f, b, method)
            wf, wb = _quiet(np_ops.smooth_flow_step, f, b, method)
            _eq(gf, wf)
            _eq(gb, wb)
            H, W = f.shape[:2]
            fd, bd = torch.from_numpy(f).cuda(), torch.from_numpy(b).cuda()
            fo, bo = torch.empty_like(fd), torch.empty_like(bd)
            _lib.check(L.tf_smooth_flow_step_clip(_lib.ptr(fd), _lib.ptr(bd), H, W, _lib.INTERP[method], _lib.ptr(fo),
                                                  _lib.ptr(bo), maxv, _lib.stream_ptr()), "tf_smooth_flow_step_clip")
            _eq(fo.cpu().numpy(), np.minimum(np.maximum(wf, np.float32(-maxv)), np.float32(maxv)))
            _eq(bo.cpu().numpy(), np.minimum(np.maximum(wb, np.float32(-maxv)), np.float32(maxv)))
        except AssertionError as e:
            raise AssertionError(f"{name} {method}: {e}") from None
