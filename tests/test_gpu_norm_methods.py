"""The normalisation methods of calculate_flow on the device (normalise_pair_dev, tf_norm8_pair) against the reference's own
bytes in tests/golden/norm_ref*.npz: equal for the exact class, under the fixed cap for the rounding class
(tests/norm_cases.py; tests/test_norm_cases_cpu.py shows that a numpy model of the device arithmetic and the kernel
bodies compiled for the host stay under the same cap on every case used here)."""
import numpy as np
import pytest

import norm_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tf():
    import tobac_flow_amd.flow as flow
    return flow


@pytest.fixture(scope="module")
def golden():
    return nc.golden()


@pytest.fixture(scope="module")
def dev():
    from tobac_flow_amd import _lib
    return lambda a: _lib.to_dev(np.ascontiguousarray(a))


def _run(method, pair, dev, **kw):
    from tobac_flow_amd.utils.normalisation_utils import normalise_pair_dev
    o0, o1 = normalise_pair_dev(method, dev(pair[0]), dev(pair[1]), **kw)
    return np.stack([o0.cpu().numpy(), o1.cpu().numpy()])


@pytest.mark.parametrize("name", list(nc.cases()))
def test_device_bytes_against_the_reference(golden, dev, name):
    c = golden[name]
    got = _run(c["method"], c["pair"], dev, **c["kwargs"])
    nc.hold(got, c["want"], c["exact"], name)
    again = _run(c["method"], c["pair"], dev, **c["kwargs"])
    assert np.array_equal(got, again), "two runs differ"


def test_linear_without_arguments_is_the_existing_kernel(golden, dev):
    from tobac_flow_amd.utils.normalisation_utils import linear_norm, to_8bit, to_8bit_pair_dev
    pair = nc.fields()["nan_one"]
    got = _run("linear", pair, dev)
    o0, o1 = to_8bit_pair_dev(dev(pair[0]), dev(pair[1]))
    assert np.array_equal(got, np.stack([o0.cpu().numpy(), o1.cpu().numpy()]))
    assert np.array_equal(got, to_8bit(linear_norm(pair.copy()), 0, 1))
    # the general entry computes the same bytes when it is asked for linear without bounds
    from tobac_flow_amd import _lib
    t, L = _lib.torch(), _lib.lib()
    H, W = pair.shape[1:]
    p = _lib.NormParams()
    L.tf_norm8_default_params(p)
    assert (p.max_std, p.quantiles, p.size, p.flags) == (3.0, 256, 100, 0)
    a, b = dev(pair[0]), dev(pair[1])
    out = _lib.empty((2, H, W), t.uint8)
    ws = _lib.empty((L.tf_norm8_workspace_bytes(H, W, 0, p),), t.uint8)
    assert L.tf_norm8_pair(_lib.ptr(a), _lib.ptr(b), H, W, 0, p, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws), ws.numel(),
                           _lib.stream_ptr()) == 0
    assert np.array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("method,kw", [("linear", {"vmin": 220, "vmax": 280}), ("z_score", {}), ("local_linear", {"size": 7}),
                                       ("uniform", {"quantiles": 64})])
def test_out_views_are_written_in_place(dev, method, kw):
    from tobac_flow_amd import _lib
    from tobac_flow_amd.utils.normalisation_utils import normalise_pair_dev
    t = _lib.torch()
    pair = nc.fields()["smooth_odd"]
    H, W = pair.shape[1:]
    buf = t.full((5, H, W), 0x55, dtype=t.uint8, device=_lib.device())
    o0, o1 = normalise_pair_dev(method, dev(pair[0]), dev(pair[1]), out=(buf[3], buf[1]), **kw)
    assert o0.data_ptr() == buf[3].data_ptr() and o1.data_ptr() == buf[1].data_ptr()
    host = buf.cpu().numpy()
    assert (host[[0, 2, 4]] == 0x55).all()
    assert np.array_equal(host[[3, 1]], _run(method, pair, dev, **kw))


def test_c_entry_rejects_bad_arguments(dev):
    from tobac_flow_amd import _lib
    t, L = _lib.torch(), _lib.lib()
    pair = nc.fields()["smooth_odd"]
    H, W = pair.shape[1:]
    a, b = dev(pair[0]), dev(pair[1])
    out = _lib.empty((2, H, W), t.uint8)
    out.fill_(7)
    p = _lib.NormParams()
    L.tf_norm8_default_params(p)
    ws = _lib.empty((L.tf_norm8_workspace_bytes(H, W, 5, p),), t.uint8)

    def call(method, params, f0=a, f1=b, o0=out[0], o1=out[1], w=ws, nbytes=None, shape=(H, W)):
        return L.tf_norm8_pair(_lib.ptr(f0), _lib.ptr(f1), shape[0], shape[1], method, params, _lib.ptr(o0), _lib.ptr(o1),
                               _lib.ptr(w), w.numel() if nbytes is None and w is not None else (nbytes or 0), _lib.stream_ptr())

    EINVAL, ENOMEM = -1, -2
    for null in ("f0", "f1", "o0", "o1", "w"):
        assert call(3, p, **{null: None}) == EINVAL and b"null" in L.tf_last_error()
    assert call(3, None) == EINVAL
    for method in (-1, 6, 99):
        assert call(method, p) == EINVAL and b"unknown method" in L.tf_last_error()
        assert L.tf_norm8_workspace_bytes(H, W, method, p) == 0
    assert call(3, p, shape=(0, W)) == EINVAL and call(3, p, shape=(H, -1)) == EINVAL
    bad = _lib.NormParams()
    for field, value, method, word in (("size", 0, 5, b"size"), ("size", -3, 5, b"size"), ("quantiles", 0, 4, b"quantiles"),
                                       ("quantiles", 1025, 4, b"quantiles"), ("quantiles", 3000, 4, b"quantiles")):
        L.tf_norm8_default_params(bad)
        setattr(bad, field, value)
        assert call(method, bad) == EINVAL and word in L.tf_last_error(), (field, value)
        assert L.tf_norm8_workspace_bytes(H, W, method, bad) == 0
    for method in range(6):
        need = L.tf_norm8_workspace_bytes(H, W, method, p)
        assert 0 < need <= ws.numel() or method == 4
        big = ws if method != 4 else _lib.empty((need,), t.uint8)
        assert call(method, p, w=big, nbytes=need - 1) == ENOMEM and b"workspace" in L.tf_last_error()
        assert call(method, p, w=big, nbytes=256) == ENOMEM
    t.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()                       # no rejected call wrote anything
    # the Python layer: TypeError for a keyword the host call would not take, ValueError where only the host form computes it
    from tobac_flow_amd.utils.normalisation_utils import normalise_pair_dev
    with pytest.raises(TypeError):
        normalise_pair_dev("z_score", a, b, vmin=0)
    with pytest.raises(ValueError):
        normalise_pair_dev("linear", a, b, vmin=np.float64(230.0))
    with pytest.raises(ValueError):
        normalise_pair_dev("uniform", a, b, quantiles=2048)
    nan = a.clone()
    nan[3, 4] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        normalise_pair_dev("uniform", nan, b)
    with pytest.raises(ValueError):
        normalise_pair_dev("log", a, b[:-1])
    with pytest.raises(ValueError):
        normalise_pair_dev("log", pair[0], pair[1])               # host arrays


# ---- through calculate_flow -------------------------------------------------------------------------------------------
def _stack():
    base = nc.fields()["smooth_mid"][0]
    return np.stack([np.roll(base, (i, -2 * i), (0, 1)) for i in range(3)]).astype(np.float32)


def _forbid_host_glue(monkeypatch, tf, method):
    from tobac_flow_amd.utils import normalisation_utils as nu

    def boom(*args, **kwargs):
        raise AssertionError("the host glue ran for a device tensor")
    monkeypatch.setattr(nu, "to_8bit", boom)
    monkeypatch.setattr(tf, "to_8bit", boom)
    monkeypatch.setitem(nu.NORMALISATION_METHODS, method, boom)


FLOW_CASES = [("linear", {"vmin": 215, "vmax": 290.5}, True), ("linear", {"vmax": np.float32(280)}, True), ("log", {}, True),
              ("inverse_log", {}, False), ("inverse_log", {"vmin": -1}, False), ("z_score", {}, False), ("z_score", {"max_std": 2}, False),
              ("uniform", {}, True), ("uniform", {"quantiles": 64}, True), ("local_linear", {"size": 25}, True),
              ("local_linear", {}, True)]


@pytest.mark.parametrize("method,kw,exact", FLOW_CASES)
def test_calculate_flow_stays_on_the_device(tf, dev, monkeypatch, method, kw, exact):
    from tobac_flow_amd.utils.normalisation_utils import normalise_pair_dev
    stack = _stack()
    host = tf.calculate_flow(stack, "Farneback", normalisation_method=method, **kw) if exact else None
    d = dev(stack)
    with monkeypatch.context() as m:
        _forbid_host_glue(m, tf, method)
        fwd, bwd = tf.calculate_flow(d, "Farneback", normalisation_method=method, **kw)
    assert fwd.is_cuda and bwd.is_cuda
    fwd, bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    model = tf.select_of_model("Farneback")
    for i in range(2):
        p0, p1 = normalise_pair_dev(method, d[i], d[i + 1], **kw)
        f, b = tf.calculate_flow_frame(p0, p1, model)
        assert np.array_equal(fwd[i], f.cpu().numpy()) and np.array_equal(bwd[i + 1], b.cpu().numpy()), (method, i)
    if exact:
        assert np.array_equal(fwd, host[0], equal_nan=True) and np.array_equal(bwd, host[1], equal_nan=True)


@pytest.mark.parametrize("kw,poison", [({}, True), ({"quantiles": 2048}, False)])
def test_uniform_outside_the_device_form_takes_the_host_glue(tf, dev, kw, poison):
    stack = _stack()
    if poison:
        stack[1, 20, 30] = np.nan
    want = tf.calculate_flow(stack, "Farneback", normalisation_method="uniform", **kw)
    got = tf.calculate_flow(dev(stack), "Farneback", normalisation_method="uniform", **kw)
    assert np.array_equal(got[0].cpu().numpy(), want[0], equal_nan=True)
    assert np.array_equal(got[1].cpu().numpy(), want[1], equal_nan=True)


@pytest.mark.parametrize("method,kw", [("local_linear", {"size": 10}), ("z_score", {})])
def test_calculate_flow_2_on_two_device_stacks(tf, dev, monkeypatch, method, kw):
    from tobac_flow_amd.utils.normalisation_utils import normalise_pair_dev
    a = _stack()
    b = np.roll(a, (1, 2), (1, 2)).copy()
    da, db = dev(a), dev(b)
    with monkeypatch.context() as m:
        _forbid_host_glue(m, tf, method)
        fwd, bwd = tf.calculate_flow_2(da, db, "Farneback", normalisation_method=method, **kw)
    model = tf.select_of_model("Farneback")
    for i in range(a.shape[0] - 1):
        p0, p1 = normalise_pair_dev(method, da[i], db[i], **kw)
        f, bk = tf.calculate_flow_frame(p0, p1, model)
        assert np.array_equal(fwd[i].cpu().numpy(), f.cpu().numpy()) and np.array_equal(bwd[i + 1].cpu().numpy(), bk.cpu().numpy())
