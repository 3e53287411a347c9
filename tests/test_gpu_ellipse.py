"""The 3-D distance transform with a time sampling on the GPU (validation.get_marker_distance_ellipse_dev,
ndimage_dev.distance_transform_edt / edt_time_envelope and the C ABI of tf_edt_time_envelope) against the reference's own
results (tests/golden/ellipse_ref.npz), SciPy and brute force, under the contract of tests/ellipse_cases.py: the reported
voxel is a feature, the distance is SciPy's expression for it bit for bit and within 4 eps of the brute-force minimum,
both equal SciPy's and the reference's wherever one feature lies within 4 eps of the minimum (everywhere, for an integer
sampling), the closest marker is the value there, and two runs are identical."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import ellipse_cases as ec
import validation_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def host(x):
    return x.cpu().numpy()


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def transform(lib, name, sname):
    from tobac_flow_amd import ndimage_dev
    x = lib.to_dev(ec.VOLUMES[name]() == 0)                       # SciPy measures the distance to the nearest ZERO of its input
    return ndimage_dev.distance_transform_edt(x, sampling=(ec.sampling(sname), 1, 1), return_indices=True)


@pytest.mark.parametrize("name,sname", ec.CASES)
def test_marker_distance_ellipse_keeps_the_contract_against_the_reference(lib, name, sname):
    from tobac_flow_amd import validation as v
    markers = ec.VOLUMES[name]()
    margin, time_margin = ec.SAMPLINGS[sname]
    dist_t, closest_t = v.get_marker_distance_ellipse_dev(lib.to_dev(markers), time_margin, margin)
    assert lib.is_tensor(dist_t) and lib.is_tensor(closest_t)
    dist, closest = host(dist_t), host(closest_t)
    indices = host(transform(lib, name, sname)[1])                # the voxel the same two kernels report
    exempt, differing = ec.check(name, sname, dist, indices, closest)                                # points 1 - 6
    print(f"{name} at {sname}: {exempt} voxels with several features within 4 eps, {differing} of them differ from SciPy")
    dist_n, closest_n = v.get_marker_distance_ellipse_dev(markers, time_margin, margin)              # NumPy in, NumPy out
    assert isinstance(dist_n, np.ndarray) and isinstance(closest_n, np.ndarray)
    same(dist_n, dist)                                                                               # (7)
    same(closest_n, closest)
    again = v.get_marker_distance_ellipse_dev(lib.to_dev(markers), time_margin, margin)
    assert np.array_equal(host(again[0]), dist) and np.array_equal(host(again[1]), closest)
    if name == "none":
        assert np.isposinf(dist).all() and not closest.any() and (indices == -1).all()
    if name == "full":
        assert not dist.any() and np.array_equal(indices, np.indices(markers.shape)) and np.array_equal(closest, markers)
    if name == "gap":                                             # the empty frame is filled from its neighbours
        assert np.isfinite(dist[3]).all() and (indices[0, 3] != 3).all() and (dist[3] >= ec.sampling(sname)).all()


@pytest.mark.parametrize("name,sname", [(v, s) for v, s in ec.CASES if v != "none"])
def test_distance_transform_edt_against_scipy(lib, name, sname):
    from tobac_flow_amd import ndimage_dev
    markers, s = ec.VOLUMES[name](), ec.sampling(sname)
    x = markers == 0
    xd = lib.to_dev(x)
    want, want_indices = ndi.distance_transform_edt(x, sampling=(s, 1, 1), return_indices=True)
    dist_t, indices_t = ndimage_dev.distance_transform_edt(xd, sampling=(s, 1, 1), return_indices=True)
    dist, indices = host(dist_t), host(indices_t)
    ec.check(name, sname, dist, indices)
    one = ec.brute_force(name, sname)["count"] == 1
    assert np.array_equal(dist[one], want[one]) and np.array_equal(indices[:, one], want_indices[:, one])
    if sname in ec.INTEGER_SAMPLINGS:
        assert np.array_equal(dist, want)
    same(host(ndimage_dev.distance_transform_edt(xd, sampling=(s, 1, 1))), dist)                      # without indices: the same
    same(host(ndimage_dev.distance_transform_edt(xd, sampling=(s, 1, 1), return_distances=False, return_indices=True)), indices)
    if sname == "1":
        same(host(ndimage_dev.distance_transform_edt(xd)), dist)
        same(host(ndimage_dev.distance_transform_edt(xd, sampling=1)), dist)


def test_a_frame_goes_to_the_frames_path_and_one_frame_volumes_equal_scipy(lib):
    """T = 1: no other frame, A = 0, the sum is the integer d2.  vc.wide() is the product's row length"""
    from tobac_flow_amd import ndimage_dev
    for markers in (vc.wide(), ec.tiny()):
        x = markers == 0
        want, want_indices = ndi.distance_transform_edt(x[0], return_indices=True)
        for s in (10 / 3, 0.3):
            dist, indices = ndimage_dev.distance_transform_edt(lib.to_dev(x), sampling=(s, 1, 1), return_indices=True)
            same(host(dist)[0], want)
            assert (host(indices)[0] == 0).all()
            assert np.array_equal(ec.at_indices(host(indices), s), host(dist))
        dist2, indices2 = ndimage_dev.distance_transform_edt(lib.to_dev(x[0]), return_indices=True)
        assert tuple(dist2.shape) == x.shape[1:] and tuple(indices2.shape) == (2,) + x.shape[1:]
        same(host(dist2), want)
        same(host(indices2), host(indices)[1:, 0])
        same(host(ndimage_dev.distance_transform_edt(lib.to_dev(x[0]))), want)
        same(host(ndimage_dev.distance_transform_edt(lib.to_dev(x[0]), sampling=(1, 1), return_distances=False, return_indices=True)),
             host(indices2))
    one = ndi.distance_transform_edt(ec.tiny()[0] == 0, return_indices=True)[1]
    same(host(indices2), one.astype(np.int32))                    # two features: no pixel of the (5, 7) frame is equally near both


def test_scan_runs_the_whole_of_t_at_a_small_sampling_and_stops_early_at_a_large_one(lib):
    """(40, 9, 11), features in frames 0 and 39 only, 38 frames without one between them.  At s = 0.3 the whole of t is
    11.7 pixels long, no longer than the frame is wide: the scans pass through every empty frame, and the farther end wins
    where its feature is nearer in the plane.  At s = 3 one frame outweighs the whole plane (8^2 + 10^2 < 3^2 (20^2 - 19^2)):
    the nearer end wins everywhere, and next to an end the scan stops after a few frames"""
    markers = ec.ends()
    for sname in ("0.3", "3"):
        dist, indices = (host(a) for a in transform(lib, "ends", sname))
        ec.check("ends", sname, dist, indices)
        assert set(np.unique(indices[0])) == {0, 39}
        want = ndi.distance_transform_edt(markers == 0, sampling=(ec.sampling(sname), 1, 1))
        if sname == "3":
            assert np.array_equal(dist, want)
            assert (indices[0, :20] == 0).all() and (indices[0, 20:] == 39).all()
        else:
            assert (indices[0, :19] == 39).any() and (indices[0, 21:] == 0).any()
            one = ec.brute_force("ends", sname)["count"] == 1
            assert np.array_equal(dist[one], want[one])


def test_a_huge_sampling_leaves_every_frame_with_a_feature_to_itself(lib):
    """s = 1e9: a frame with a feature never looks beyond itself and equals distance_transform_edt_frames bit for bit; a
    frame without one takes the nearest frame that has one, points 1 - 3 of the contract (SciPy itself is not nearest
    there)"""
    from tobac_flow_amd import ndimage_dev
    s = 1e9
    for name in ("boxes", "gap"):
        markers = ec.VOLUMES[name]()
        xd = lib.to_dev(markers == 0)
        dist, indices = (host(a) for a in ndimage_dev.distance_transform_edt(xd, sampling=(s, 1, 1), return_indices=True))
        frames, frame_indices = (host(a) for a in ndimage_dev.distance_transform_edt_frames(xd, return_indices=True))
        empty = [t for t in range(markers.shape[0]) if not markers[t].any()]
        assert empty
        for t in range(markers.shape[0]):
            if t not in empty:
                same(dist[t], frames[t])
                assert (indices[0, t] == t).all() and np.array_equal(indices[1:, t], frame_indices[:, t])
        assert (markers[indices[0], indices[1], indices[2]] != 0).all()                              # (1)
        assert np.array_equal(dist, ec.at_indices(indices, s))                                       # (2)
        ft, fy, fx = np.nonzero(markers)
        for t in empty:                                                                              # (3), by brute force
            tt, yy, xx = (c.ravel()[:, None] for c in np.meshgrid([t], *map(np.arange, markers.shape[1:]), indexing="ij"))
            minimum = ec.expression(ft[None], fy[None], fx[None], tt, yy, xx, s).min(1).reshape(markers.shape[1:])
            assert (dist[t] <= minimum * (1 + 4 * ec.EPS)).all() and (dist[t] >= s).all()
            assert (np.abs(indices[0, t] - t) == 1).all()


# ---- the C ABI directly ----------------------------------------------------------------------------------------------
def _frames(lib, markers):
    from tobac_flow_amd import ndimage_dev
    return ndimage_dev.edt_squared_frames(lib.to_dev(markers), return_nearest=True)


def test_c_abi_takes_misaligned_views_a_null_src_and_a_null_nearest(lib):
    from tobac_flow_amd import ndimage_dev
    t, L = lib.torch(), lib.lib()
    markers, s = ec.gap(), 10 / 3
    T, H, W = markers.shape
    n = markers.size
    d2, nearest = _frames(lib, markers)
    want_dist, want_src = ndimage_dev.edt_time_envelope(d2, nearest, s)
    ec.check("gap", "10_3", host(want_dist), host(transform(lib, "gap", "10_3")[1]))
    assert np.array_equal(host(want_src), np.ravel_multi_index(tuple(host(transform(lib, "gap", "10_3")[1]).astype(np.int64)), markers.shape))
    shifted = []
    for a in (d2, nearest):                                       # one element past the allocation's alignment
        flat = t.zeros(n + 1, dtype=t.int32, device=d2.device)
        flat[1:].copy_(a.reshape(-1))
        assert flat[1:].data_ptr() % 16 == 4
        shifted.append(flat[1:])
    dist = t.full((n + 2,), -7.0, dtype=t.float64, device=d2.device)
    src = t.full((n + 2,), -7, dtype=t.int64, device=d2.device)
    call = lambda near, dst, out: lib.check(L.tf_edt_time_envelope(lib.ptr(shifted[0]), near, T, H, W, s, lib.ptr(dst[1:]), out,   # noqa: E731
                                                                    lib.stream_ptr()), "tf_edt_time_envelope")
    call(lib.ptr(shifted[1]), dist, lib.ptr(src[1:]))
    same(host(dist[1:-1]), host(want_dist).ravel())
    same(host(src[1:-1]), host(want_src).ravel())
    assert host(dist)[[0, -1]].tolist() == [-7, -7] and host(src)[[0, -1]].tolist() == [-7, -7]      # nothing beyond the volume
    dist.fill_(-7.0)
    call(lib.ptr(shifted[1]), dist, None)                                                            # NULL src
    same(host(dist[1:-1]), host(want_dist).ravel())
    dist.fill_(-7.0)
    call(None, dist, None)                                                                           # NULL nearest and src
    d2h = host(d2).astype(np.float64)
    key = np.full(markers.shape, np.inf)
    for k in range(T):                                            # sqrt of the smallest fl(fl((k - t) s)^2 + d2[k]): NOT SciPy's order
        a = (k - np.arange(T, dtype=np.float64)) * s
        key = np.minimum(key, np.where(d2h[k] == 2 ** 31 - 1, np.inf, (a * a)[:, None, None] + d2h[k][None]))
    same(host(dist[1:-1]), np.sqrt(key).ravel())
    assert (np.abs(host(dist[1:-1]) - host(want_dist).ravel()) <= 4 * ec.EPS * host(want_dist).ravel()).all()
    plain, no_src = ndimage_dev.edt_time_envelope(d2, None, s)
    assert no_src is None
    same(host(plain).ravel(), np.sqrt(key).ravel())


def test_c_abi_reports_what_it_requires(lib):
    t, L = lib.torch(), lib.lib()
    x = t.zeros(8, dtype=t.int32, device=lib.device())
    d = t.zeros(8, dtype=t.float64, device=x.device)
    s = t.zeros(8, dtype=t.int64, device=x.device)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.tf_edt_time_envelope(lib.ptr(x), lib.ptr(x), 1, 2, 4, bad, lib.ptr(d), lib.ptr(s), lib.stream_ptr()) == -1
        assert b"finite" in L.tf_last_error()
    assert L.tf_edt_time_envelope(lib.ptr(x), None, 1, 2, 4, 1.0, lib.ptr(d), lib.ptr(s), lib.stream_ptr()) == -1       # src needs nearest
    assert b"nearest" in L.tf_last_error()
    assert L.tf_edt_time_envelope(lib.ptr(x), None, 1, 2, 4, 1.0, None, None, lib.stream_ptr()) == -1
    assert L.tf_edt_time_envelope(lib.ptr(x), None, 1, 32769, 32769, 1.0, lib.ptr(d), None, lib.stream_ptr()) == -1
    assert b"2^31" in L.tf_last_error()
    assert L.tf_edt_time_envelope(lib.ptr(x), None, 0, 2, 4, 1.0, lib.ptr(d), None, lib.stream_ptr()) == -1
    assert L.tf_edt_time_envelope(lib.ptr(x), lib.ptr(x), 1, 2, 4, 1.0, lib.ptr(d), lib.ptr(s), lib.stream_ptr()) == 0
    yy, xx = np.mgrid[:2, :4]                                     # nearest = 0 everywhere: the distance to voxel (0, 0)
    same(host(d), np.sqrt((yy * yy + xx * xx).astype(np.float64)).ravel())
    assert host(s).tolist() == [0] * 8


def test_marker_dtypes_come_back_as_they_went_in(lib):
    from tobac_flow_amd import validation as v
    markers = ec.gap()
    want = ec.reference("gap", "10_3")
    one_label = vc.single_label(ec.brute_force("gap", "10_3")["sets"])
    for dtype in (np.int64, np.uint8, np.float32, np.float64):
        dist, closest = v.get_marker_distance_ellipse_dev(markers.astype(dtype), 3, 10)
        assert closest.dtype == dtype and dist.dtype == np.float64
        one = ec.brute_force("gap", "10_3")["count"] == 1
        assert np.array_equal(dist[one], want["distances"][one])
        assert np.array_equal(closest[one_label], want["closest"][one_label].astype(dtype))
