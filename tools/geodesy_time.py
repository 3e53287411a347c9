"""Time the geodesy kernels (csrc/geodesy.hip) at the size of a GOES full-disk grid on the GPU, next to the store rate of the
copy kernel in the same run and to the package's NumPy path on this machine's CPU (pyproj is not available):

  grid inverse     tf_geos_inverse on N x N (float64 and float32 out) against tf_copy16 over buffers of the float64 outputs' size
  spacing          tf_grid_spacing on the N x N lat / lon (area alone, and dx, dy, area), and the whole create_new_goes_ds
  points           tf_geod_inverse and tf_geos_forward (without and with alt) on P points
  GLM parallax     tf_glm_parallax on P flashes (float32 and float64 in), tf_ecef in both modes on P points, and
                   glm.regrid_glm_lat_lon end to end onto a FRAMES x N x N grid, corrected against uncorrected

Device events around the entry point alone, operands on the device; create_new_goes_ds by a host clock around a
synchronise.  Median (min .. max) of RUNS windows of REPS calls each, per call, after WARM warm-ups.  The NumPy path runs on a CPU_SHARE-th of the rows / points
(one call) and is scaled.  Usage: python tools/geodesy_time.py [N] [P] [output file]
(development aid; the figures are kept in profiles/geodesy.txt)"""
import ctypes
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from tobac_flow_amd import _lib, _lmatools, dataset, geo, glm
from tobac_flow_amd.utils.xarray_utils import get_coord_bin_edges

N = int(sys.argv[1]) if len(sys.argv) > 1 else 5424
P = int(sys.argv[2]) if len(sys.argv) > 2 else 10 ** 7
OUT = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
WARM, RUNS, REPS, CPU_SHARE = 2, 9, 20, 10
FRAMES = 16
H_GOES, LON_0 = 35786023.0, -75.0


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def events(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(f, timer=events, reps=REPS):
    """per call: every timed window holds `reps` calls back to back"""
    def window():
        for _ in range(reps):
            f()
    for _ in range(WARM):
        f()
    torch.cuda.synchronize()
    times = [timer(window) / reps for _ in range(RUNS)]
    return statistics.median(times), min(times), max(times)


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


class Abi:
    class Projection:
        perspective_point_height = H_GOES
        longitude_of_projection_origin = LON_0
        latitude_of_projection_origin = 0.0
        sweep_angle_axis = "x"

    goes_imager_projection = Projection()
    t = np.datetime64("2018-06-19T17:00:00")


def main():
    L = _lib.lib()
    dev = _lib.device()
    say(f"device: {torch.cuda.get_device_name(0)}; tf_version {L.tf_version()}; N = {N}, P = {P}; median (min .. max) per call of {RUNS} windows of {REPS} calls after {WARM} warm-ups")
    step = 2 * 0.151844 / N
    x_host = -0.151844 + step * (np.arange(N) + 0.5)
    y_host = x_host[::-1].copy()
    x, y = torch.from_numpy(x_host).to(dev), torch.from_numpy(y_host).to(dev)
    p = geo.GeosProj(H_GOES, LON_0)
    geos = p._params()
    out_bytes = 2 * N * N * 8

    src, dst = torch.empty(out_bytes, dtype=torch.uint8, device=dev), torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    src.zero_()
    copy = timed(lambda: _lib.check(L.tf_copy16(_lib.ptr(src), _lib.ptr(dst), out_bytes, _lib.stream_ptr()), "tf_copy16"))
    say(f"tf_copy16, {out_bytes / 1e6:.0f} MB read and as much written          {fmt(copy)}   {out_bytes / copy[0] / 1e6:.0f} GB/s stored")
    del src, dst

    for name, tdtype, code, size in (("float64", torch.float64, _lib.TF_F64, 8), ("float32", torch.float32, _lib.TF_F32, 4)):
        lat, lon = torch.empty((N, N), dtype=tdtype, device=dev), torch.empty((N, N), dtype=tdtype, device=dev)
        t = timed(lambda: _lib.check(L.tf_geos_inverse(ctypes.byref(geos), _lib.ptr(x), N, _lib.ptr(y), N, _lib.ptr(lat), _lib.ptr(lon), code,
                                                        _lib.stream_ptr()), "tf_geos_inverse"))
        say(f"tf_geos_inverse {N} x {N} -> {name}, {2 * N * N * size / 1e6:.0f} MB stored     {fmt(t)}   {2 * N * N * size / t[0] / 1e6:.0f} GB/s stored, "
            f"{N * N / t[0] / 1e6:.1f} Gpixel/s")
    lat, lon = p.inverse_grid(x, y)
    say(f"  on the disk: {int(torch.isfinite(lat).sum())} of {N * N} pixels")

    ws = _lib.workspace(L.tf_grid_spacing_workspace_bytes(N, N), "geodesy")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    dx, dy, area = (torch.empty((N, N), dtype=torch.float64, device=dev) for _ in range(3))
    for label, outs in (("area", (None, None, area)), ("dx, dy, area", (dx, dy, area))):
        t = timed(lambda: _lib.check(L.tf_grid_spacing(geo.ELLIPSOIDS["WGS84"][0], geo.ELLIPSOIDS["WGS84"][1], _lib.ptr(lat), _lib.ptr(lon), N, N,
                                                        _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(status), _lib.ptr(ws),
                                                        ws.numel(), _lib.stream_ptr()), "tf_grid_spacing"))
        say(f"tf_grid_spacing {N} x {N} -> {label:<13}                  {fmt(t)}   {2 * N * N / t[0] / 1e6:.2f} G inverses/s; not converged: {int(status.item())}")
    del dx, dy, area
    source = Abi()
    source.x, source.y = x, y
    t = timed(lambda: dataset.create_new_goes_ds(source), wall, 1)
    say(f"create_new_goes_ds {N} x {N}, device tensors in and out (wall)   {fmt(t)}")

    rng = np.random.default_rng(0)
    lon1, lat1 = rng.uniform(-180, 180, P), rng.uniform(-80, 80, P)
    lon2, lat2 = lon1 + rng.uniform(-0.2, 0.2, P), lat1 + rng.uniform(-0.2, 0.2, P)
    far_lon2, far_lat2 = rng.uniform(-180, 180, P), rng.uniform(-80, 80, P)
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(lon1=lon1, lat1=lat1, lon2=lon2, lat2=lat2, far_lon2=far_lon2, far_lat2=far_lat2).items()}
    out = [torch.empty(P, dtype=torch.float64, device=dev) for _ in range(3)]
    ws = _lib.workspace(L.tf_geod_inverse_workspace_bytes(P), "geodesy")
    a, rf = geo.ELLIPSOIDS["WGS84"]
    for label, l2, p2 in (("neighbouring points (< 0.3 degrees apart)", "lon2", "lat2"), ("random pairs on the globe", "far_lon2", "far_lat2")):
        t = timed(lambda: _lib.check(L.tf_geod_inverse(a, rf, _lib.ptr(d["lon1"]), _lib.ptr(d["lat1"]), _lib.ptr(d[l2]), _lib.ptr(d[p2]), P,
                                                        _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(status), _lib.ptr(ws),
                                                        ws.numel(), _lib.stream_ptr()), "tf_geod_inverse"))
        say(f"tf_geod_inverse {P} {label:<42} {fmt(t)}   {P / t[0] / 1e6:.2f} G pairs/s, {P * 56 / t[0] / 1e6:.0f} GB/s moved; not converged: {int(status.item())}")
    plat, plon, alt = rng.uniform(20, 55, P), rng.uniform(-125, -65, P), rng.uniform(0, 15000, P)
    dp = [torch.from_numpy(v).to(dev) for v in (plat, plon, alt)]
    for label, altitude, moved in (("", None, 32), (" with alt", dp[2], 40)):
        t = timed(lambda: _lib.check(L.tf_geos_forward(ctypes.byref(geos), _lib.ptr(dp[0]), _lib.ptr(dp[1]), _lib.ptr(altitude), P, _lib.ptr(out[0]),
                                                        _lib.ptr(out[1]), _lib.stream_ptr()), "tf_geos_forward"))
        say(f"tf_geos_forward{label:<9} {P} points                          {fmt(t)}   {P / t[0] / 1e6:.2f} G points/s, {P * moved / t[0] / 1e6:.0f} GB/s moved")

    ltg = geo.GeosProj(H_GOES, LON_0, a=_lmatools.ltg_ellps_re, rf=_lmatools.semiaxes_to_invflattening(_lmatools.ltg_ellps_re, _lmatools.ltg_ellps_rp))
    ltg_geos = ltg._params()
    lla = geo.ELLIPSOIDS["GRS80"]
    more = [torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2)]
    for label, code, size, flat, flon in (("float64", _lib.TF_F64, 8, dp[0], dp[1]), ("float32", _lib.TF_F32, 4, dp[0].float(), dp[1].float())):
        for what, outs, stored in (("offsets and scan angles", (out[0], out[1], more[0], more[1]), 32), ("scan angles alone", (None, None, out[0], out[1]), 16)):
            t = timed(lambda: _lib.check(L.tf_glm_parallax(ctypes.byref(geos), ctypes.byref(ltg_geos), lla[0], lla[1], _lib.ptr(flat), _lib.ptr(flon), code, P,
                                                            _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(outs[3]), _lib.stream_ptr()),
                                         "tf_glm_parallax"))
            say(f"tf_glm_parallax {P} flashes, {label} in, {what:<24}    {fmt(t)}   {P / t[0] / 1e6:.2f} G flashes/s, "
                f"{P * (2 * size + stored) / t[0] / 1e6:.0f} GB/s moved")
    ecef = [torch.empty(P, dtype=torch.float64, device=dev) for _ in range(3)]
    t = timed(lambda: _lib.check(L.tf_ecef(_lib.ECEF_FROM_GEODETIC, lla[0], lla[1], _lib.ptr(dp[1]), _lib.ptr(dp[0]), _lib.ptr(dp[2]), P, _lib.ptr(ecef[0]),
                                           _lib.ptr(ecef[1]), _lib.ptr(ecef[2]), _lib.stream_ptr()), "tf_ecef"))
    say(f"tf_ecef geodetic -> ECEF {P} points                          {fmt(t)}   {P / t[0] / 1e6:.2f} G points/s, {P * 48 / t[0] / 1e6:.0f} GB/s moved")
    t = timed(lambda: _lib.check(L.tf_ecef(_lib.ECEF_TO_GEODETIC, lla[0], lla[1], _lib.ptr(ecef[0]), _lib.ptr(ecef[1]), _lib.ptr(ecef[2]), P, _lib.ptr(out[0]),
                                           _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()), "tf_ecef"))
    say(f"tf_ecef ECEF -> geodetic {P} points                          {fmt(t)}   {P / t[0] / 1e6:.2f} G points/s, {P * 48 / t[0] / 1e6:.0f} GB/s moved")
    del ecef, more

    grid_ds = Abi()
    grid_ds.x, grid_ds.y = x_host, y_host
    x_bins, y_bins = get_coord_bin_edges(x_host), get_coord_bin_edges(y_host)
    start = np.datetime64("2018-06-19T17:00:00", "us")
    goes_dates = start + np.arange(FRAMES) * np.timedelta64(300, "s")
    file_times = start - np.timedelta64(140, "s") + np.arange(FRAMES * 15) * np.timedelta64(20, "s")
    flash_file = torch.from_numpy(rng.integers(0, file_times.size, P)).to(dev)
    flat, flon = dp[0].float(), dp[1].float()
    for corrected in (False, True):
        t = timed(lambda: glm.regrid_glm_lat_lon(flat, flon, flash_file, file_times, grid_ds, goes_dates, x_bins, y_bins, corrected=corrected), wall, 1)
        say(f"regrid_glm_lat_lon {P} float32 flashes -> {FRAMES} x {N} x {N}, corrected={corrected!s:<5} (wall)   {fmt(t)}")
    del flash_file, flat, flon

    say(f"NumPy path on this machine's CPU, one call on a {CPU_SHARE}th of the work, scaled by {CPU_SHARE}:")
    rows = max(2, N // CPU_SHARE)

    def cpu(f):
        t0 = time.perf_counter()
        result = f()
        return (time.perf_counter() - t0) * 1e3 * CPU_SHARE, result
    t, (lat_h, lon_h) = cpu(lambda: p.inverse_grid(x_host, y_host[N // 2 - rows // 2:N // 2 - rows // 2 + rows]))
    say(f"  inverse_grid {N} x {N}                   {t:10.0f} ms")
    t, _ = cpu(lambda: geo.get_pixel_area(lat_h, lon_h))
    say(f"  get_pixel_area {N} x {N}                 {t:10.0f} ms")
    m = P // CPU_SHARE
    t, _ = cpu(lambda: geo.Geod().inv(lon1[:m], lat1[:m], lon2[:m], lat2[:m]))
    say(f"  Geod.inv {P} neighbouring points         {t:10.0f} ms")
    t, _ = cpu(lambda: p.forward_points(plat[:m], plon[:m]))
    say(f"  forward_points {P}                       {t:10.0f} ms")
    t, _ = cpu(lambda: p.forward_points(plat[:m], plon[:m], alt[:m]))
    say(f"  forward_points with alt {P}              {t:10.0f} ms")
    t, _ = cpu(lambda: geo.glm_parallax(p, ltg, lla, plat[:m], plon[:m]))
    say(f"  glm_parallax {P}                         {t:10.0f} ms")
    t, xyz = cpu(lambda: geo.geodetic_to_ecef(plon[:m], plat[:m], alt[:m], ellps="GRS80"))
    say(f"  geodetic_to_ecef {P}                     {t:10.0f} ms")
    t, _ = cpu(lambda: geo.ecef_to_geodetic(*xyz, ellps="GRS80"))
    say(f"  ecef_to_geodetic {P}                     {t:10.0f} ms")


if __name__ == "__main__":
    main()
