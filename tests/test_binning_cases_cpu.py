"""The yardsticks of the point binning without a device: the NumPy restatement of tests/binning_cases.py against the
libraries' results in tests/golden/binning_ref.npz and against the live libraries (counts exactly, sums bit for bit: the
restatement runs the libraries' own sequential bincount), the recipes' one-call host forms against the plain per-frame
loops, the host side of tobac_flow_amd.binning / glm / nexrad before the library is touched, and the kernel body compiled
for the host (tools/bin_host_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import stats

import binning_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def test_fixture_inputs_are_the_cases_of_this_module():
    g = bc.golden()
    for name, case in (("glm", bc.glm_case()), ("flux", bc.flux_case())):
        for k, v in case.items():
            if k != "area64":
                _same(v, g[f"{name}/{k}"])
    nex = bc.nexrad_case()
    for s, site in enumerate(nex["sites"]):
        for k, v in site.items():
            _same(v, g[f"nexrad/site{s}/{k}"])
    for nd in (1, 2, 3):
        c = bc.scattered(500, nd, seed=40 + nd)
        for d in range(nd):
            _same(c["coords"][d], g[f"scattered{nd}/coord{d}"])
            _same(c["edges"][d], g[f"scattered{nd}/edges{d}"])
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        _same(bc.edge_points(g["edges/edges"], dtype), g[f"edges/{name}_points"])


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_restatement_equals_the_fixture_and_the_live_libraries(nd):
    g = bc.golden()
    c = bc.scattered(500, nd, seed=40 + nd)
    r = bc.restate(c["coords"], c["edges"], "numpy", weights=c["w64"])
    _same(r["count"][0], g[f"scattered{nd}/histogramdd"])
    _same(r["count"][0], np.histogramdd(c["coords"], bins=c["edges"])[0])
    _same(r["sum_w"][0], g[f"scattered{nd}/histogramdd_weights"])
    _same(r["sum_w"][0], np.histogramdd(c["coords"], bins=c["edges"], weights=c["w64"])[0])
    r = bc.restate(c["coords"], c["edges"], "scipy", values=c["v64"])
    assert r["status"] == 0 and (r["count"] == r["count_v"]).all()
    with np.errstate(all="ignore"):
        mean = np.where(r["count"] > 0, r["sum_wv"] / r["count"], np.nan)
    for statistic, mine in (("count", r["count"]), ("sum", r["sum_wv"]), ("mean", mean)):
        _same(mine[0], g[f"scattered{nd}/binned_{statistic}"])
        _same(mine[0], stats.binned_statistic_dd(c["coords"], c["v64"], statistic, bins=c["edges"])[0])
    assert r["count"].sum() < 500 and r["count"].max() > 1         # points outside the grid, and shared bins


def test_restatement_of_both_edge_rules_equals_the_libraries():
    g = bc.golden()
    edges = g["edges/edges"]
    assert edges.size == 68 and np.unique(np.diff(edges)[1:-1]).size > 1  # float32-derived midpoints: not equidistant
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        pts = bc.edge_points(edges, dtype)
        r = bc.restate([pts], [edges], "numpy")
        _same(r["count"][0], g[f"edges/{name}_numpy"])
        _same(r["count"][0], np.histogramdd([pts], bins=[edges])[0])
        finite = bc.edge_points(edges, dtype, specials=False)
        r = bc.restate([finite], [edges], "scipy")
        _same(r["count"][0], g[f"edges/{name}_scipy"])
        _same(r["count"][0], stats.binned_statistic_dd([finite], None, "count", bins=[edges])[0])
        assert bc.restate([pts], [edges], "scipy")["status"] & bc.STATUS_COORD
    _same(bc.restate([bc.ZERO_WIDTH_POINTS], [bc.ZERO_WIDTH_EDGES])["count"][0], [1, 0, 2])
    with pytest.raises(ValueError, match="numerically 0"):
        stats.binned_statistic_dd([bc.ZERO_WIDTH_POINTS], None, "count", bins=[bc.ZERO_WIDTH_EDGES])
    for width in bc.SCIPY_WIDTHS:
        e, pts = bc.scipy_rounding_case(width)
        r = bc.restate([pts], [e], "scipy")
        _same(r["count"][0], g[f"rounding/{width}_scipy"])
        _same(r["count"][0], stats.binned_statistic_dd([pts], None, "count", bins=[e])[0])
        assert r["count"][0, -1] == 3 and r["status"] == bc.STATUS_RULES_DIFFER
        _same(bc.restate([pts], [e], "numpy")["count"][0], g[f"rounding/{width}_numpy"])


def test_np_around_is_what_the_kernel_is_told_it_is():
    """multiply by 10^d, rint, divide for d > 0; divide, rint, multiply for d < 0 -- in the array's own type"""
    from tobac_flow_amd.binning import power_of_ten, scipy_decimals
    rng = np.random.default_rng(5)
    for dtype in (np.float32, np.float64):
        v = (rng.uniform(-2000, 2000, 4000)).astype(dtype)
        for d in (6, 8, 4, 1, 0, -2):
            s = dtype(power_of_ten(abs(d)))
            mine = np.rint(v * s) / s if d > 0 else np.rint(v / s) * s if d < 0 else np.rint(v)
            _same(mine, np.around(v, d))
            assert mine.dtype == dtype
    for width, d in bc.SCIPY_WIDTHS.items():
        assert scipy_decimals(width) == d
    assert power_of_ten(22) == 1e22 and power_of_ten(0) == 1.0 and power_of_ten(9) == 1e9
    with pytest.raises(ValueError, match="numerically 0"):
        scipy_decimals(0.0)


def test_recipe_host_forms_equal_the_per_frame_loops_and_the_fixture():
    g = bc.golden()
    glm = bc.glm_case()
    loop = bc.glm_loop(glm)
    _same(loop, g["glm/grid"])
    _same(bc.glm_host(glm), loop)
    assert (loop[1] == -1).all() and (loop[3] == 0).all() and loop.max() > 0 and loop.dtype == np.int64
    nex = bc.nexrad_case()
    stacks = []
    for s, site in enumerate(nex["sites"]):
        loop = bc.nexrad_site_loop(site, nex)
        raw, masked, mean, tol = bc.nexrad_site_host(site, nex)
        for name, a, b in zip(("raw", "masked", "mean"), loop, (raw, masked, mean)):
            _same(a, g[f"nexrad/site{s}/{name}"])
            _same(b, a)                                            # the restatement sums in the libraries' order: bit-equal
        assert (tol >= 0).all() and tol.max() < 1e-12
        stacks.append(loop)
        site32 = dict(site, x=site["x"].astype(np.float32), y=site["y"].astype(np.float32))      # SciPy bins these on float32 edges
        for a, b in zip(bc.nexrad_site_loop(site32, nex), bc.nexrad_site_host(site32, nex)[:3]):
            _same(b, a)
    grid, mask = bc.nexrad_regrid(stacks)
    _same(grid, g["nexrad/ref_grid"])
    _same(mask, g["nexrad/ref_mask"])
    assert grid[0, 5, 7] == -33 and mask.any() and np.isnan(grid[mask]).all() and (stacks[1][2][3] == 0).all()
    flux = bc.flux_case()
    for weights, name in (("area", "mean_f32_weights"), ("area64", "mean_f64_weights")):
        loop = bc.flux_loop(flux, weights)
        _same(loop, g[f"flux/{name}"])
        _same(bc.flux_host(flux, weights)[0], loop)
    assert not np.array_equal(g["flux/mean_f32_weights"], g["flux/mean_f64_weights"], equal_nan=True)   # the product's type matters


def test_glm_windows_and_bin_edges_of_the_package_equal_the_plain_forms():
    from tobac_flow_amd.glm import glm_windows
    from tobac_flow_amd.utils import get_coord_bin_edges
    from types import SimpleNamespace
    glm = bc.glm_case()
    starts, ends = bc.glm_windows_plain(glm["goes_dates"])
    ws, we = glm_windows(glm["goes_dates"])
    _same(ws, [bc.ticks(s) for s in starts])
    _same(we, [bc.ticks(e) for e in ends])
    as_datetime64 = glm["goes_dates"].astype("datetime64[us]")
    _same(glm_windows(as_datetime64)[0], ws)
    _same(glm_windows([bc.EPOCH + (t - np.datetime64(0, "us")).item() for t in as_datetime64], 15)[1], we)
    _same(glm_windows(as_datetime64, max_time_diff=4)[1] - glm_windows(as_datetime64, max_time_diff=4)[0], [240_000_000] * 5)
    for coord in (bc.abi_x(), bc.abi_y(), np.array([3.0, 4.0])):
        want = bc.coord_bin_edges(coord)
        _same(get_coord_bin_edges(coord), want)
        _same(get_coord_bin_edges(SimpleNamespace(data=coord, size=coord.size)), want)
        assert get_coord_bin_edges(coord).dtype == np.float64 and want.size == coord.size + 1


# ---- input validation: before the library is touched ---------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    from tobac_flow_amd import _lib

    def refuse(*args, **kwargs):
        raise AssertionError("the library was touched before the inputs were validated")
    for name in ("lib", "device", "to_dev", "torch"):
        monkeypatch.setattr(_lib, name, refuse)


def test_bad_inputs_raise_before_the_library_is_touched(no_library):
    from tobac_flow_amd import binning as b
    from tobac_flow_amd import glm
    x = np.linspace(0, 1, 9)
    e = np.linspace(0, 1, 5)
    for bins in (4, [4, 4], None):
        with pytest.raises(NotImplementedError, match="edge arrays"):
            b.histogram2d(x, x, bins)
        with pytest.raises(NotImplementedError, match="edge arrays"):
            b.binned_statistic_2d(x, x, x, "sum", bins)
    with pytest.raises(NotImplementedError, match="edge arrays"):
        b.histogramdd([x], 10)
    with pytest.raises(NotImplementedError, match="edge arrays"):
        b.weighted_binned_mean_2d(x, x, x, x)
    for statistic in ("median", "std", "min", np.mean):
        with pytest.raises(NotImplementedError, match="statistic"):
            b.binned_statistic_dd([x], x, statistic, [e])
    with pytest.raises(ValueError, match="monotonically"):
        b.histogramdd([x], [e[::-1]])
    with pytest.raises(ValueError, match="monotonically"):
        b.histogramdd([x], [np.array([0.0, np.nan, 1.0])])
    with pytest.raises(ValueError, match="numerically 0"):
        b.binned_statistic_dd([bc.ZERO_WIDTH_POINTS], None, "count", [bc.ZERO_WIDTH_EDGES])
    with pytest.raises(ValueError, match="at least 2 edges"):
        b.histogramdd([x], [e[:1]])
    with pytest.raises(ValueError, match="dimension of bins"):
        b.histogramdd([x, x], [e])
    with pytest.raises(ValueError, match="1 to 3"):
        b.bin_points([x] * 4, [e] * 4)
    with pytest.raises(TypeError, match="float32 or all"):
        b.bin_points([x, x.astype(np.float32)], [e, e])
    with pytest.raises(TypeError, match="coords"):
        b.bin_points([np.arange(9)], [e])
    with pytest.raises(ValueError, match="one entry per point"):
        b.bin_points([x, x[:-1]], [e, e])
    with pytest.raises(ValueError, match="one entry per point"):
        b.bin_points([x], [e], weights=x[:-1], outputs=("sum_w",))
    with pytest.raises(TypeError, match="keep"):
        b.bin_points([x], [e], keep=np.ones(9))
    with pytest.raises(ValueError, match="sum_wv needs values"):
        b.bin_points([x], [e], outputs=("sum_wv",))
    with pytest.raises(ValueError, match="outputs"):
        b.bin_points([x], [e], outputs=("median",))
    with pytest.raises(ValueError, match="go together"):
        b.bin_points([x], [e], time=np.zeros(9, np.int64))
    with pytest.raises(ValueError, match="non-decreasing"):
        b.bin_points([x], [e], time=np.zeros(9, np.int64), win_start=[5, 0], win_end=[6, 7])
    with pytest.raises(TypeError, match="time"):
        b.bin_points([x], [e], time=np.zeros(9), win_start=[0], win_end=[6])
    with pytest.raises(ValueError, match="flip"):
        b.bin_points([x], [e], flip=(1,))
    with pytest.raises(ValueError, match="rule"):
        b.bin_points([x], [e], rule="pandas")
    with pytest.raises(TypeError, match="times"):
        b.time_ticks(np.array([0.5, 1.5]))
    c = bc.glm_case()
    with pytest.raises(ValueError, match="at least 2 frames"):
        glm.regrid_glm(c["flash_x"], c["flash_y"], c["flash_file"], c["file_times"], c["goes_dates"][:1], c["x_bins"], c["y_bins"])
    with pytest.raises(ValueError, match="must increase"):
        glm.regrid_glm(c["flash_x"], c["flash_y"], c["flash_file"], c["file_times"], c["goes_dates"][::-1], c["x_bins"], c["y_bins"])
    with pytest.raises(ValueError, match="outside file_times"):
        glm.regrid_glm(c["flash_x"], c["flash_y"], c["flash_file"] + 1, c["file_times"], c["goes_dates"], c["x_bins"], c["y_bins"])


def test_abi_version_entry_point_and_argument_checks():
    """the host side of tf_bin_points: every check returns before a kernel is launched, so it runs without a device"""
    import ctypes
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 108 and "tf_bin_points" in _lib.EXPORTS and hasattr(L, "tf_bin_points")
    assert ctypes.sizeof(_lib.BinPoints) == 40 + 24 + 16 + 24 + 24 + 24 + 8 * 12
    somewhere = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value

    def params(**changes):
        P = _lib.BinPoints()
        P.n_dims, P.coord_dtype, P.rule, P.n_points, P.n_frames = 1, _lib.TF_F64, _lib.BIN_RULE_NUMPY, 5, 1
        P.n_edges[0], P.edges[0], P.coord[0], P.count, P.round_scale[0] = 2, somewhere, somewhere, somewhere, 1.0
        for k, v in changes.items():
            if isinstance(v, tuple):
                getattr(P, k)[v[0]] = v[1]
            else:
                setattr(P, k, v)
        return P

    assert L.tf_bin_points(ctypes.byref(params(n_points=0)), None) == 0      # no point: nothing is launched
    assert L.tf_bin_points(None, None) == -1
    for bad in (dict(n_dims=0), dict(n_dims=4), dict(coord_dtype=_lib.TF_I32), dict(rule=2), dict(flags=2), dict(n_points=2 ** 31),
                dict(n_points=-1), dict(n_frames=0), dict(n_frames=2), dict(time=somewhere), dict(n_edges=(0, 1)), dict(edges=(0, None)),
                dict(count=None), dict(sum_wv=somewhere), dict(value=somewhere, value_dtype=_lib.TF_U8), dict(flip_mask=2),
                dict(weight=somewhere, weight_dtype=_lib.TF_I32), dict(rule=_lib.BIN_RULE_SCIPY, round_scale=(0, 0.0)),
                dict(coord=(0, None))):
        assert L.tf_bin_points(ctypes.byref(params(**bad)), None) == -1, bad
        with pytest.raises(ValueError, match="tf_bin_points"):
            _lib.check(-1, "tf_bin_points")


def test_kernel_body_on_the_host_against_plain_loops(tmp_path):
    """tools/bin_host_check.cpp: the body of csrc/bin_kernels.h compiled for the CPU and run lane after lane on exactly-sized
    buffers, flat indices beyond 2^32 included (its first lines give the AddressSanitizer / UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "bin_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tools", "bin_host_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout + out.stderr
