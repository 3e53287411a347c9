"""Point binning on the GPU (tobac_flow_amd.binning / glm / nexrad, tf_bin_points) against the NumPy restatement of
tests/binning_cases.py, the libraries' results in tests/golden/binning_ref.npz and the recipes' host forms.

The contract: counts -- and every integer grid derived from them -- equal NumPy's and SciPy's bit for bit and are the same
in every run; a sum differs from the libraries' sequential bincount by the summation order only, so per bin by at most
bc.bound() = 2 (n - 1) 2^-53 sum|term| computed from the inputs (a one-term bin is bit-equal); means and weighted means by
that bound propagated through the quotient (bc.quotient_bound()).  Every case runs from 16-byte aligned tensors and from
tensors that start one element later (the element-load form of the kernel)."""
import numpy as np
import pytest

import binning_cases as bc

pytestmark = pytest.mark.gpu
SHIFTS = (0, 1)
ALL = ("count", "count_v", "sum_w", "sum_wv")


@pytest.fixture(scope="module")
def lib():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib


def shifted(lib, a, shift):
    """the array on the device, starting `shift` elements past an allocation (which is at least 256-byte aligned)"""
    if a is None:
        return None
    t = lib.torch()
    a = np.ascontiguousarray(a)
    src = t.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a)
    buf = t.empty(a.size + shift, dtype=src.dtype, device=lib.device())
    buf[shift:] = src.to(lib.device())
    out = buf[shift:]
    assert a.size == 0 or out.data_ptr() % 16 == (shift * out.element_size()) % 16
    return out


def run(lib, shift, coords, edges, outputs=ALL, **kw):
    from tobac_flow_amd import binning
    per_point = {k: shifted(lib, kw.pop(k, None), shift) for k in ("values", "weights", "keep", "keep_value", "time")}
    got = binning.bin_points([shifted(lib, c, shift) for c in coords], edges, outputs=outputs,
                             **{k: v for k, v in per_point.items() if v is not None}, **kw)
    return {k: (v if k == "status" else v.cpu().numpy()) for k, v in got.items()}


def check(got, want, outputs=ALL):
    """counts exactly, sums within the summation-order bound of their bin"""
    for name in outputs:
        g, w = got[name], want[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if name.startswith("count"):
            assert g.dtype == np.int32 and np.array_equal(g, w), name
            continue
        tol = bc.bound(want["count_v"], want["abs_" + name[4:]])
        finite = np.isfinite(w)
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~finite], w[~finite], equal_nan=True), name
        err = np.abs(g[finite] - w[finite])
        assert (err <= tol[finite]).all(), (name, float(err.max()), float(tol.max()))
        assert np.array_equal(g[want["count_v"] <= 1], w[want["count_v"] <= 1], equal_nan=True), name   # one term: bit-equal


def both(lib, shift, coords, edges, outputs=ALL, **kw):
    got = run(lib, shift, coords, edges, outputs=outputs, **kw)
    want = bc.restate(coords, edges, outputs=outputs, **kw)
    check(got, want, outputs)
    assert got["status"] == want["status"]
    return got, want


# ---- edges and points --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name,dtype", [("f32", np.float32), ("f64", np.float64)])
def test_points_on_and_next_to_every_edge(lib, name, dtype, shift):
    g = bc.golden()
    edges = g["edges/edges"]
    pts = bc.edge_points(edges, dtype)                            # every edge, nextafter on either side, the ends, +-inf, NaN
    got, _ = both(lib, shift, [pts], [edges], outputs=("count",), rule="numpy")
    assert np.array_equal(got["count"][0], g[f"edges/{name}_numpy"])
    finite = bc.edge_points(edges, dtype, specials=False)
    got, _ = both(lib, shift, [finite], [edges], outputs=("count",), rule="scipy")
    assert np.array_equal(got["count"][0], g[f"edges/{name}_scipy"])


@pytest.mark.parametrize("shift", SHIFTS)
def test_zero_width_bin(lib, shift):
    from tobac_flow_amd import binning
    got, _ = both(lib, shift, [bc.ZERO_WIDTH_POINTS], [bc.ZERO_WIDTH_EDGES], outputs=("count",), rule="numpy")
    assert got["count"][0].tolist() == [1, 0, 2]
    with pytest.raises(ValueError, match="numerically 0"):
        binning.bin_points([shifted(lib, bc.ZERO_WIDTH_POINTS, shift)], [bc.ZERO_WIDTH_EDGES], rule="scipy")


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("width", list(bc.SCIPY_WIDTHS))
def test_scipy_last_edge_rounding(lib, width, shift):
    g = bc.golden()
    edges, pts = bc.scipy_rounding_case(width)                    # last + 10^(-d-3), last + 10^(-d+1), nextafter(last), last
    got, _ = both(lib, shift, [pts], [edges], outputs=("count",), rule="scipy")
    assert np.array_equal(got["count"][0], g[f"rounding/{width}_scipy"]) and got["count"][0, -1] == 3
    assert got["status"] == bc.STATUS_RULES_DIFFER
    got, _ = both(lib, shift, [pts], [edges], outputs=("count",), rule="numpy")
    assert np.array_equal(got["count"][0], g[f"rounding/{width}_numpy"]) and got["count"][0, -1] == 1


# ---- lane partition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_lane_partition_and_dimensions(lib, nd, shift):
    for n in (0, 1, 63, 64, 65, 1003):
        c = bc.scattered(n, nd, seed=100 + n)
        both(lib, shift, c["coords"], c["edges"], rule="numpy", values=c["v64"], weights=c["w64"])
        c32 = bc.scattered(n, nd, seed=200 + n, dtype=np.float32)
        both(lib, shift, c32["coords"], c32["edges"], rule="scipy", values=c32["v32"], weights=c32["w32"])
        one_bin = [np.array([e[0], e[-1]]) for e in c["edges"]]   # n_edges = 2
        got, _ = both(lib, shift, c["coords"], one_bin, rule="numpy", values=c["v64"])
        assert got["count"].shape == (1,) + (1,) * nd


# ---- contention ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_contention_and_runs(lib, shift):
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 5000)
    got, _ = both(lib, shift, [np.full(5000, 0.5)], [np.array([0.0, 1.0, 2.0])], rule="numpy", values=v, weights=np.abs(v) + 1)
    assert got["count"][0].tolist() == [5000, 0] and got["count_v"][0].tolist() == [5000, 0]
    patterns, edges = bc.run_patterns()
    for name, coords in patterns.items():
        v = rng.uniform(-1, 1, coords.size).astype(np.float32)
        got, _ = both(lib, shift, [coords], [edges], rule="numpy", values=v)
        assert got["count"].sum() == coords.size, name


# ---- windows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_time_windows(lib, shift):
    c = bc.scattered(1003, 2, seed=7)
    c["time"][:12] = [0, 9, 10, 11, 12, 19, 20, 29, 30, 49, 50, 60]  # exactly at starts and ends, in the overlap, in the gap
    args = dict(rule="numpy", values=c["v32"], weights=c["w32"], time=c["time"])
    got, want = both(lib, shift, c["coords"], c["edges"], win_start=bc.WIN_START, win_end=bc.WIN_END, **args)
    per_frame = want["count"].reshape(5, -1).sum(1)
    assert got["count"].shape[0] == 5 and per_frame[3] == 0 and (per_frame[[0, 1, 2, 4]] > 0).all()
    inside = bc.restate(c["coords"], c["edges"])["count"].sum()
    assert want["count"].sum() != inside                             # the overlap counts twice, the gap drops
    both(lib, shift, c["coords"], c["edges"], win_start=bc.WIN_START + 1, win_end=bc.WIN_END, **args)      # lower-open
    got1, _ = both(lib, shift, c["coords"], c["edges"], rule="numpy", values=c["v32"], weights=c["w32"])   # T = 1, no windows
    assert got1["count"].shape[0] == 1 and got1["count"].sum() == inside
    both(lib, shift, c["coords"], c["edges"], win_start=bc.WIN_START[:1], win_end=bc.WIN_END[:1], **args)


# ---- masks and values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_masks_values_and_products(lib, shift):
    c = bc.scattered(1003, 2, seed=9)
    v32, v64 = c["v32"].copy(), c["v64"].copy()
    v32[::37], v64[::37] = np.nan, np.nan
    v32[5::91], v64[5::91] = np.inf, -np.inf
    for masks in (dict(keep=c["keep"]), dict(keep_value=c["keep_value"]), dict(finite_value=True),
                  dict(keep=c["keep"], keep_value=c["keep_value"], finite_value=True), dict(keep=c["keep"].astype(np.uint8))):
        for values, weights in ((v32, c["w32"]), (v32, c["w64"]), (v64, c["w32"]), (v64, None), (v32, None)):
            got, want = both(lib, shift, c["coords"], c["edges"], rule="numpy", values=values, weights=weights, **masks)
            if "finite_value" in masks:
                assert np.isfinite(got["sum_wv"]).all() and (got["count_v"] < got["count"]).any()
    # float32 * float32 rounds in float32: the two products differ
    a = bc.restate(c["coords"], c["edges"], values=c["v32"], weights=c["w32"])["sum_wv"]
    b = bc.restate(c["coords"], c["edges"], values=c["v32"], weights=c["w32"].astype(np.float64))["sum_wv"]
    assert not np.array_equal(a, b)
    # weights without values: np.histogramdd(weights=...)
    both(lib, shift, c["coords"], c["edges"], outputs=("count", "sum_w"), rule="numpy", weights=c["w64"])
    # the SciPy rule: finite_value drops silently, otherwise the status bit and SciPy's ValueError
    both(lib, shift, c["coords"], c["edges"], rule="scipy", values=v64, weights=c["w64"], finite_value=True, keep=c["keep"])
    from tobac_flow_amd import binning
    dev = [shifted(lib, x, shift) for x in c["coords"]]
    good = binning.bin_points(dev, c["edges"], rule="scipy", values=shifted(lib, c["v64"], shift), outputs=("sum_wv",))
    assert good["status"] == 0
    got = binning.bin_points(dev, c["edges"], rule="scipy", values=shifted(lib, v64, shift), outputs=("sum_wv",), raise_on_status=False)
    assert got["status"] & bc.STATUS_VALUE and not got["status"] & bc.STATUS_COORD
    with pytest.raises(ValueError, match="values contains non-finite"):
        binning.bin_points(dev, c["edges"], rule="scipy", values=shifted(lib, v64, shift), outputs=("sum_wv",))
    masked = binning.bin_points(dev, c["edges"], rule="scipy", values=shifted(lib, v64, shift), outputs=("sum_wv",),
                                keep_value=shifted(lib, np.isfinite(v64), shift))
    assert masked["status"] == 0                                     # a NaN behind keep_value is never looked at
    bad = [c["coords"][0].copy(), c["coords"][1]]
    bad[0][17] = np.nan
    got = binning.bin_points([shifted(lib, x, shift) for x in bad], c["edges"], rule="scipy", raise_on_status=False)
    assert got["status"] & bc.STATUS_COORD
    assert got["status"] == bc.restate(bad, c["edges"], "scipy", outputs=("count",))["status"]
    with pytest.raises(ValueError, match="sample contains non-finite"):
        binning.bin_points([shifted(lib, x, shift) for x in bad], c["edges"], rule="scipy")
    keep = np.ones(1003, bool)
    keep[17] = False
    assert binning.bin_points([shifted(lib, x, shift) for x in bad], c["edges"], rule="scipy", keep=shifted(lib, keep, shift))["status"] == 0


# ---- accumulation and repeat runs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_two_launches_into_one_buffer_equal_one_over_the_concatenation(lib, shift):
    from tobac_flow_amd import binning
    c = bc.scattered(1003, 2, seed=13)
    args = lambda sl: dict(values=shifted(lib, c["v64"][sl], shift), weights=shifted(lib, c["w32"][sl], shift),   # noqa: E731
                           time=shifted(lib, c["time"][sl], shift), win_start=bc.WIN_START, win_end=bc.WIN_END, outputs=ALL)
    first, second = slice(0, 400), slice(400, None)
    acc = binning.bin_points([shifted(lib, x[first], shift) for x in c["coords"]], c["edges"], **args(first))
    acc.pop("status")
    again = binning.bin_points([shifted(lib, x[second], shift) for x in c["coords"]], c["edges"], out=acc, **args(second))
    assert all(again[k].data_ptr() == acc[k].data_ptr() for k in ALL)
    want = bc.restate(c["coords"], c["edges"], values=c["v64"], weights=c["w32"], time=c["time"], win_start=bc.WIN_START, win_end=bc.WIN_END)
    check({k: again[k].cpu().numpy() for k in ALL}, want)
    with pytest.raises(ValueError, match="contiguous device tensor"):
        binning.bin_points([shifted(lib, x, shift) for x in c["coords"]], c["edges"], out={"count": acc["count"][:, :-1]})


def test_repeat_runs_give_identical_counts(lib):
    c = bc.scattered(5000, 2, seed=15)
    runs = [run(lib, 0, c["coords"], c["edges"], values=c["v64"], weights=c["w64"], keep_value=c["keep_value"]) for _ in range(3)]
    want = bc.restate(c["coords"], c["edges"], values=c["v64"], weights=c["w64"], keep_value=c["keep_value"])
    for r in runs:
        check(r, want)
        assert np.array_equal(r["count"], runs[0]["count"]) and np.array_equal(r["count_v"], runs[0]["count_v"])


# ---- the libraries' names -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_thin_forms_against_the_fixture(lib, nd):
    from tobac_flow_amd import binning
    g = bc.golden()
    c = bc.scattered(500, nd, seed=40 + nd)
    r = bc.restate(c["coords"], c["edges"], "numpy", weights=c["w64"])
    hist, edges = binning.histogramdd(c["coords"], c["edges"])
    assert isinstance(hist, np.ndarray) and hist.dtype == np.float64 and np.array_equal(hist, g[f"scattered{nd}/histogramdd"])
    assert len(edges) == nd and all(np.array_equal(a, b) for a, b in zip(edges, c["edges"]))
    hist, _ = binning.histogramdd(np.stack(c["coords"], axis=1), c["edges"], weights=c["w64"])       # the (N, D) form
    want = g[f"scattered{nd}/histogramdd_weights"]
    assert (np.abs(hist - want) <= bc.bound(r["count_v"], r["abs_w"])[0]).all()
    r = bc.restate(c["coords"], c["edges"], "scipy", values=c["v64"])
    res = binning.binned_statistic_dd(c["coords"], c["v64"], "count", c["edges"])
    assert res.binnumber is None and np.array_equal(res.statistic, g[f"scattered{nd}/binned_count"]) and len(res.bin_edges) == nd
    tol = bc.bound(r["count_v"], r["abs_wv"])[0]
    res = binning.binned_statistic_dd(c["coords"], c["v64"], "sum", c["edges"])
    assert (np.abs(res.statistic - g[f"scattered{nd}/binned_sum"]) <= tol).all()
    res = binning.binned_statistic_dd(c["coords"], c["v64"], "mean", c["edges"])
    want = g[f"scattered{nd}/binned_mean"]
    filled = r["count_v"][0] > 0
    assert np.array_equal(np.isnan(res.statistic), ~filled) and np.array_equal(np.isnan(want), ~filled)
    qtol = bc.quotient_bound(r["sum_wv"][0], r["count_v"][0].astype(np.float64), tol, 0.0)
    assert (np.abs(res.statistic - want)[filled] <= qtol[filled]).all()
    assert np.array_equal(res.statistic[r["count_v"][0] == 1], want[r["count_v"][0] == 1])
    if nd == 2:
        hist, xe, ye = binning.histogram2d(c["coords"][0], c["coords"][1], c["edges"])
        assert np.array_equal(hist, g["scattered2/histogram2d"]) and np.array_equal(xe, c["edges"][0]) and np.array_equal(ye, c["edges"][1])
        res = binning.binned_statistic_2d(c["coords"][0], c["coords"][1], c["v64"], "mean", c["edges"])
        want = g["scattered2/binned_2d_mean"]
        assert res.binnumber is None and (np.abs(res.statistic - want)[filled] <= qtol[filled]).all()
        assert np.array_equal(res.x_edge, c["edges"][0]) and np.array_equal(res.y_edge, c["edges"][1])
        # device tensors stay on the device
        t = lib.torch()
        hist_t, _ = binning.histogramdd([lib.to_dev(x) for x in c["coords"]], [lib.to_dev(e) for e in c["edges"]])
        assert isinstance(hist_t, t.Tensor) and hist_t.is_cuda and np.array_equal(hist_t.cpu().numpy(), g["scattered2/histogramdd"])
        res = binning.binned_statistic_dd([lib.to_dev(x) for x in c["coords"]], lib.to_dev(c["v64"]), "count", c["edges"])
        assert isinstance(res.statistic, t.Tensor) and np.array_equal(res.statistic.cpu().numpy(), g["scattered2/binned_count"])


# ---- the recipes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_regrid_glm(lib, shift):
    from tobac_flow_amd.glm import regrid_glm
    g = bc.golden()
    c = bc.glm_case()
    grid = regrid_glm(c["flash_x"], c["flash_y"], c["flash_file"], c["file_times"], c["goes_dates"], c["x_bins"], c["y_bins"])
    assert isinstance(grid, np.ndarray) and grid.dtype == np.int64 and grid.shape == (5, 33, 67)
    assert np.array_equal(grid, g["glm/grid"]) and np.array_equal(grid, bc.glm_host(c))
    assert (grid[1] == -1).all() and (grid[3] == 0).all() and grid[[0, 2, 4]].max() > 0
    dates = c["goes_dates"].astype("datetime64[us]")
    dev = regrid_glm(shifted(lib, c["flash_x"], shift), shifted(lib, c["flash_y"], shift), shifted(lib, c["flash_file"], shift),
                     c["file_times"].astype("datetime64[us]"), dates, c["x_bins"], c["y_bins"])
    assert dev.is_cuda and dev.dtype == lib.torch().int32 and np.array_equal(dev.cpu().numpy(), g["glm/grid"])
    # the grid is what the validation consumes: no frame is all -1 once the files cover it
    short = regrid_glm(c["flash_x"], c["flash_y"], c["flash_file"], c["file_times"], c["goes_dates"], c["x_bins"], c["y_bins"], max_time_diff=4)
    assert np.array_equal(short, bc.glm_loop(c, max_time_diff=4)) and not np.array_equal(short, grid)
    none = regrid_glm(c["flash_x"][:0], c["flash_y"][:0], c["flash_file"][:0], c["file_times"], c["goes_dates"], c["x_bins"], c["y_bins"])
    assert np.array_equal(none, np.where(grid < 0, -1, 0))


def _within(got, want, tol):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= tol[ok]).all(), float(np.abs(got[ok] - want[ok]).max())


@pytest.mark.parametrize("shift", SHIFTS)
def test_nexrad_site_grids_and_regrid(lib, shift):
    from tobac_flow_amd import nexrad
    g = bc.golden()
    c = bc.nexrad_case()
    order = ("time", "alt", "x", "y", "ref", "ref_valid")
    tols = []
    for s, site in enumerate(c["sites"]):
        raw, masked, mean = nexrad.get_site_grids(*[site[k] for k in order], c["x_bins"], c["y_bins"], c["goes_dates"], half_window=bc.HALF_WINDOW)
        _, _, host_mean, tol = bc.nexrad_site_host(site, c)
        tols.append(tol)
        assert raw.dtype == masked.dtype == mean.dtype == np.float64 and raw.shape == (4, 33, 67)
        assert np.array_equal(raw, g[f"nexrad/site{s}/raw"]) and np.array_equal(masked, g[f"nexrad/site{s}/masked"])
        _within(mean, g[f"nexrad/site{s}/mean"], tol)
        _within(mean, host_mean, tol)
        one = masked == 1
        assert one.any() and np.array_equal(mean[one], g[f"nexrad/site{s}/mean"][one])       # one gate: bit-equal
        dev = nexrad.get_site_grids(*[shifted(lib, site[k], shift) for k in order], c["x_bins"], c["y_bins"], c["goes_dates"])
        assert all(x.is_cuda for x in dev) and np.array_equal(dev[0].cpu().numpy(), raw) and np.array_equal(dev[1].cpu().numpy(), masked)
        # one frame alone, with datetimes
        f = 1
        start = (c["goes_dates"][f] - 150_000_000).astype("datetime64[us]")
        end = (c["goes_dates"][f] + 150_000_000).astype("datetime64[us]")
        raw1, masked1, mean1 = nexrad.get_nexrad_hist(*[site[k] for k in order], c["x_bins"], c["y_bins"], start, end)
        assert raw1.shape == (33, 67) and np.array_equal(raw1, raw[f]) and np.array_equal(masked1, masked[f])
        _within(mean1, g[f"nexrad/site{s}/mean"][f], tol[f])
        # float32 gates: SciPy bins them on float32-rounded edges, NumPy on the edges as given
        site32 = dict(site, x=site["x"].astype(np.float32), y=site["y"].astype(np.float32))
        want = bc.nexrad_site_loop(site32, c)
        raw, masked, mean = nexrad.get_site_grids(*[site32[k] for k in order], c["x_bins"], c["y_bins"], c["goes_dates"])
        assert np.array_equal(raw, want[0]) and np.array_equal(masked, want[1])
        _within(mean, want[2], bc.nexrad_site_host(site32, c)[3])
    assert (g["nexrad/site1/mean"][3] == 0).all()                   # the frame without a valid gate: zeros, not NaN
    grid, mask = nexrad.regrid_nexrad([[site[k] for k in order] for site in c["sites"]], c["x_bins"], c["y_bins"], c["goes_dates"])
    want, want_mask = g["nexrad/ref_grid"], g["nexrad/ref_mask"]
    assert mask.dtype == np.bool_ and np.array_equal(mask, want_mask) and grid.dtype == np.float64
    assert grid[0, 5, 7] == -33 and np.array_equal(grid == -33, want == -33) and np.isnan(grid[mask]).all()
    # total = sum over the two sites of mean * count, grid = total / n_valid.  A site's mean differs from the library's by
    # at most its bound, so its product by bound * count; then either side rounds each product, the sum of the two and
    # the division once: 2 * 3 roundings of relative size 2^-53 on quantities bounded by sum |mean| * count
    counts = [g[f"nexrad/site{s}/masked"] for s in range(2)]
    total_abs = sum(np.abs(np.nan_to_num(g[f"nexrad/site{s}/mean"])) * counts[s] for s in range(2))
    n_valid = counts[0] + counts[1]
    with np.errstate(all="ignore"):
        tol = (sum(t * n for t, n in zip(tols, counts)) + 6 * bc.U * total_abs) / np.where(n_valid > 0, n_valid, 1)
    _within(grid, want, tol)


@pytest.mark.parametrize("shift", SHIFTS)
def test_weighted_binned_mean_2d(lib, shift):
    from tobac_flow_amd.binning import weighted_binned_mean_2d
    g = bc.golden()
    c = bc.flux_case()
    bins = (c["lat_bins"], c["lon_bins"])
    for weights, name in (("area", "mean_f32_weights"), ("area64", "mean_f64_weights")):
        host, tol = bc.flux_host(c, weights)
        got = weighted_binned_mean_2d(c["lat"], c["lon"], c["data"], c[weights], bins=bins)       # 2-D arrays, NaN and inf data
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (20, 30)
        _within(got, g[f"flux/{name}"], tol)
        _within(got, host, tol)
        dev = weighted_binned_mean_2d(*[shifted(lib, c[k].ravel(), shift) for k in ("lat", "lon", "data", weights)], bins=bins)
        assert dev.is_cuda
        _within(dev.cpu().numpy(), g[f"flux/{name}"], tol)
    assert np.isnan(got).any() and np.isfinite(got).any()
