"""The yardsticks of the device normalisation methods, without a device (tests/norm_cases.py has the cases, the classes
and the cap):

* the committed fixture holds the module's inputs and an expected result for every case;
* the numpy restatement of the device arithmetic (weak scalars, float64-then-round log and moments, running extremes over
  the window clipped to the frame and the frames SciPy's window holds along the pair axis, rank selection + numpy's lerp,
  the digitising map) against the reference's bytes: equal for the exact class, under the cap for the rounding class --
  so the cap cannot hide a failure of the kernels;
* the kernel bodies themselves, compiled for the host (tools/norm_host_check.cpp), against the same bytes;
* the compiler's resource figures of the new kernels: no scratch, LDS within a CU;
* the argument rules of normalise_pair_dev's parameter block."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import norm_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tobac_flow_amd", "csrc")
CU_LDS = 163840


@pytest.fixture(scope="module")
def golden():
    return nc.golden()


def test_fixture_holds_the_modules_cases(golden):
    fields = nc.fields()
    stored = np.load(nc.GOLDEN)
    assert sorted(k[len("field/"):] for k in stored.files if k.startswith("field/")) == sorted(fields)
    for name, value in fields.items():
        assert value.dtype == np.float32 and value.shape[0] == 2
        assert np.array_equal(stored["field/" + name].view(np.uint32), value.view(np.uint32)), name      # bit for bit: -0.0, NaN
    assert sorted(golden) == sorted(nc.cases())
    for name, c in golden.items():
        assert c["want"].dtype == np.uint8 and c["want"].shape == c["pair"].shape, name
    for path in (nc.GOLDEN, nc.GOLDEN_BIG):
        assert os.path.getsize(path) < 1 << 20
    # the content the cases are there for
    assert {c["pair"].shape[1:] for c in golden.values()} == {nc.ODD, nc.MID, nc.BIG}
    assert np.signbit(fields["signed"][fields["signed"] == 0]).any() and (fields["signed"] < 0).any()
    assert np.isposinf(fields["pinf"]).sum() == 1 and np.isneginf(fields["ninf"]).sum() == 1
    assert np.isnan(fields["nan_all"]).all() and np.isnan(fields["nan_one"][0]).any() and not np.isnan(fields["nan_one"][1]).any()
    assert np.array_equal(np.isnan(fields["nan_both"][0]), np.isnan(fields["nan_both"][1])) and np.isnan(fields["nan_both"]).any()
    assert np.unique(fields["three"]).size == 3 and np.unique(fields["constant"]).size == 1
    for method in ("log", "inverse_log", "z_score", "local_linear"):
        assert any(c["method"] == method and not c["exact"] and np.unique(c["want"]).size > 20 for c in golden.values()), method
    assert any(c["method"] == "log" and c["exact"] and not c["want"].any() for c in golden.values())


@pytest.mark.parametrize("name", list(nc.cases()))
def test_numpy_restatement_of_the_device_arithmetic(golden, name):
    c = golden[name]
    nc.hold(nc.model(c["method"], c["pair"], **c["kwargs"]), c["want"], c["exact"], name)


@pytest.mark.parametrize("quantiles", [1, 3, 64, 256, 1024])
def test_rank_selection_and_lerp_give_numpys_quantile_edges(quantiles):
    for field in ("smooth_odd", "three", "signed", "constant"):
        pair = nc.fields()[field]
        want = np.quantile(pair, np.linspace(0, 1, quantiles + 1))
        want[-1] = want[-1] + 1
        assert np.array_equal(nc.uniform_edges(pair, quantiles), want), field


@pytest.mark.parametrize("size", [1, 2, 3, 4, 7, 10, 100])
def test_clipped_window_equals_scipys_reflected_one(size):
    """SciPy's reflect border adds no value the window clipped to the frame does not hold, and from size 3 on the
    (2, H, W) filter is the 2-D filter of the pointwise extreme of the two frames"""
    import scipy.ndimage as ndi
    pair = nc.fields()["smooth_odd"]
    for op, filt in ((np.fmin, ndi.minimum_filter), (np.fmax, ndi.maximum_filter)):
        want = filt(pair, size)
        for f, frames in enumerate(nc.pair_sources(size)):
            assert np.array_equal(nc.window_extreme(op.reduce(pair[frames], 0), size, op), want[f]), (size, f)
    assert nc.pair_sources(size) == ([[0], [1]] if size == 1 else [[0], [0, 1]] if size == 2 else [[0, 1], [0, 1]])


def _manifest_line(name, c, prefix):
    from tobac_flow_amd.utils.normalisation_utils import norm_params_dev
    mid, p = norm_params_dev(c["method"], c["pair"].shape[1:], **c["kwargs"])
    H, W = c["pair"].shape[1:]
    return (f"{name} {mid} {H} {W} {p.flags} {p.vmin!r} {p.vmax!r} {p.max_std!r} {p.quantiles} {p.size} {int(c['exact'])} "
            f"{prefix}.in {prefix}.want")


def test_kernel_bodies_on_the_host(golden, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "norm_host_check")
    r = subprocess.run([cxx, "-O2", "-std=c++17", os.path.join(ROOT, "tools", "norm_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = []
    for k, (name, c) in enumerate(golden.items()):
        prefix = str(tmp_path / f"case{k}")
        np.ascontiguousarray(c["pair"]).tofile(prefix + ".in")
        np.ascontiguousarray(c["want"]).tofile(prefix + ".want")
        lines.append(_manifest_line(name, c, prefix))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(manifest)], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert f"in {len(golden)} cases" in r.stdout


# ---- the compiler's resource figures (the mechanism of tests/test_kernel_resources_cpu.py) -------------------------------
NEW_KERNELS = ["k_nm_reduce", "k_nm_finish", "k_nm_map", "k_nm_row_filter", "k_nm_col_suffix", "k_nm_col_finish", "k_nm_plan",
               "k_nm_hist", "k_nm_scan", "k_nm_resolve", "k_nm_uniform_map"]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("no hipcc")
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    tmp = str(tmp_path_factory.mktemp("norm_resources"))
    cmd = [hipcc] + flags.replace("$(ARCH)", arch).split() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                              os.path.join(CSRC, "norm_methods.hip"), "-o", os.path.join(tmp, "norm_methods.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    fields = {"VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    return out


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_new_kernels_do_not_spill_and_fit_the_lds(resources, kernel):
    hits = {k: v for k, v in resources.items() if re.search(r"\d" + kernel + r"(?![a-z_])", k)}
    assert len(hits) == 1, (kernel, sorted(resources))
    (name, k), = hits.items()
    print(name, k)
    assert k["scratch"] == 0
    dynamic = 2 * 4 * 8192 if kernel == "k_nm_row_filter" else 0          # two rows of TF_NORM_MAX_ROW floats at launch
    assert k["lds"] + dynamic <= 65536 <= CU_LDS                          # what a workgroup may hold without opting in


# ---- the parameter block ---------------------------------------------------------------------------------------------
def test_parameter_block_follows_the_host_calls_keywords():
    from tobac_flow_amd import _lib
    from tobac_flow_amd.utils.normalisation_utils import norm_params_dev
    mid, p = norm_params_dev("linear", vmin=1, vmax=2.5)
    assert (mid, p.vmin, p.vmax, p.flags) == (0, 1.0, 2.5, _lib.NORM_HAS_VMIN | _lib.NORM_HAS_VMAX)
    mid, p = norm_params_dev("log", vmax=np.float32(0.1))
    assert mid == 1 and p.vmax == float(np.float32(0.1)) and p.flags == _lib.NORM_HAS_VMAX | _lib.NORM_F32_SCALARS
    assert norm_params_dev("linear", vmin=None, vmax=3)[1].flags == _lib.NORM_HAS_VMAX
    assert norm_params_dev("z_score")[1].max_std == 3 and norm_params_dev("z_score", max_std=2)[1].max_std == 2
    assert norm_params_dev("local_linear")[1].size == 100 and norm_params_dev("uniform")[1].quantiles == 256
    for method, kw in (("linear", {"size": 3}), ("z_score", {"vmin": 0}), ("uniform", {"size": 3}), ("local_linear", {"quantiles": 4}),
                       ("log", {"max_std": 1})):
        with pytest.raises(TypeError):
            norm_params_dev(method, **kw)
    for method, kw in (("linear", {"vmin": np.float64(1.0)}), ("linear", {"vmax": np.int64(3)}), ("z_score", {"max_std": np.float64(2)}),
                       ("linear", {"vmin": np.array(1.0, np.float32)}), ("local_linear", {"size": 0}), ("local_linear", {"size": 2.0}),
                       ("uniform", {"quantiles": 0}), ("uniform", {"quantiles": 1025}), ("uniform", {"quantiles": 2048})):
        with pytest.raises(ValueError):
            norm_params_dev(method, **kw)
    with pytest.raises(ValueError):
        norm_params_dev("local_linear", (10, 8193), size=5)
    with pytest.raises(ValueError):
        norm_params_dev("uniform", (4, 8), quantiles=64)
    with pytest.raises(ValueError, match="not an acceptable"):
        norm_params_dev("quadratic")


def test_library_exports_the_entry_points():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 104
    p = _lib.NormParams()
    L.tf_norm8_default_params(p)
    assert (p.max_std, p.quantiles, p.size, p.flags) == (3.0, 256, 100, 0)
    assert L.tf_norm8_workspace_bytes(64, 96, 6, p) == 0 and L.tf_norm8_workspace_bytes(64, 96, 0, p) > 0
    names = [L.tf_profile_kernel_name(i) for i in range(L.tf_profile_kernel_count())]
    assert b"norm8_pair" in names and names[0] == b"to8bit_pair"
