"""The register and LDS budget of the kernels that share a CU in the pipelined step, as build-time facts.

The one-lane iteration kernel k_fb_iter<2, 0> keeps two waves resident per SIMD; a SIMD has 512 registers per lane in
granules of 8.  What the two waves leave free -- 64 registers, and the LDS four of its workgroups do not hold -- is what the
connectivity-1 flood sweeps have to fit into if they are to run BESIDE those waves instead of displacing them (DESIGN.md
section 4, "What runs beside the iteration kernel").  The figures are the compiler's own
(-Rpass-analysis=kernel-resource-usage on the Makefile's flags); no GPU is needed.

The per-label pass kernels that walk runs of equal labels (csrc/label_runs.h) are held to the same 64 registers for another
reason: they are bound by memory and atomics, and 64 registers are the 8 waves per SIMD that hide both."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tobac_flow_amd", "csrc")
SIMD_REGISTERS, GRANULE, CU_LDS = 512, 8, 163840

FB_ITER = "_Z9k_fb_iterILi2ELi0EE"                        # k_fb_iter<2, 0>
# phase A, and the chain levels / root phase at K = 1..3 (the depths the library starts with) and at run-time k (K = 0)
SWEEPS_IN_64 = ["_Z13k_ws_sweep_a63WsC"] + [f"_Z17k_ws_sweep_chain6ILi{k}ELb{r}EE" for k in (1, 2, 3, 0) for r in (0, 1)]
# any neighbour count: not part of the budget, reported
SWEEPS_ANY = ["_Z12k_ws_sweep_a3WsC", "_Z16k_ws_sweep_chainILb0EE", "_Z16k_ws_sweep_chainILb1EE", "_Z13k_ws_sweep_m1ILi6EE"]
# the per-label pass kernels, every instantiation: (source, mangled prefix)
LABEL_PASSES = ([("wstats.hip", f"_Z14k_wstats_pass{p}I{f}E") for p in (1, 2) for f in "fd"] + [("wstats.hip", "_Z12k_wprop_pass")]
                + [("edt.hip", f"_Z19k_label_nanmin_passI{f}E") for f in "hfd"]
                + [("props.hip", f"_Z13k_label_propsILb{a}EE") for a in (0, 1)]
                + [("label_filter.hip", f"_Z14k_label_filterILb{a}EE") for a in (0, 1)])


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def _resources(source, tmp):
    """{mangled kernel name: {"vgpr", "agpr", "scratch", "lds"}} of one source file, device code only"""
    cmd = [_hipcc()] + _makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                            os.path.join(CSRC, source), "-o", os.path.join(tmp, source + ".o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    fields = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    return out


def _one(res, prefix):
    hits = [v for k, v in res.items() if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} kernels"
    assert set(hits[0]) == {"vgpr", "agpr", "scratch", "lds"}, hits[0]
    return hits[0]


def _allocated(k):
    return -(-(k["vgpr"] + k["agpr"]) // GRANULE) * GRANULE


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    tmp = str(tmp_path_factory.mktemp("kernel_resources"))
    return {"ws": _resources("watershed.hip", tmp), "fb": _resources("farneback.hip", tmp)}


def test_two_iteration_waves_leave_64_registers(resources):
    it = _one(resources["fb"], FB_ITER)
    print("k_fb_iter<2, 0>:", it, "allocated", _allocated(it))
    assert 2 * _allocated(it) + 64 <= SIMD_REGISTERS


@pytest.mark.parametrize("kernel", SWEEPS_IN_64)
def test_connectivity_1_sweeps_fit_beside_them(resources, kernel):
    it, sw = _one(resources["fb"], FB_ITER), _one(resources["ws"], kernel)
    print(kernel, sw, "allocated", _allocated(sw))
    assert _allocated(sw) <= 64
    assert sw["scratch"] == 0
    assert 4 * it["lds"] + sw["lds"] <= CU_LDS


def test_the_other_sweep_forms_do_not_spill(resources):
    for kernel in SWEEPS_ANY:
        sw = _one(resources["ws"], kernel)
        print(kernel, sw, "allocated", _allocated(sw))
        assert sw["scratch"] == 0


@pytest.fixture(scope="module")
def label_resources(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    tmp = str(tmp_path_factory.mktemp("label_pass_resources"))
    return {source: _resources(source, tmp) for source in sorted({s for s, _ in LABEL_PASSES})}


@pytest.mark.parametrize("source,kernel", LABEL_PASSES)
def test_label_pass_kernels_keep_8_waves_per_simd(label_resources, source, kernel):
    k = _one(label_resources[source], kernel)
    print(kernel, k, "allocated", _allocated(k))
    assert k["scratch"] == 0
    assert _allocated(k) <= 64
