"""The register budget of tf_relabel_merge's two kernels as build-time facts (the compiler's own figures,
-Rpass-analysis=kernel-resource-usage on the Makefile's flags; no GPU is needed).  The pass streams the volumes and gathers
from small tables: 64 registers are the 8 waves per SIMD that hide both latencies, and scratch would add traffic of its own."""
import pytest

from test_kernel_resources_cpu import _allocated, _hipcc, _one, _resources

KERNELS = [f"_ZN12_GLOBAL__N_115k_relabel_mergeILi{per}EEE" for per in (4, 1)]      # 16-byte form, element form


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    return _resources("relabel_merge.hip", str(tmp_path_factory.mktemp("relabel_merge_resources")))


@pytest.mark.parametrize("kernel", KERNELS)
def test_relabel_merge_keeps_8_waves_per_simd(resources, kernel):
    k = _one(resources, kernel)
    print(kernel, k, "allocated", _allocated(k))
    assert k["scratch"] == 0
    assert _allocated(k) <= 64
    assert k["lds"] == 0
