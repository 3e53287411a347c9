"""The fifth stage without a GPU: the restatements of tests/field_props_cases.py against the fixture written by the
reference's own add_cre_to_dataset, the NumPy paths of the package against both, the kernel bodies on the host, and the
argument errors of the stage functions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_props_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_restatement_equals_the_reference_fixture_bit_for_bit(dtype):
    cases, names, provenance = fc.golden()
    assert names == list(fc.CRE_NAMES) and "reference" in provenance
    inputs = cases[dtype]["in"]
    assert all(_same_bytes(inputs[n], fc.cre_inputs(dtype)[n]) for n in fc.RAW), "the fixture's inputs are the seeded ones"
    got = fc.restate_cre(inputs)
    assert list(got) == names
    for name in names:
        want = cases[dtype]["out"][name]
        assert want.dtype == np.dtype(dtype)
        assert fc.bits_equal(got[name], want), name
    # the plants are there: NaN, inf - inf, a zero from exact cancellation, and a tree that regrouping would change
    out = cases[dtype]["out"]
    assert np.isinf(inputs["toa_swup"][1, 2, 3]) and np.isnan(out["toa_swup_cre"][1, 2, 3]) and np.isnan(out["boa_lwdn_cre"][1, 2, 3])
    assert np.isnan(out["toa_net_cre"][1, 2, 3]) and np.isinf(out["boa_net"][1, 2, 3])
    assert out["boa_swdn_cre"][0, 0, 1] == 0 and not np.signbit(out["boa_swdn_cre"][0, 0, 1])
    if dtype == "float32":
        regrouped = inputs["toa_swdn"] - inputs["toa_swup"] - inputs["toa_lwup"]
        differs = np.isfinite(regrouped) & (regrouped != out["toa_net"])
        assert differs.mean() > 0.1, "regrouping the tree must show in the fixture"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("container", ["dict", "LabelDataset"])
def test_numpy_path_of_add_cre_to_dataset_equals_the_fixture(dtype, container):
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    cases, names, _ = fc.golden()
    inputs = {n: a.copy() for n, a in cases[dtype]["in"].items()}
    if container == "dict":
        ds = dict(inputs)
    else:
        ds = LabelDataset(coords={"t": np.arange(3)})
        for n, a in inputs.items():
            ds.add(n, a, ("t", "y", "x"))
    assert pp.add_cre_to_dataset(ds) is ds
    assert list(ds) == list(fc.RAW) + names                       # the reference's names in the reference's order
    for n in names:
        assert fc.bits_equal(np.asarray(ds[n]), cases[dtype]["out"][n]), n
        if container == "LabelDataset":
            assert ds.dims[n] == ("t", "y", "x")
    for n in fc.RAW:
        assert _same_bytes(np.asarray(ds[n]), cases[dtype]["in"][n]), "inputs are not modified"
    assert fc.bits_equal(pp.get_cre(inputs["boa_lwup"], inputs["boa_lwup_clr"]), cases[dtype]["out"]["boa_lwup_cre"])
    assert pp.CRE_NAMES == fc.CRE_NAMES and pp.FLUX_VARIABLES == fc.FLUX_VARIABLES and pp.CLOUD_VARIABLES == fc.CLOUD_VARIABLES
    assert pp.CLOUD_FLAGS == tuple(fc.CLOUD_FLAGS) and pp.STEP_DIMS == fc.DIMS


@pytest.mark.parametrize("shape", fc.SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("plane", [False, True])
def test_quality_weights_on_numpy_equal_the_restatement(shape, dtype, plane):
    from tobac_flow_amd import postprocess as pp
    c = fc.quality_case(shape, dtype, plane)
    got = pp.cloud_quality_weights(c["weights"], c["qcflag"], c["cth"], c["cot"])
    assert isinstance(got, np.ndarray) and got.shape == tuple(shape)
    assert fc.bits_equal(got, c["want"]), "NaN placement included"
    # any weights but float32 give float64, and a (1, H, W) plane is a plane
    ints = np.nan_to_num(c["weights"], nan=1, posinf=2).astype(np.int32)
    assert pp.cloud_quality_weights(ints, c["qcflag"], c["cth"], c["cot"]).dtype == np.float64
    if plane:
        assert fc.bits_equal(pp.cloud_quality_weights(c["weights"][None], c["qcflag"], c["cth"], c["cot"]), got)


def test_kernel_bodies_on_the_host_against_plain_loops(tmp_path):
    """tools/field_props_host_check.cpp: the bodies of csrc/field_props_kernels.h, every set and both type parameters,
    compiled for the CPU and run lane after lane on exactly-sized buffers (its first lines give the AddressSanitizer /
    UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "field_props_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "field_props_host_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "all equal" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def _dataset(case, dims=fc.DIMS):
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords={dim: case["index"][dim] for dim in dims})
    for dim in dims:
        ds.add(f"{dim}_label", case["labels"][dim], ("t", "y", "x"))
    return ds


def test_host_form_of_the_stage_functions_equals_the_loop_of_existing_calls():
    """weights of shape (T, 1, W) merely broadcast: every variable takes the per-variable host arm, on which the stage
    functions ARE the loop -- names, order, dims, dtypes and values, with an int16 variable among float ones"""
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case((3, 37, 41), False)
    fields = dict(case["fields"])
    w = case["weights"][:, :1, :].astype(np.float64)
    variables = ("cot", "dem", "cwp", "lts")
    got = pp.add_weighted_stats_of_fields(_dataset(case), fields, w, variables)
    want = _dataset(case)
    for var in variables:
        for dim in fc.DIMS:
            pp.add_weighted_stats_to_dataset(want, fields, w, var, dim)
    assert list(got) == list(want) and got.dims == want.dims
    assert got["core_step_dem_mean"].dtype == np.float64 and got["core_step_cot_max_error"].dtype == np.float32
    for name in want:
        assert fc.bits_equal(np.asarray(got[name]), np.asarray(want[name])), name
    # the flux section on the host: equal to add_cre_to_dataset and the loop, and flx_ds is left as it was
    flux = {n: fields[n] for n in fc.RAW + ("lts", "fth", "fth_uncertainty", "cbh")}
    keys = list(flux)
    got = pp.add_flux_properties(_dataset(case), flux, w, dims=fc.DIMS[:2])
    assert list(flux) == keys
    composed, want = pp.add_cre_to_dataset(dict(flux)), _dataset(case)
    for var in fc.FLUX_VARIABLES:
        for dim in fc.DIMS[:2]:
            pp.add_weighted_stats_to_dataset(want, composed, w, var, dim)
    assert list(got) == list(want) and got.dims == want.dims
    for name in want:
        assert fc.bits_equal(np.asarray(got[name]), np.asarray(want[name])), name
    _, names = fc.restate_flux_section(case["labels"], case["index"], fields, w, dims=fc.DIMS[:2])
    assert [n for n in got if not n.endswith("_label")] == names


def test_argument_errors():
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case((2, 32, 64), True)
    fields, w = case["fields"], case["weights"]
    with pytest.raises(KeyError, match="toa_lwup_clr"):
        pp.add_cre_to_dataset({n: fields[n] for n in fc.RAW if n != "toa_lwup_clr"})
    ds = _dataset(case)
    with pytest.raises(KeyError, match="no_such_variable"):
        pp.add_weighted_stats_of_fields(ds, fields, w, ("cot", "no_such_variable"))
    assert not any(n.endswith("_mean") for n in ds), "nothing is added before every variable is found"
    with pytest.raises(KeyError, match="boa_lwdn_clr"):
        pp.add_flux_properties(ds, {n: fields[n] for n in fields if n != "boa_lwdn_clr"}, w, ("toa_net", "boa_net_cre"))
    with pytest.raises(ValueError, match="id < 1"):
        bad = _dataset(case)
        bad.coords["core_step"] = np.array([3, 0, 1])
        pp.add_weighted_stats_of_fields(bad, fields, w, ("cot",))
    with pytest.raises(ValueError, match="broadcast"):
        pp.add_weighted_stats_of_fields(_dataset(case), fields, w[:, :-1], ("cot",))
    with pytest.raises(TypeError):
        pp.add_cloud_properties(_dataset(case), fields, w)        # the flag values have no default
    with pytest.raises(ValueError, match="weights"):
        pp.cloud_quality_weights(w[:, :-1], fields["lsflag"], fields["cth"], fields["cot"])
    with pytest.raises(ValueError, match="one shape"):
        pp.cloud_quality_weights(w, fields["lsflag"][:1], fields["cth"], fields["cot"])
    for name in ("get_cre", "add_cre_to_dataset", "cloud_quality_weights", "add_weighted_stats_of_fields", "add_cloud_properties",
                 "add_flux_properties"):
        assert name in pp.__all__ and callable(getattr(pp, name))


def test_entry_points_are_declared():
    from tobac_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "tobac_flow_hip.h")).read()
    for name in ("tf_flux_cre", "tf_quality_weights", "tf_label_wstats_multi", "tf_label_wstats_multi_workspace_bytes"):
        assert name in _lib.EXPORTS and f" {name}(" in header
    assert (_lib.TF_FIELDS_PLAIN, _lib.TF_FIELDS_TOA, _lib.TF_FIELDS_BOA) == (0, 1, 2)
    L = _lib.lib()
    assert L.tf_version() >= 119 and hasattr(L, "tf_label_wstats_multi")
    assert L.tf_label_wstats_multi_workspace_bytes(_lib.TF_FIELDS_BOA, 8, 100) >= 10 * 100 * 128
    assert L.tf_label_wstats_multi_workspace_bytes(_lib.TF_FIELDS_BOA, 5, 100) == 0 and L.tf_label_wstats_multi_workspace_bytes(_lib.TF_FIELDS_PLAIN, 9, 100) == 0
