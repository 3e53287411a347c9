"""The fifth stage on the GPU (tf_flux_cre, tf_quality_weights, tf_label_wstats_multi and the stage functions of
tobac_flow_amd.postprocess) against the reference-written fixture, the restatements of tests/field_props_cases.py and
the package's own composed calls.

Bounds (field_props_cases.check_stats, all computed from the restatement's side).  The NaN pattern of every column, n,
min, max and the errors at them are exact.  The mean is held to |d mean| <= 8 n 2^-53 sum|w x| / sum w per label: both
sides sum n products in double in some order, each within n 2^-53 sum|w x| of exact and sum w within n 2^-53 relative,
(4 n + 1) 2^-53 sum|w x| / sum w to first order; the fields are signed, so the bound is absolute.  std, the uncertainty
of the mean and the combined error are held to rtol 1e-9 (non-negative terms; the mean's perturbation enters the squared
deviations in second order) on the condition, asserted with the cases, that std >= 1e-6 max|x| for every label of n >= 2
but the constant one, which is held by std <= 8 n 2^-53 |x| / sqrt(c).  The same bounds hold between the fused and the
composed evaluation: they are bounds on any two orders of summation."""
import functools

import numpy as np
import pytest

import field_props_cases as fc

pytestmark = pytest.mark.gpu

TYPES = [(f, w) for f in ("float32", "float64") for w in ("float32", "float64")]
PLAIN_GROUPS = (("lts", "fth", "cbh", "cot", "cer"), ("cwp", "ctp", "cth"))       # five planes: the 8-plane kernel; three: the 4-plane one


def _dev(a, misaligned=False):
    """a device tensor of the array; misaligned: a view that starts one element into its buffer"""
    import torch
    a = np.ascontiguousarray(a)
    if not misaligned:
        return torch.as_tensor(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.as_tensor(a).dtype, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.as_tensor(a))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _expected(shape, plane, ftype, dim, var):
    """(restated columns, bounds) of one variable of a case over one label volume, computed once; the weights' type does
    not enter: a case's weights are float32 numbers in either type"""
    case = fc.stats_case(shape, plane)
    fields = fc.case_fields(case, ftype)
    x = fc.set_fields(fields, (var,))[0]
    return fc.restate_with_bounds(case["labels"][dim], x, fields.get(f"{var}_uncertainty"), case["weights"], case["index"][dim])


def _constant(index):
    at = np.flatnonzero(index == fc.L_CONST)
    return int(at[0]) if at.size else None


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_add_cre_to_dataset_on_device_equals_the_reference_fixture(dtype):
    import torch
    from tobac_flow_amd import postprocess as pp
    from tobac_flow_amd.dataset import LabelDataset
    cases, names, _ = fc.golden()
    ds = LabelDataset()
    for n in fc.RAW:
        ds.add(n, _dev(cases[dtype]["in"][n]), ("t", "y", "x"))
    before = {n: ds[n].clone() for n in fc.RAW}
    assert pp.add_cre_to_dataset(ds) is ds
    assert list(ds) == list(fc.RAW) + names                       # the reference's names in the reference's order
    for n in names:
        assert isinstance(ds[n], torch.Tensor) and ds.dims[n] == ("t", "y", "x")
        assert fc.bits_equal(ds[n].cpu().numpy(), cases[dtype]["out"][n]), n
    for n in fc.RAW:
        assert fc.bits_equal(ds[n].cpu().numpy(), before[n].cpu().numpy()), n + ": inputs are not modified"
    # a plain mapping, and every operand misaligned (the element-load and element-store form of the kernel)
    plain = {n: _dev(cases[dtype]["in"][n], misaligned=True) for n in fc.RAW}
    pp.add_cre_to_dataset(plain)
    assert list(plain) == list(fc.RAW) + names
    assert all(fc.bits_equal(plain[n].cpu().numpy(), cases[dtype]["out"][n]) for n in names)
    assert fc.bits_equal(pp.get_cre(plain["toa_swup"], plain["toa_swup_clr"]).cpu().numpy(), cases[dtype]["out"]["toa_swup_cre"])


def _sets(fields, misaligned):
    """(set name, variables, device planes, device errors or None) of the three field sets and both plain kernels"""
    dev = {n: _dev(a, misaligned) for n, a in fields.items() if a.dtype.kind == "f"}
    yield "TOA", fc.TOA_FIELDS, [dev[n] for n in fc.TOA_PLANES], None
    yield "BOA", fc.BOA_FIELDS, [dev[n] for n in fc.BOA_PLANES], None
    for group in PLAIN_GROUPS:
        yield "PLAIN", group, [dev[n] for n in group], [dev.get(f"{n}_uncertainty") for n in group]


def _multi_against_everything(shape, plane, ftype, wtype, misaligned=False, composed=True):
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case(shape, plane)
    fields = fc.case_fields(case, ftype)
    dim = fc.DIMS[0]
    labels, index = case["labels"][dim], case["index"][dim]
    n_labels = int(index.max())
    lab, w = _dev(labels, misaligned), _dev(case["weights"].astype(wtype), misaligned)
    before = lab.clone()
    materialised = pp.add_cre_to_dataset({n: _dev(fields[n]) for n in fc.RAW}) if composed else None
    for set_name, variables, planes, errors in _sets(fields, misaligned):
        records = pp._wstats_multi(lab, n_labels, set_name, planes, errors, w, plane)
        assert records.shape == (len(variables), n_labels, 10)
        for k, var in enumerate(variables):
            what = f"{shape} plane={plane} {ftype}/{wtype} {set_name} {var}"
            want, bounds = _expected(shape, plane, ftype, dim, var)
            got = records[k][index - 1]
            with_e = errors is not None and errors[k] is not None
            ok = ~np.isnan(bounds[:, 0])
            assert np.array_equal(got[ok, 0], bounds[ok, 0]), what + ": n"
            assert with_e or np.isnan(got[:, 6:]).all(), what + ": no errors, no error columns"
            fc.check_stats(got[:, 2:10] if with_e else got[:, 2:6], want, bounds, _constant(index), what)
            if composed:                                          # the same field handed to today's call, derived ones materialised
                source = {var: materialised[var] if var in materialised else _dev(fields[var])}
                if with_e:
                    source[f"{var}_uncertainty"] = errors[k]
                other = pp.weighted_label_stats(lab, w, source, var, index, "x", uncertainty=with_e, dtype=np.float64)
                other = np.stack([v for _, v in other], 1)
                fc.check_pair(got[:, 2:2 + other.shape[1]], other, want, bounds, _constant(index), what)
    assert bool((lab == before).all())                            # the label volume is only read


@pytest.mark.parametrize("plane", [False, True], ids=["volume", "plane"])
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_wstats_multi_equals_the_restatement_and_the_single_field_call(shape, plane):
    """all three sets and all four type combinations: exact columns and NaN patterns equal the float64 restatement and
    today's weighted_label_stats on the materialised field; the summed columns within the bounds of the module docstring.
    A shared mask or a regrouped tree fails here: the cases plant a NaN in one _clr plane only, a label all-NaN in one
    plane, inf - inf, a NaN weight, a weight-0 extreme, ties, a constant label and a single voxel."""
    for ftype, wtype in TYPES:
        _multi_against_everything(shape, plane, ftype, wtype)


@pytest.mark.parametrize("plane", [False, True], ids=["volume", "plane"])
def test_wstats_multi_with_every_operand_misaligned(plane):
    _multi_against_everything((3, 37, 41), plane, "float32", "float64", misaligned=True, composed=False)
    _multi_against_everything((3, 37, 41), plane, "float64", "float32", misaligned=True, composed=False)


def _dataset(case, put):
    from tobac_flow_amd.dataset import LabelDataset
    ds = LabelDataset(coords={dim: case["index"][dim] for dim in fc.DIMS})
    for dim in fc.DIMS:
        ds.add(f"{dim}_label", put(case["labels"][dim]), ("t", "y", "x"))
    return ds


def _hold_stage(got, composed, stats, names):
    """a stage function's dataset against the composed one and the restated section"""
    keys = [n for n in got if not n.endswith("_label")]
    assert keys[:len(names)] == names and (composed is None or list(got) == list(composed))
    for prefix, (want, bounds) in stats.items():
        dim = next(d for d in fc.DIMS if prefix.startswith(d + "_"))
        n_out = 8 if f"{prefix}_max_error" in got else 4
        assert (f"{prefix}_max_error" in names) == (n_out == 8), prefix
        index = np.asarray(got.coords[dim])
        constant = _constant(index) if dim == fc.DIMS[0] else None                        # the plants lie in the first label volume
        mine = fc.stat_columns(got, prefix, n_out)
        rounding = 2.0 ** -24 if got[f"{prefix}_mean"].dtype == np.float32 else 0.0      # results in the field's type
        fc.check_stats(mine, want, bounds, constant, prefix, rounding)
        if composed is not None:
            fc.check_pair(mine, fc.stat_columns(composed, prefix, n_out), want, bounds, constant, prefix, rounding)
            for s in ("mean", "std", "min", "max"):
                name = f"{prefix}_{s}"
                assert got.dims[name] == composed.dims[name] == (dim,) and got[name].dtype == composed[name].dtype, name


STAGE_CASES = [((3, 37, 41), True, "float64"), ((5, 64, 96), False, "float32")]   # float32 fields; the production mix first


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("shape,plane,wtype", STAGE_CASES)
def test_flux_stage_equals_its_composed_definition(shape, plane, wtype, device):
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case(shape, plane)
    put = _dev if device else (lambda a: a.copy())
    names_in = fc.RAW + ("lts", "fth", "fth_uncertainty", "cbh")
    flx = {n: put(case["fields"][n]) for n in names_in}
    w = put(case["weights"].astype(wtype))
    ds = _dataset(case, put)
    before = {dim: (ds[f"{dim}_label"].clone() if device else ds[f"{dim}_label"].copy()) for dim in fc.DIMS}
    assert pp.add_flux_properties(ds, flx, w) is ds
    assert list(flx) == list(names_in), "flx_ds is not modified and holds no derived name"
    assert all(bool((ds[f"{dim}_label"] == before[dim]).all()) for dim in fc.DIMS)
    composed = _dataset(case, put)
    full = pp.add_cre_to_dataset(dict(flx))
    for var in fc.FLUX_VARIABLES:
        for dim in fc.DIMS:
            pp.add_weighted_stats_to_dataset(composed, full, w, var, dim)
    stats, names = fc.restate_flux_section(case["labels"], case["index"], {n: case["fields"][n] for n in names_in}, case["weights"])
    _hold_stage(ds, composed, stats, names)
    # the same bits whether or not flx_ds already holds the derived names; a subset launches only what it needs
    again = pp.add_flux_properties(_dataset(case, put), full, w, ("boa_net_cre", "lts", "toa_swup_cre"), fc.DIMS[1:2])
    assert [n for n in again if not n.endswith("_label")] == [f"thick_anvil_step_{v}_{s}" for v in ("boa_net_cre", "lts", "toa_swup_cre")
                                                               for s in ("mean", "std", "min", "max")]
    for n in again:
        if n.endswith(("_min", "_max")):
            assert fc.bits_equal(again[n], ds[n]), n


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("shape,plane,wtype", STAGE_CASES)
def test_cloud_stage_equals_its_composed_definition(shape, plane, wtype, device):
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case(shape, plane)
    put = _dev if device else (lambda a: a.copy())
    fields = case["fields"]
    names_in = fc.CLOUD_VARIABLES + tuple(f"{v}_uncertainty" for v in fc.WITH_UNCERTAINTY if v in fc.CLOUD_VARIABLES) + tuple(fc.CLOUD_FLAGS)
    cld = {n: put(fields[n]) for n in names_in}
    assert "int16" in str(cld["dem"].dtype)
    # the script's weights: the area times the three masks (a volume whatever the area was)
    qcflag = (np.arange(fields["cot"].size).reshape(shape) % 9 == 0).astype(np.int16)
    area = case["weights"].astype(wtype)
    weights = pp.cloud_quality_weights(put(area), put(qcflag), cld["cth"], cld["cot"])
    want_w = fc.restate_quality_weights(area, qcflag, fields["cth"], fields["cot"])
    assert fc.bits_equal(weights.cpu().numpy() if device else weights, np.ascontiguousarray(np.broadcast_to(want_w, shape)))
    ds = _dataset(case, put)
    assert pp.add_cloud_properties(ds, cld, weights, flags=fc.CLOUD_FLAGS) is ds
    composed = _dataset(case, put)
    for var in fc.CLOUD_VARIABLES:
        for dim in fc.DIMS:
            pp.add_weighted_stats_to_dataset(composed, cld, weights, var, dim)
    for flag, values in fc.CLOUD_FLAGS.items():
        for dim in fc.DIMS:
            pp.add_weighted_proportions_to_dataset(composed, cld[flag], weights, dim, flag_values=values, name=flag)
    stats, proportions, names = fc.restate_cloud_section(case["labels"], case["index"], {n: fields[n] for n in names_in},
                                                         np.broadcast_to(want_w, shape))
    _hold_stage(ds, composed, stats, names)
    assert ds["core_step_dem_mean"].dtype == np.float64 and ds["core_step_cot_mean"].dtype == np.float32
    rtol = 8 * int(np.prod(shape)) * 2.0 ** -53                   # two double sums of at most that many non-negative weights
    for name, want in proportions.items():
        np.testing.assert_allclose(ds[name], want, rtol=rtol, atol=0, equal_nan=True, err_msg=name)
        np.testing.assert_allclose(ds[name], composed[name], rtol=rtol, atol=0, equal_nan=True, err_msg=name)
        assert ds.dims[name] == composed.dims[name]


def test_a_variable_the_fused_kernel_does_not_take_keeps_its_place():
    """an int16 variable and one whose errors have another dtype than the field take the per-variable arm between fused
    ones; more than eight float variables make two groups; float64 and float32 variables make a group each"""
    from tobac_flow_amd import postprocess as pp
    case = fc.stats_case((3, 37, 41), True)
    f = case["fields"]
    source = {n: _dev(f[n]) for n in fc.CLOUD_VARIABLES + ("lts", "fth", "cbh", "cot_uncertainty", "cth_uncertainty", "fth_uncertainty")}
    source["cer"] = source["cer"].double()
    source["cth_uncertainty"] = source["cth_uncertainty"].double()
    variables = ("cot", "dem", "cer", "cwp", "ctp", "cth", "lts", "ctt", "fth", "cbh", "stemp", "ctp_corrected", "cth_corrected")
    w = _dev(case["weights"].astype(np.float64))
    ds = pp.add_weighted_stats_of_fields(_dataset(case, _dev), source, w, variables)
    composed = _dataset(case, _dev)
    for var in variables:
        for dim in fc.DIMS:
            pp.add_weighted_stats_to_dataset(composed, source, w, var, dim)
    host = {n: f[n] for n in source}
    stats, names = fc.restate_stage(case["labels"], case["index"], host, case["weights"], variables)
    _hold_stage(ds, composed, stats, names)
    assert ds["thin_anvil_step_cer_std"].dtype == np.float64 and ds["thin_anvil_step_dem_max"].dtype == np.float64


@pytest.mark.parametrize("plane", [False, True], ids=["volume", "plane"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_quality_weights_on_device_equal_the_restatement(shape, dtype, plane):
    import torch
    from tobac_flow_amd import postprocess as pp
    c = fc.quality_case(shape, np.dtype(dtype).type, plane)
    for misaligned in (False, True):
        got = pp.cloud_quality_weights(*[_dev(c[k], misaligned) for k in ("weights", "qcflag", "cth", "cot")])
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == tuple(shape)
        assert fc.bits_equal(got.cpu().numpy(), np.ascontiguousarray(c["want"])), "NaN placement included"
    mixed = pp.cloud_quality_weights(_dev(c["weights"]), c["qcflag"].astype(np.int64), c["cth"].astype(np.float64), _dev(c["cot"]))
    assert fc.bits_equal(mixed.cpu().numpy(), np.ascontiguousarray(c["want"]))
