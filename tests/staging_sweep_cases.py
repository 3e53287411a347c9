"""The sweep of tests/test_gpu_staging_truth.py: every public function that hands a host array to the staging cache
(`share=True`), remembers a result (`remember=True`) or prefetches (`_staging.Prefetch`), as one case each, and the table
SITES that maps every such call site of the package to the case that runs through it -- tests/test_staging_sites_cpu.py
holds the table against the package's source, so a new site fails there until it has a case here.

A case is a zero-argument callable that builds its host arguments as FRESH COPIES of values made once (so a second call is
recognised by content, never by address), calls the public function the way a script would, and returns {name: host
array}.  Shapes: (6, 300, 400) float32 / int32 = 2.9 MB and the (10, 300, 420) scene of tests/test_gpu_staging.py -- the
smallest array the cache remembers is 1 MiB; the property case is 440 wide so that its float64 (y, x) planes pass 1 MiB too.

Equality.  Everything the cases return is documented bit-identical from run to run and is compared with np.array_equal
-- the label reducers are called with exact reducers (np.nanmax, np.nanmin) for that reason -- with one exception:
calculate_label_properties' areas and locations are double atomics that may differ in the last bits between runs
(include/tobac_flow_hip.h, tf_label_props).  That case holds every run to the float64 restatement with the bounds of its own
test (tests/test_gpu_label_props._compare) inside the case, and hands only its exact variables (counts, times) to the
array-for-array comparison."""
import ast
import functools
import os
import warnings

import numpy as np

SHAPE = (6, 300, 400)
SCENE = (10, 300, 420)
PROPS_SHAPE = (6, 300, 440)
MINUTES = 5
MARGIN, TIME_MARGIN = 10, 1

PATTERNS = ("share=True", "remember=True", "_staging.upload(", "_staging.download(", "Prefetch(")

# (file under tobac_flow_amd/, enclosing top-level function or Class.method, "<module>" outside any) -> the case that runs it
SITES = {
    ("_lib.py", "to_dev"): "calculate_flow",                       # the door every share=True site goes through
    ("_lib.py", "to_host"): "get_anvil_markers",                   # ... and every remember=True site
    ("_staging.py", "<module>"): "calculate_flow",                 # (the module docstring names the keyword)
    ("_staging.py", "download"): "get_anvil_markers",
    ("flow.py", "_calculate_flow"): "calculate_flow",
    ("detection.py", "_to_device"): "detect_cores",
    ("detection.py", "_to_device_later"): "detect_cores",          # Prefetch: wvd and swd beside the kernels on bt
    ("detection.py", "_deliver"): "get_anvil_markers",
    ("detection.py", "detect_growth_markers"): "detect_growth_markers",
    ("detection.py", "detect_growth_markers_multichannel"): "detect_growth_markers_multichannel",
    ("validation.py", "_cylinder"): "get_marker_distance_cylinder",
    ("validation.py", "get_marker_distance_ellipse_dev"): "get_marker_distance_ellipse_dev",
    ("validation.py", "_label_nanmin"): "get_min_dist_for_objects",
    ("validation.py", "_list_flashes"): "flash_list",
    ("validation.py", "_cylinder_at"): "validate_markers",
    ("validation.py", "get_edge_filter_dev"): "get_edge_filter_dev",
    ("validation.py", "_keep_labels"): "validate_wrappers",
    ("validation.py", "_present"): "validate_detection",
    ("label.py", "label_props"): "calculate_label_properties",
    ("label.py", "unique_along_t"): "get_label_stats",
    ("label.py", "unique_per_frame"): "get_label_stats",
    ("dataset.py", "calculate_label_properties"): "calculate_label_properties",
    ("utils/label_utils.py", "_to_device"): "labeled_comprehension",
}


def scan_sites(package_dir):
    """{(file, enclosing function)} of every line of the package's Python source that holds one of PATTERNS -- code,
    comment or docstring alike: a plain text search, so nothing slips through by being spelt in an unusual place"""
    found = set()
    for folder, _, names in os.walk(package_dir):
        for name in sorted(names):
            if not name.endswith(".py"):
                continue
            path = os.path.join(folder, name)
            with open(path, encoding="utf-8") as f:
                text = f.read()
            spans = []
            for node in ast.parse(text).body:
                if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    spans.append((node.lineno, node.end_lineno, node.name))
                elif isinstance(node, ast.ClassDef):
                    for sub in node.body:
                        if isinstance(sub, (ast.FunctionDef, ast.AsyncFunctionDef)):
                            spans.append((sub.lineno, sub.end_lineno, f"{node.name}.{sub.name}"))
            for number, line in enumerate(text.splitlines(), 1):
                if any(p in line for p in PATTERNS):
                    inside = [s[2] for s in spans if s[0] <= number <= s[1]]
                    found.add((os.path.relpath(path, package_dir).replace(os.sep, "/"), inside[0] if inside else "<module>"))
    return found


# ---- values made once; the cases hand out copies ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """bt, wvd, swd of the script-sequence scene as host float32 arrays (do not modify)"""
    import torch
    from tools.script_sequence import scene
    return tuple(x.cpu().numpy() for x in scene(*SCENE, MINUTES, torch.device("cuda", 0)))


def _fields():
    from tools.synth import field_with_time
    return [field_with_time(x.copy(), minutes=MINUTES) for x in _scene()]


def _flow(bt):
    import tobac_flow_amd.flow as tf
    return tf.create_flow(bt, model="Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")


def _blobs(shape, seed, sigma=12.0):
    import scipy.ndimage as ndi
    return ndi.gaussian_filter(np.random.default_rng(seed).normal(size=shape), (0.7, sigma, sigma))


@functools.lru_cache(maxsize=None)
def _product():
    """A detection product on SHAPE: cores inside thick anvils inside thin anvils (the recipe of tests/props_cases.volumes,
    smoother so that a frame holds tens of regions, not thousands), anvil markers, the coordinates and the core -> anvil
    index; a sparse int32 flash grid with its times, its cylinder distance and edge filter.  Do not modify."""
    import scipy.ndimage as ndi
    from tobac_flow_amd import validation as v
    sm = _blobs(SHAPE, 5)
    label = lambda q: ndi.label(sm > np.quantile(sm, q))[0].astype(np.int32)                # noqa: E731
    thin, thick, core, marker = label(0.65), label(0.79), label(0.91), label(0.86)
    thin = np.where(thick != 0, thick, (thin + thick.max()) * (thin != 0)).astype(np.int32)
    ids = lambda vol: np.arange(1, int(vol.max()) + 1, dtype=np.int32)                      # noqa: E731
    out = dict(core_label=core, thick_anvil_label=thick, thin_anvil_label=thin, anvil_marker_label=marker,
               core=ids(core), anvil=ids(thin), anvil_marker=ids(marker))
    index = np.asarray(ndi.maximum(thick, core, ids(core)), np.int32)                       # every core lies inside a thick anvil
    index[::3] = 0                                                                          # ... and a third of them go unlinked
    out["core_anvil_index"] = index
    rng = np.random.default_rng(6)
    grid = ((rng.random(SHAPE) < 0.002) * rng.integers(1, 4, SHAPE)).astype(np.int32)
    times = np.datetime64("2018-06-19T17:00", "ns") + np.arange(SHAPE[0]) * np.timedelta64(MINUTES, "m")
    edge = v.get_edge_filter({"glm_flashes": grid, "t": times}, MARGIN, TIME_MARGIN)
    inside = np.where(edge, grid, 0).astype(np.int32)
    out.update(glm_grid=grid, t=times, edge_filter=edge, glm_in_margin=inside, n_glm_in_margin=float(inside.sum()),
               glm_distance=np.array(v.get_marker_distance_cylinder(inside, TIME_MARGIN)),
               field=rng.random(SHAPE))
    assert min(len(out[c]) for c in ("core", "anvil", "anvil_marker")) >= 3 and index.max() > 0 and inside.sum() > 100
    return out


def _detection_ds():
    from tobac_flow_amd.dataset import LabelDataset
    p = _product()
    ds = LabelDataset(coords={c: p[c].copy() for c in ("core", "anvil", "anvil_marker")})
    for name in ("core_label", "thick_anvil_label", "thin_anvil_label", "anvil_marker_label"):
        ds.add(name, p[name].copy(), ("t", "y", "x"))
    ds.add("core_anvil_index", p["core_anvil_index"].copy(), ("core",))
    return ds


def _variables(ds):
    return {name: np.asarray(value) for name, value in ds.items()}


@functools.lru_cache(maxsize=None)
def _linked():
    """tests/props_cases.linked_case on PROPS_SHAPE with volumes smoother still than _product's: the restatement the case is
    held to loops over the ids once per run (do not modify)"""
    import scipy.ndimage as ndi
    import props_cases as pc
    from oracle import np_dataset
    sm = _blobs(PROPS_SHAPE, 8, 20.0)
    label = lambda q: ndi.label(sm > np.quantile(sm, q))[0].astype(np.int32)                # noqa: E731
    thin, thick, core = label(0.65), label(0.79), label(0.91)
    thin = np.where(thick != 0, thick, (thin + thick.max()) * (thin != 0)).astype(np.int32)
    ref = {"core_label": core, "thick_anvil_label": thick, "thin_anvil_label": thin, "coords": {}}
    np_dataset.add_label_coords(ref)
    np_dataset.link_cores_and_anvils(ref)
    np_dataset.add_step_labels(ref)
    np_dataset.add_label_coords(ref)
    np_dataset.link_step_labels(ref)
    g = pc.grid(PROPS_SHAPE, 8)
    ref["coords"] = dict(ref["coords"], x=g["x"], y=g["y"], t=g["t"])
    ref.update(area=g["area"], lat=g["lat"], lon=g["lon"])
    return ref


def _props_ds():
    from tobac_flow_amd.dataset import LabelDataset
    case = _linked()
    ds = LabelDataset(coords={k: np.array(x) for k, x in case["coords"].items()})
    for name, value in case.items():
        if name == "coords":
            continue
        if name.endswith("_label"):
            ds.add(name, value.copy(), ("t", "y", "x"))
        else:
            ds[name] = np.array(value)
    return ds


# ---- the cases ----------------------------------------------------------------------------------------------------------
def calculate_flow():
    import tobac_flow_amd.flow as tf
    forward, backward = tf.calculate_flow(_scene()[0].copy(), model="Farneback", vr_steps=1, smoothing_passes=1, interp_method="cubic")
    return dict(forward=forward, backward=backward)


def create_flow():
    flow = _flow(_fields()[0])
    return dict(forward=flow.forward_flow, backward=flow.backward_flow)


def detect_cores():
    from tobac_flow_amd.detection import detect_cores as recipe
    bt, wvd, swd = _fields()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        core = recipe(_flow(bt), bt, wvd, swd, wvd_threshold=0.25, bt_threshold=0.5, overlap=0.5, absolute_overlap=4,
                      subsegment_shrink=0.0, min_length=2, use_wvd=False)
    return dict(core=np.asarray(core))


def _anvil_chain(upto):
    """the script's anvil calls, each result coming back as the next call's `markers=` / `anvil_labels`"""
    from tobac_flow_amd.detection import detect_anvils, get_anvil_markers, relabel_anvils
    bt, wvd, swd = _fields()
    flow = _flow(bt)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out["markers"] = get_anvil_markers(flow, wvd - swd, threshold=-5, overlap=0.5, absolute_overlap=4, subsegment_shrink=0.0, min_length=2)
        if upto >= 1:
            out["thick0"] = detect_anvils(flow, wvd - swd, markers=out["markers"], upper_threshold=-5, lower_threshold=-12.5,
                                          erode_distance=2, min_length=2)
        if upto >= 2:
            out["thick"] = relabel_anvils(flow, out["thick0"], markers=out["markers"], overlap=0.5, absolute_overlap=4, min_length=2)
            out["thin"] = detect_anvils(flow, wvd + swd, markers=out["thick"], upper_threshold=0, lower_threshold=-7.5,
                                        erode_distance=2, min_length=2)
    return {k: np.asarray(x) for k, x in out.items()}


def get_anvil_markers():
    return _anvil_chain(0)


def detect_anvils():
    return _anvil_chain(1)


def relabel_anvils():
    return _anvil_chain(2)


def _anvils_from(flow, wvd, swd, markers):
    """a returned marker volume coming back as `markers=`"""
    from tobac_flow_amd.detection import detect_anvils as recipe
    return np.asarray(recipe(flow, wvd - swd, markers=markers, upper_threshold=-5, lower_threshold=-12.5, erode_distance=2, min_length=2))


def detect_growth_markers():
    from tobac_flow_amd.detection import detect_growth_markers as recipe
    bt, wvd, swd = _fields()
    flow = _flow(bt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        smoothed, markers = recipe(flow, wvd)
        assert int(np.max(markers)) >= 1
        return dict(smoothed=np.asarray(smoothed), markers=np.asarray(markers), anvils=_anvils_from(flow, wvd, swd, markers))


def detect_growth_markers_multichannel():
    from tobac_flow_amd.detection import detect_growth_markers_multichannel as recipe
    bt, wvd, swd = _fields()
    flow = _flow(bt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wvd_s, bt_s, markers = recipe(flow, wvd, bt, min_length=2, lower_threshold=0.05, upper_threshold=0.1)
        assert int(np.max(markers)) >= 1
        return dict(wvd_s=np.asarray(wvd_s), bt_s=np.asarray(bt_s), markers=np.asarray(markers), anvils=_anvils_from(flow, wvd, swd, markers))


def get_marker_distance_cylinder():
    from tobac_flow_amd import validation as v
    distance, closest = v.get_marker_distance_cylinder(_product()["core_label"].copy(), 2, get_closest=True)
    return dict(distance=distance, closest=closest)


def get_marker_distance():
    from tobac_flow_amd import validation as v
    return dict(distance=v.get_marker_distance(_product()["core_label"].copy(), 1))


def get_marker_distance_ellipse_dev():
    from tobac_flow_amd import validation as v
    distance, closest = v.get_marker_distance_ellipse_dev(_product()["core_label"].copy(), 2, MARGIN)
    return dict(distance=distance, closest=closest)


def get_min_dist_for_objects():
    from tobac_flow_amd import validation as v
    p = _product()
    return dict(minima=v.get_min_dist_for_objects(p["field"].copy(), p["thick_anvil_label"].copy()))


def flash_list():
    from tobac_flow_amd import validation as v
    return dict(voxel=v.flash_list(_product()["glm_grid"].copy()).voxel.cpu().numpy())


def get_edge_filter_dev():
    from tobac_flow_amd import validation as v
    p = _product()
    got = v.get_edge_filter_dev({"glm_flashes": p["glm_grid"].copy(), "t": p["t"].copy()}, MARGIN, TIME_MARGIN).cpu().numpy()
    assert np.array_equal(got, p["edge_filter"])
    return dict(edge_filter=got)


def _operands():
    p = _product()
    return [p["glm_in_margin"].copy(), p["glm_distance"].copy(), p["edge_filter"].copy(), p["n_glm_in_margin"]]


def validate_markers():
    from tobac_flow_amd import validation as v
    p = _product()
    names = ("flash_distance", "flash_closest", "marker_distance", "pod", "far", "n_marker_in_margin", "margin_flag")
    got = v.validate_markers(p["core_label"].copy(), *_operands(), coord=p["core"].copy(), margin=MARGIN, time_margin=TIME_MARGIN, get_closest=True)
    return {name: np.asarray(x) for name, x in zip(names, got)}


def validate_wrappers():
    from tobac_flow_amd import validation as v
    from tobac_flow_amd.dataset import LabelDataset
    out = LabelDataset()
    for wrapper in (v.validate_cores, v.validate_cores_with_anvils, v.validate_anvils, v.validate_anvils_with_cores, v.validate_anvil_markers):
        wrapper(_detection_ds(), out, *_operands(), MARGIN, TIME_MARGIN, get_closest=True)
    return _variables(out)


def validate_detection():
    from tobac_flow_amd import validation as v
    p = _product()
    return _variables(v.validate_detection(_detection_ds(), {"glm_flashes": p["glm_grid"].copy(), "t": p["t"].copy()}, MARGIN, TIME_MARGIN,
                                           get_closest=True))


def calculate_label_properties():
    from test_gpu_label_props import _compare
    from tobac_flow_amd.dataset import calculate_label_properties as stage
    ds = _props_ds()
    before = set(ds)
    stage(ds)
    _compare(ds, before, _linked())                                # every variable at the bounds of the function's own test
    return {name: np.asarray(ds[name]) for name in set(ds) - before if np.asarray(ds[name]).dtype.kind in "iumM"}


def get_label_stats():
    from tobac_flow_amd.analysis import get_label_stats as stage
    ds = _props_ds()
    before = set(ds)
    stage("thick_anvil_label", ds)
    stage(ds["core_step_label"], ds, name="core_step")
    return {name: np.asarray(ds[name]) for name in set(ds) - before}


def labeled_comprehension():
    """host labels beside a device field, and a host field beside device labels: the mixed calls are the ones that upload"""
    import torch
    from tobac_flow_amd.utils import label_utils as lu
    p = _product()
    field = p["field"].astype(np.float32)
    field_dev, labels_dev = torch.from_numpy(field).cuda(), torch.from_numpy(p["thick_anvil_label"]).cuda()
    highest = lu.labeled_comprehension(field_dev, p["thick_anvil_label"].copy(), np.nanmax, default=np.nan)
    lowest = lu.apply_func_to_labels(labels_dev, field.copy(), func=np.nanmin, default=np.nan)
    return dict(highest=np.asarray(highest), lowest=lowest.cpu().numpy() if isinstance(lowest, torch.Tensor) else np.asarray(lowest))


CASES = {f.__name__: f for f in (
    calculate_flow, create_flow, detect_cores, get_anvil_markers, detect_anvils, relabel_anvils, detect_growth_markers,
    detect_growth_markers_multichannel, get_marker_distance_cylinder, get_marker_distance, get_marker_distance_ellipse_dev,
    get_min_dist_for_objects, flash_list, get_edge_filter_dev, validate_markers, validate_wrappers, validate_detection,
    calculate_label_properties, get_label_stats, labeled_comprehension)}
assert set(SITES.values()) <= set(CASES)
