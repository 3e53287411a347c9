"""The step-level convolve API without a GPU: the three names import, their signatures are the reference's
(tobac_flow/convolve.py:8-245, written out here), and every argument error is raised before any device work."""
import inspect

import numpy as np
import pytest
import scipy.ndimage as ndi

E = inspect.Parameter.empty
NAN = float("nan")

# (name, default) in order, as the reference declares them
SIGNATURES = {
    "warp_flow": [("img", E), ("flow", E), ("method", "linear"), ("fill_value", NAN), ("offsets", np.array([[0, 0]])),
                  ("res", None), ("grid_locs", None)],
    "convolve_same_step": [("img", E), ("offsets", E), ("fill_value", NAN), ("res", None), ("grid_locs", None)],
    "convolve_step": [("prev_step", E), ("same_step", E), ("next_step", E), ("forward_flow", E), ("backward_flow", E),
                      ("structure", ndi.generate_binary_structure(3, 1)), ("method", "linear"), ("dtype", np.float32),
                      ("fill_value", NAN), ("res", None), ("grid_locs", None)],
}


def _same_default(a, b):
    if a is E or b is E:
        return a is b
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a is b or (type(a) is type(b) and a == b)


def test_the_three_names_import():
    from tobac_flow_amd.convolve import convolve_same_step, convolve_step, warp_flow  # noqa: F401
    import tobac_flow_amd.convolve as c
    assert {"warp_flow", "convolve_same_step", "convolve_step", "convolve"} <= set(c.__all__)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_is_the_references(name):
    import tobac_flow_amd.convolve as c
    params = list(inspect.signature(getattr(c, name)).parameters.values())
    assert [p.name for p in params] == [n for n, _ in SIGNATURES[name]]
    for p, (n, default) in zip(params, SIGNATURES[name]):
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, n
        assert _same_default(p.default, default), (n, p.default, default)


@pytest.fixture
def no_device(monkeypatch):
    """any upload, allocation or library call fails the test: the errors below must come first"""
    from tobac_flow_amd import _lib

    def boom(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    for name in ("to_dev", "empty", "lib", "device", "stream_ptr"):
        monkeypatch.setattr(_lib, name, boom)


IMG = np.zeros((5, 6), np.float32)
FLOW = np.zeros((5, 6, 2), np.float32)
GRID = np.stack(np.meshgrid(np.arange(6), np.arange(5)), -1)


def test_bad_method_raises(no_device):
    from tobac_flow_amd.convolve import convolve_step, warp_flow
    msg = r"method must be one of \['nearest', 'linear', 'cubic', 'lanczos'\]"
    with pytest.raises(ValueError, match=msg):
        warp_flow(IMG, FLOW, method="bilinear")
    with pytest.raises(ValueError, match=msg):
        convolve_step(IMG, IMG, IMG, FLOW, FLOW, method="quintic")


def test_structure_errors_raise(no_device):
    from tobac_flow_amd.convolve import convolve_step
    with pytest.raises(ValueError, match="structure must have three dimensions"):
        convolve_step(IMG, IMG, IMG, FLOW, FLOW, structure=np.ones((3, 3), bool))
    with pytest.raises(ValueError, match="leading dimension of structure must have length 3"):
        convolve_step(IMG, IMG, IMG, FLOW, FLOW, structure=np.ones((5, 3, 3), bool))


def test_non_integral_same_step_offsets_raise(no_device):
    from tobac_flow_amd.convolve import convolve_same_step
    with pytest.raises(ValueError, match="offsets must be integer-valued"):
        convolve_same_step(IMG, np.array([[0.5, 0.0], [1.0, 1.0]]))
    with pytest.raises(ValueError, match="offsets must be integer-valued"):
        convolve_same_step(IMG, [[0, 0], [np.nan, 1]], grid_locs=GRID)


@pytest.mark.parametrize("bad", ["half", "nan"])
def test_non_integral_grid_locs_raise(no_device, bad):
    from tobac_flow_amd.convolve import convolve_same_step, convolve_step, warp_flow
    grid = GRID.astype(np.float64)
    grid[2, 3, 0] = 3.5 if bad == "half" else np.nan
    with pytest.raises(ValueError, match="grid_locs must hold integer values"):
        warp_flow(IMG, FLOW, grid_locs=grid)
    with pytest.raises(ValueError, match="grid_locs must hold integer values"):
        convolve_same_step(IMG, [[0, 1]], grid_locs=grid)
    with pytest.raises(ValueError, match="grid_locs must hold integer values"):
        convolve_step(IMG, IMG, IMG, FLOW, FLOW, grid_locs=grid)


def test_integer_image_needs_nearest(no_device):
    from tobac_flow_amd.convolve import convolve_step, warp_flow
    lab = np.zeros((5, 6), np.int32)
    with pytest.raises(ValueError, match="nearest"):
        warp_flow(lab, FLOW, method="linear", fill_value=0)
    with pytest.raises(ValueError, match="nearest"):
        convolve_step(lab, lab, lab, FLOW, FLOW, method="cubic", dtype=np.int32, fill_value=0)


def test_abi_version_is_bumped_and_the_entry_points_are_bound():
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() > 100                 # 100: the ABI before tf_warp_offsets / tf_gather_offsets / tf_convolve_step
    for name in ("tf_warp_offsets", "tf_gather_offsets", "tf_convolve_step"):
        assert name in _lib.EXPORTS and hasattr(L, name)

