"""The level plan of the Farneback host driver (csrc/fb_plan.h), without a GPU: the plan checked against itself
(tools/fb_plan_check.cpp) and the library's size functions and batch hint against figures of the commit before the plan
existed.  None of these calls touches a device; the hint assumes 256 CUs where none answers, which is the MI355X's count."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_agrees_with_itself(tmp_path):
    """tools/fb_plan_check.cpp over 12 shapes x 3 pyramid scales x 2 window sizes x 3 level counts x 6 batch sizes x 4 part
    counts: carving stays inside the reported bytes, arrays and pairs do not overlap, every level's sampled blur rows and
    hand-over words fit the tmp stride, the phases join at FB_SPLIT_LEVEL, level 0 lands in slot 0 for 1 .. 10 iterations, and
    the size functions compose as documented (its first lines give the AddressSanitizer / UBSan command; here a plain build)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "fb_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "fb_plan_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "plan consistent" in out.stdout, out.stdout + out.stderr


# taken from the library of the parent commit (hand-written size formulas in farneback.hip), which the plan must reproduce:
# (H, W, overrides of the defaults) -> {(function, arguments): value}
PARENT_SIZES = [
    ((5424, 5424, {}), {("one",): 2000596736, ("batch", 42): 84024727040, ("split", 42, 2): 42012367616, ("phase", 42, 1): 7413910016,
                        ("phase", 23, 2): 46013544704, ("hint", 1024, 115 * 10 ** 9): 42, ("hint", 54, 0): 42, ("hint", 43, 0): 42,
                        ("hint", 41, 0): 41, ("hint", 1024, 8 * 10 ** 9): 3}),
    ((3712, 3712, {}), {("split", 23, 23): 1901508352}),
    ((131, 140, {}), {("batch", 3): 3759104, ("split", 3, 2): 2508800, ("phase", 3, 1): 351488, ("phase", 2, 2): 2508800}),
    ((203, 331, dict(win_size=9)), {("split", 23, 3): 47333376}),
    ((333, 517, dict(pyr_scale=0.6, win_size=9)), {("batch", 5): 76470272, ("split", 5, 3): 76470272, ("phase", 5, 1): 0}),
    ((1500, 2500, dict(pyr_scale=0.8)), {("batch", 2): 528010752, ("hint", 1024, 8 * 10 ** 9): 23}),
    ((65, 127, dict(num_levels=1)), {("phase", 3, 1): 0}),
    ((33, 70, {}), {("batch", 1): 175616}),
    ((1, 1, dict(num_levels=0)), {("one",): 28160}),
]


@pytest.mark.parametrize("geom,want", PARENT_SIZES, ids=[f"{g[0]}x{g[1]}" for g, _ in PARENT_SIZES])
def test_sizes_and_hint_are_those_of_the_hand_written_formulas(geom, want):
    from tobac_flow_amd import _lib
    L = _lib.lib()
    H, W, over = geom
    kw = dict(dict(num_levels=5, pyr_scale=0.5, win_size=13, num_iters=10, poly_n=5, poly_sigma=1.1), **over)
    p = _lib.FarnebackParams(kw["num_levels"], kw["pyr_scale"], kw["win_size"], kw["num_iters"], kw["poly_n"], kw["poly_sigma"], 0, 0)
    fns = {"one": lambda: L.tf_farneback_workspace_bytes(H, W, ctypes.byref(p)),
           "batch": lambda B: L.tf_farneback_workspace_bytes_batch(B, H, W, ctypes.byref(p)),
           "split": lambda B, parts: L.tf_farneback_workspace_bytes_split(B, parts, H, W, ctypes.byref(p)),
           "phase": lambda B, phase: L.tf_farneback_workspace_bytes_phase(B, H, W, ctypes.byref(p), phase),
           "hint": lambda max_pairs, max_bytes: L.tf_farneback_batch_hint(H, W, ctypes.byref(p), max_pairs, max_bytes)}
    for (name, *args), value in want.items():
        assert fns[name](*args) == value, (name, args)
