"""CPU checks of tests/gather_cases.py: the path classifier on hand-made coordinates, and -- for every input family
of tests/test_gpu_gather_geometry.py -- the pixel counts per class that the GPU tests rely on (asserted and printed)."""
import numpy as np
import pytest

import gather_cases as gc

F = np.float32


def _plane(fx, fy, H, W, method, x, y):
    """classes of pixel (x, y) of an H x W plane whose flow is (fx, fy) everywhere"""
    fl = np.empty((H, W, 2), F)
    fl[..., 0], fl[..., 1] = fx, fy
    return {k: bool(v[y, x]) for k, v in gc.plane_classes(fl, method).items() if k not in ("ax", "ay")}


def test_loc_and_rounding_restate_the_kernel():
    assert gc.cvround(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], F)).tolist() == [0, 2, 2, 0, -2, -2]
    # (k + 0.5) / 32 falls on a bin tie: half to even
    assert gc.bin32(np.array([16.5 / 32, 17.5 / 32, -16.5 / 32, -17.5 / 32], F)).tolist() == [16, 18, -16, -18]
    # negative bins: arithmetic shift and two's-complement mask, as `fx >> 5` and `fx & 31` on the device
    b = gc.bin32(np.array([-1 / 32, -33 / 32], F))
    assert (b >> 5).tolist() == [-1, -2] and (b & 31).tolist() == [31, 31]
    # the coordinate is rounded twice: flow + off in float32, then + grid through float64
    f = np.nextafter(F(0.515625), F(np.inf))
    assert gc.loc(f, 0, 0) == f and gc.loc(f, 1, 0) == F(1.515625)          # the neighbour is rounded away at exponent 0
    assert gc.loc(F(0.25), 0, 16384) == F(16384.25) and gc.loc(F(2.0 ** -12), 0, 16384) == F(16384.0)
    assert gc.loc(F(3 * 2.0 ** -11), 0, 16384) == F(16384.0 + 2.0 ** -9)    # a float32 tie of the SUM: to even


def test_plane_classifier_on_each_side_of_each_limit():
    H, W = 12, 20
    for method, P, first in (("linear", 4, 0), ("cubic", 6, 1)):
        # zero flow: tap 0 is the pixel to the upper left, the patch starts at (x - 1 - first, y - 1 - first)
        x0, y0 = 1 + first, 1 + first                       # bx == 0, by == 0: the first pixel on the fast path
        c = _plane(0, 0, H, W, method, x0, y0)
        assert c["fast"] and c["x_lo_in0"] and c["y_lo_in0"] and not c["edge"]
        c = _plane(0, 0, H, W, method, x0 - 1, y0 + 1)      # bx == -1 only
        assert c["edge"] and c["x_lo_out1"] and not c["y_lo_out1"] and not c["fast"]
        c = _plane(0, 0, H, W, method, x0 + 1, y0 - 1)      # by == -1 only
        assert c["edge"] and c["y_lo_out1"] and not c["x_lo_out1"]
        c = _plane(0, 0, H, W, method, x0 - 1, y0 - 1)      # two limits fail: `edge`, but no `_out1` witness
        assert c["edge"] and not c["x_lo_out1"] and not c["y_lo_out1"]
        x1, y1 = W - P + 1 + first, H - P + 1 + first       # bx + P == W, by + P == H: the last pixel on the fast path
        c = _plane(0, 0, H, W, method, x1, y1)
        assert c["fast"] and c["x_hi_in0"] and c["y_hi_in0"]
        c = _plane(0, 0, H, W, method, x1 + 1, y1)
        assert c["edge"] and c["x_hi_out1"] and not c["y_hi_out1"]
        c = _plane(0, 0, H, W, method, x1, y1 + 1)
        assert c["edge"] and c["y_hi_out1"] and not c["x_hi_out1"]
        # a flow of -1/32 px moves the integer part down by one (negative bins round towards minus infinity)
        c = _plane(-1 / 32, 0, H, W, method, x0, y0 + 1)
        assert c["edge"] and c["x_lo_out1"]
        # a patch larger than the image never fits
        assert not gc.plane_classes(np.zeros((P - 1, P - 1, 2), F), method)["fast"].any()
    # taps that do not line up: the tap at flow + 1 is rounded onto the bin tie, the tap at flow is above it
    f = np.nextafter(F(16.5 / 32), F(np.inf))
    c = _plane(f, 0, H, W, "cubic", 0, 5)
    assert c["unaligned"] and not c["fast"] and not c["edge"]
    c = _plane(F(16.5 / 32), 0, H, W, "cubic", 8, 5)
    assert c["fast"]                                        # the exact tie rounds alike for the three taps


def test_tap_classifier_branches():
    H, W = 10, 10
    z = np.zeros(1, F)
    for method, R, first in (("linear", 2, 0), ("cubic", 4, 1), ("lanczos", 8, 3)):
        cls = lambda x, y: {k for k, v in gc.tap_classes(z + F(x), z + F(y), H, W, method).items() if v[0]}   # noqa: E731
        assert cls(first, first) == {"inside"} and cls(W - R + first, H - R + first) == {"inside"}
        assert cls(first - 1, first) == {"straddle"} and cls(first, H - R + first + 1) == {"straddle"}
        assert cls(first - R, first) == {"outside"} and cls(W + first, first) == {"outside"}
        assert cls(first - R + 31 / 32, first) == {"outside"} and cls(first - R + 1, first) == {"straddle"}
        assert cls(first - 1 / 32, first) == {"straddle"}   # the bin below an integer belongs to the pixel before it
        assert cls(1e6, 3) == {"outside"} and cls(3, -1e6) == {"outside"}
    cls = lambda x, y: {k for k, v in gc.tap_classes(z + F(x), z + F(y), H, W, "nearest").items() if v[0]}       # noqa: E731
    assert cls(-0.5, 9.5) == {"outside"}                    # -0.5 -> 0 but 9.5 -> 10
    assert cls(-0.5, 8.5) == {"inside"} and cls(9.5, 0) == {"outside"} and cls(-0.5000001, 0) == {"outside"}


def _report(name, method, counts):
    print(f"{name:18s} {method:8s} " + " ".join(f"{k}={v}" for k, v in counts.items()))


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_border_sweep_reaches_both_sides_of_every_limit_at_every_phase(method):
    cases = gc.family("border_sweep")
    assert sorted({c["data"].shape for c in cases}) == sorted(gc.SWEEP_SHAPES)
    counts = gc.family_counts("border_sweep", method)
    _report("border_sweep", method, counts)
    gc.require(counts, gc.PLANE_KEYS + ("inside", "straddle", "outside", "miss_inside", "miss_straddle", "miss_outside"),
               f"border sweep, {method}")
    assert counts["unaligned"] == 0                         # k / 32 at small coordinates is exact: nothing but the borders here
    # every k = -96 .. 96 occurs in x and in y on a plane that reads a real frame, negative coordinates included
    fl = np.concatenate([gc.warped_planes(c)[:, 0, 0] for c in cases])
    for comp in (0, 1):
        assert set(np.rint(fl[:, comp] * 32).astype(int)) == set(gc.SWEEP_K.tolist())
    # ... and next to each limit, on either side of it, every sub-pixel phase 0 .. 31 occurs
    seen = {}
    for c in cases:
        pc = gc.plane_classes(gc.warped_planes(c), method)
        for L in gc.LIMITS:
            for side in ("_out1", "_in0"):
                seen.setdefault(L + side, set()).update(pc["ax" if L[0] == "x" else "ay"][pc[L + side]].tolist())
    assert all(v == set(range(32)) for v in seen.values()), {k: sorted(set(range(32)) - v) for k, v in seen.items()}


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_bin_ties_reach_the_unaligned_path_and_exact_ties_stay_aligned(method):
    cases = gc.family("bin_ties")
    assert [c["data"].shape for c in cases] == [(3, 8, 4096), (3, 4096, 8)]
    counts = gc.family_counts("bin_ties", method)
    _report("bin_ties", method, counts)
    gc.require(counts, gc.PLANE_KEYS + ("unaligned", "inside", "straddle", "outside"), f"bin ties, {method}")
    for c in cases:                                         # per volume: x is the long axis in one, y in the other
        counts = gc.count_classes([c], method)
        _report(c["name"], method, counts)
        gc.require(counts, ("fast", "edge", "unaligned", "inside", "straddle", "outside"), f"{c['name']}, {method}")
        # exact ties (half to even decides the bin) on the fast path, with an even and with an odd bin below them
        fl = gc.warped_planes(c)
        fast = gc.plane_classes(fl, method)["fast"]
        for comp in (0, 1):
            t = fl[..., comp].astype(np.float64) * 32 - 0.5
            tie = fast & (t == np.rint(t))
            for parity in (0, 1):
                assert np.count_nonzero(tie & (np.rint(t).astype(np.int64) % 2 == parity)) >= gc.MIN_PIXELS
            # one-ulp neighbours of a tie, kept apart from it by the float32 coordinate (small coordinates only)
            near = (np.nextafter(fl[..., comp], F(np.inf)).astype(np.float64) * 32 - 0.5) % 1 == 0
            assert np.count_nonzero(near) >= gc.MIN_PIXELS


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_large_coordinates_cover_every_class_beyond_2_to_the_11(method):
    cases = gc.family("large_coordinates")
    assert [c["data"].shape for c in cases] == [(3, 6, 32767), (3, 32767, 6)]
    counts = gc.family_counts("large_coordinates", method)
    _report("large_coordinates", method, counts)
    gc.require(counts, gc.PLANE_KEYS + ("unaligned", "inside", "straddle", "outside"), f"large coordinates, {method}")
    for c, axis in zip(cases, (2, 1)):
        counts = gc.count_classes([c], method)
        _report(c["name"], method, counts)
        gc.require(counts, ("fast", "edge", "unaligned", "inside", "straddle", "outside"), f"{c['name']}, {method}")
        # the unaligned pixels are not all at small coordinates: every octave from 2^11 to the ABI limit holds some
        un = gc.plane_classes(gc.warped_planes(c), method)["unaligned"]
        pos = np.nonzero(un)[axis]
        for lo in (2048, 4096, 8192, 16384):
            n = np.count_nonzero((pos >= lo) & (pos < 2 * lo))
            print(f"  unaligned at coordinate [{lo}, {2 * lo}): {n}")
            assert n >= gc.MIN_PIXELS


def test_nearest_ties_hit_exact_halves_at_even_and_odd_pixels_at_both_borders():
    cases = gc.family("nearest_ties")
    counts = gc.family_counts("nearest_ties", "nearest")
    _report("nearest_ties", "nearest", counts)
    gc.require(counts, ("inside", "outside", "miss_inside", "miss_outside"), "nearest ties")
    beyond = {}
    for c in cases:
        fl = gc.warped_planes(c)
        H, W = fl.shape[1:3]
        for comp, n in ((0, W), (1, H)):
            g = (np.arange(W)[None, None, :] if comp == 0 else np.arange(H)[None, :, None]) + np.zeros(fl.shape[:3], int)
            f = fl[..., comp]
            for v in gc.NEAREST_TIES:
                for parity in (0, 1):                       # an exact half at an even and at an odd pixel
                    assert np.count_nonzero((f == v) & (g % 2 == parity)) >= gc.MIN_PIXELS, (c["name"], comp, v, parity)
                for other in (np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))):
                    assert np.count_nonzero(f == other) >= gc.MIN_PIXELS
            m = gc.loc(f, 0, g)
            assert np.count_nonzero(m == F(-0.5)) >= 4 and np.count_nonzero(m == F(n - 0.5)) >= 4      # the ties ON the two borders
            for side, mask in (("lo", gc.cvround(m) < 0), ("hi", gc.cvround(m) >= n)):
                beyond[comp, side] = beyond.get((comp, side), 0) + int(np.count_nonzero(mask))
    print("nearest pixels beyond each border (component, side):", beyond)
    assert len(beyond) == 4 and min(beyond.values()) >= gc.MIN_PIXELS


@pytest.mark.parametrize("method", ["nearest", "linear", "cubic", "lanczos"])
def test_far_outside_mixes_all_outside_pixels_with_ordinary_ones(method):
    cases = gc.family("far_outside")
    counts = gc.family_counts("far_outside", method)
    _report("far_outside", method, counts)
    gc.require(counts, ("inside", "outside", "miss_inside", "miss_outside"), f"far outside, {method}")
    for c in cases:
        fl = np.concatenate([c["fwd"], c["bwd"]])
        big = np.abs(fl).max(-1)
        assert big.max() <= 1e6 and big.max() > 3e5 and np.isfinite(fl).all()
        assert (big.max() + 32768) * 32 < 2 ** 31            # cvRound(x * 32) stays an int32
        assert np.count_nonzero(big > 1e3) >= gc.MIN_PIXELS and np.count_nonzero(big < 4) >= gc.MIN_PIXELS


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_field_value_cases_hold_what_they_claim(method):
    cases = gc.family("field_values")
    counts = gc.family_counts("field_values", method)
    _report("field_values", method, counts)
    gc.require(counts, gc.PLANE_KEYS + ("inside", "straddle", "outside"), f"field values, {method}")
    by = {}
    for c in cases:
        by.setdefault(c["name"].rstrip("0123456789x"), []).append(c["data"])
    assert all(len(v) == len(gc.SWEEP_SHAPES) for v in by.values()) and len(by) == 6
    for d in by["plateau"] + by["plateau0flow"]:
        assert gc.plateau_share(d) >= 0.3 and np.mean(d == 0) >= 0.3, (d.shape, gc.plateau_share(d))
    for d in by["inf"]:
        pos, neg = np.isposinf(d), np.isneginf(d)
        assert pos.any() and neg.any()
        assert (pos[:, :, :-1] & neg[:, :, 1:]).any() and (pos[:, :-1] & pos[:, 1:]).any()      # inf - inf in both forms
    for d in by["nan"]:
        n = np.isnan(d)
        assert (n[:, 1:-1, 1:-1] & n[:, :-2, 1:-1] & n[:, 2:, 1:-1] & n[:, 1:-1, :-2] & n[:, 1:-1, 2:]).any()   # a NaN centre in a block
        assert n.any() and not n.all()
    small = np.concatenate([np.abs(d[d != 0]).ravel() for d in by["mag"]])
    assert (small < 1e-30).sum() >= gc.MIN_PIXELS and (small > 1e30).sum() >= gc.MIN_PIXELS
    with np.errstate(over="ignore"):
        d = by["mag"][0]
        assert np.isinf(d[:, :, 1:] - d[:, :, :-1]).any()    # a float32 difference that overflows
