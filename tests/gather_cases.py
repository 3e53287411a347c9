"""Inputs for the semi-Lagrangian gather tests, and a host-side classifier of the path each pixel takes.

The classifier restates PREDICATES of tobac_flow_amd/csrc/convolve.hip and remap_dev.h -- how a sampling coordinate
is built (`tf_loc`), how it is rounded (`tf_cvround`), when `sobel_plane_taps` takes its shared-patch path and which
border branch `tf_remap` takes -- never the interpolation arithmetic: expected values always come from the oracle.
The tests use it to assert that an input really reaches the class it claims to cover before anything is compared.
"""
import numpy as np

from helpers import rand_field, rand_flow

MIN_PIXELS = 32                       # a claimed class / limit must hold at least this many pixels
LIMITS = ("x_lo", "x_hi", "y_lo", "y_hi")
SWEEP_SHAPES = ((3, 9, 130), (3, 70, 7), (2, 6, 6), (2, 4, 4), (2, 5, 65))
_FOOT = {"linear": (2, 0), "cubic": (4, 1), "lanczos": (8, 3)}       # footprint size, offset of its first tap


# ----------------------------------------------------------------------------- the predicates
def loc(flow, off, grid):
    """tf_loc: float(double(float(flow + off)) + grid), the coordinate numpy builds in the reference."""
    l = (np.asarray(flow, np.float32) + np.float32(off)).astype(np.float32)
    return (l.astype(np.float64) + np.asarray(grid, np.float64)).astype(np.float32)


def cvround(v):
    """tf_cvround: round half to even."""
    return np.rint(np.asarray(v, np.float32)).astype(np.int64)


def bin32(m):
    """cvRound(m * 32) of a float32 coordinate: the 1/32-px bin (the product by 32 is exact)."""
    return cvround(np.asarray(m, np.float32) * np.float32(32))


def _grids(shape2):
    H, W = shape2
    return np.arange(W)[None, :], np.arange(H)[:, None]


def plane_classes(flow, method):
    """One warped 9-tap plane of k_sobel27.  flow: (..., H, W, 2) float32.  Returns boolean masks of shape (..., H, W):
    `fast` / `edge` / `unaligned` (a partition); per limit L `L_out1`: aligned, ONLY that limit fails, by exactly one
    pixel (bx == -1, bx + P == W + 1, the same in y) and `L_in0`: on the fast path with no room left at that limit;
    and the sub-pixel phases `ax`, `ay` (0 .. 31) of tap 0."""
    assert method in ("linear", "cubic")
    flow = np.asarray(flow, np.float32)
    H, W = flow.shape[-3:-1]
    gx, gy = _grids((H, W))
    fx = [bin32(loc(flow[..., 0], o, gx)) for o in (-1, 0, 1)]
    fy = [bin32(loc(flow[..., 1], o, gy)) for o in (-1, 0, 1)]
    aligned = (fx[0] + 32 == fx[1]) & (fx[1] + 32 == fx[2]) & (fy[0] + 32 == fy[1]) & (fy[1] + 32 == fy[2])
    R, first = _FOOT[method]
    P = R + 2
    bx, by = (fx[0] >> 5) - first, (fy[0] >> 5) - first
    fail = {"x_lo": bx < 0, "x_hi": bx + P > W, "y_lo": by < 0, "y_hi": by + P > H}
    by_one = {"x_lo": bx == -1, "x_hi": bx + P == W + 1, "y_lo": by == -1, "y_hi": by + P == H + 1}
    at_limit = {"x_lo": bx == 0, "x_hi": bx + P == W, "y_lo": by == 0, "y_hi": by + P == H}
    inside = ~(fail["x_lo"] | fail["x_hi"] | fail["y_lo"] | fail["y_hi"])
    out = {"fast": aligned & inside, "edge": aligned & ~inside, "unaligned": ~aligned,
           "ax": fx[0] & 31, "ay": fy[0] & 31}
    for L in LIMITS:
        others = np.zeros_like(aligned)
        for M in LIMITS:
            if M != L:
                others |= fail[M]
        out[L + "_out1"] = aligned & by_one[L] & ~others
        out[L + "_in0"] = out["fast"] & at_limit[L]
    return out


def tap_classes(mx, my, H, W, method):
    """The border branch tf_remap takes for one tap at float32 coordinates (mx, my): `inside` / `straddle` / `outside`."""
    if method == "nearest":
        sx, sy = np.clip(cvround(mx), -32768, 32767), np.clip(cvround(my), -32768, 32767)
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        return {"inside": inside, "straddle": np.zeros_like(inside), "outside": ~inside}
    R, first = _FOOT[method]
    bx = np.clip(bin32(mx) >> 5, -32768, 32767) - first
    by = np.clip(bin32(my) >> 5, -32768, 32767) - first
    inside = (bx >= 0) & (bx < max(W - R + 1, 0)) & (by >= 0) & (by < max(H - R + 1, 0))
    outside = ~inside & ((bx >= W) | (bx + R <= 0) | (by >= H) | (by + R <= 0))
    return {"inside": inside, "straddle": ~inside & ~outside, "outside": outside}


def warped_planes(case):
    """The (frame, flow) pairs whose warped plane reads a REAL frame: plane 0 of t >= 1 through the backward flow and
    plane 2 of t <= T - 2 through the forward flow, stacked to (n, H, W, 2); the others read the all-fill frame."""
    T = case["fwd"].shape[0]
    return np.concatenate([case["bwd"][1:], case["fwd"][:T - 1]], 0)


def missing_planes(case):
    """The two planes that stand in for the missing frames -1 and T (tf_remap_const)."""
    return np.stack([case["bwd"][0], case["fwd"][-1]], 0)


def count_classes(cases, method):
    """Pixel counts per class of `plane_classes` (warped planes that read a real frame) and per branch of `tap_classes`
    (centre tap; `miss_*`: the planes that read the all-fill frame) summed over `cases`."""
    n = {}

    def add(key, mask):
        n[key] = n.get(key, 0) + int(np.count_nonzero(mask))
    for c in cases:
        H, W = c["fwd"].shape[1:3]
        gx, gy = _grids((H, W))
        for tag, fl in (("", warped_planes(c)), ("miss_", missing_planes(c))):
            for k, m in tap_classes(loc(fl[..., 0], 0, gx), loc(fl[..., 1], 0, gy), H, W, method).items():
                add(tag + k, m)
        if method in ("linear", "cubic"):
            for k, m in plane_classes(warped_planes(c), method).items():
                if k not in ("ax", "ay"):
                    add(k, m)
    return n


def require(counts, keys, what=""):
    """The coverage condition: every claimed class holds at least MIN_PIXELS pixels."""
    short = {k: counts.get(k, 0) for k in keys if counts.get(k, 0) < MIN_PIXELS}
    assert not short, f"{what}: classes below {MIN_PIXELS} pixels: {short}"


PLANE_KEYS = ("fast", "edge") + tuple(L + s for L in LIMITS for s in ("_out1", "_in0"))


# ----------------------------------------------------------------------------- (a) border sweep
SWEEP_K = np.arange(-96, 97)                  # flows k / 32: every phase, +-3 px
SWEEP_VARIANTS = 16


def _case(name, data, fwd, bwd):
    return {"name": name, "data": np.ascontiguousarray(data, np.float32), "fwd": np.ascontiguousarray(fwd, np.float32),
            "bwd": np.ascontiguousarray(bwd, np.float32)}


def border_sweep():
    """Flows constant per frame, k / 32: consecutive (frame, direction) slots walk two independent permutations of
    k = -96 .. 96, so that over the five shapes x 16 variants every k occurs in x and in y on a plane that reads a real
    frame; the pixels of a frame then put the patch at every distance to the four borders."""
    rng = np.random.default_rng(101)
    px, py = rng.permutation(SWEEP_K), rng.permutation(SWEEP_K)
    cases, n = [], {True: 0, False: 0}
    for shape in SWEEP_SHAPES:
        T = shape[0]
        for v in range(SWEEP_VARIANTS):
            fwd, bwd = np.zeros(shape + (2,), np.float32), np.zeros(shape + (2,), np.float32)
            # the slots that read a real frame walk the permutations on their own, so that they alone cover every k
            slots = [(bwd, t, True) for t in range(1, T)] + [(fwd, t, True) for t in range(T - 1)]
            for arr, t, real in slots + [(bwd, 0, False), (fwd, T - 1, False)]:
                arr[t, ..., 0] = np.float32(px[n[real] % len(px)]) / np.float32(32)
                arr[t, ..., 1] = np.float32(py[n[real] % len(py)]) / np.float32(32)
                n[real] += 1
            cases.append(_case(f"sweep{shape[1]}x{shape[2]}v{v}", rand_field(rng, shape, smooth=(0.5, 1, 1)), fwd, bwd))
    return cases


# ----------------------------------------------------------------------------- (b) bin ties and near-ties
def _tie_candidates(rng, shape, grid):
    """Candidate flow components around the bin ties (k + 0.5) / 32, k random in +-96: the exact tie, its float32
    neighbours, and the tie moved by half the float32 spacing of the finished coordinate (then the three taps
    flow - 1, flow, flow + 1, rounded at different exponents, do not all fall on the same side of a bin limit) with ITS
    neighbours.  Returns (9,) + shape."""
    k = rng.integers(-96, 97, size=shape)
    tie = ((k + 0.5) / 32).astype(np.float32)
    half = (np.spacing((np.abs(tie) + np.broadcast_to(grid, shape)).astype(np.float32)) / 2).astype(np.float32)
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    out = [tie, np.nextafter(tie, up), np.nextafter(tie, dn)]
    for b in ((tie + half).astype(np.float32), (tie - half).astype(np.float32)):
        out += [b, np.nextafter(b, up), np.nextafter(b, dn)]
    return np.stack(out)


def _unaligned_1d(f, grid):
    b = [bin32(loc(f, o, grid)) for o in (-1, 0, 1)]
    return (b[0] + 32 != b[1]) | (b[1] + 32 != b[2])


def tie_flow(rng, shape, rounds=6):
    """(T, H, W, 2) flows made of tie candidates.  Half of the pixels keep a random candidate; for the other half the
    classifier searches `rounds` draws for a component whose three taps do not line up (`unaligned`)."""
    T, H, W = shape
    gx, gy = _grids((H, W))
    flow = np.empty(shape + (2,), np.float32)
    for comp, grid in ((0, gx), (1, gy)):
        pick = rng.integers(0, 9, size=shape)
        cand = _tie_candidates(rng, shape, grid)
        cur = np.take_along_axis(cand, pick[None], 0)[0]
        want = rng.random(shape) < 0.5
        for _ in range(rounds):
            cand = _tie_candidates(rng, shape, grid)
            for j in range(cand.shape[0]):
                take = want & ~_unaligned_1d(cur, grid) & _unaligned_1d(cand[j], grid)
                cur = np.where(take, cand[j], cur)
        flow[..., comp] = cur
    return flow


def bin_ties():
    rng = np.random.default_rng(202)
    cases = []
    for shape in ((3, 8, 4096), (3, 4096, 8)):
        cases.append(_case(f"ties{shape[1]}x{shape[2]}", rand_field(rng, shape, smooth=(0.5, 1, 1)),
                           tie_flow(rng, shape), tie_flow(rng, shape)))
    return cases


# ----------------------------------------------------------------------------- (c) large coordinates
def large_coordinates():
    """The ABI's extent limits.  A smooth +-3 px flow; every fourth column / row of the long axis carries tie flows."""
    rng = np.random.default_rng(303)
    cases = []
    for shape in ((3, 6, 32767), (3, 32767, 6)):
        flows = []
        for _ in range(2):
            f = rand_flow(rng, shape, 1.5)
            t = tie_flow(rng, shape, rounds=3)
            sel = np.zeros(shape, bool)
            if shape[2] > shape[1]:
                sel[:, :, ::4] = True
            else:
                sel[:, ::4, :] = True
            f[sel] = t[sel]
            flows.append(f)
        cases.append(_case(f"large{shape[1]}x{shape[2]}", rand_field(rng, shape, smooth=(0.5, 1, 1)), *flows))
    return cases


# ----------------------------------------------------------------------------- (d) nearest ties
NEAREST_TIES = np.array([s * h for s in (-1, 1) for h in (0.5, 1.5, 2.5)], np.float32)


def nearest_ties():
    """Per-pixel flows exactly +-0.5, +-1.5, +-2.5 and their float32 neighbours, on shapes where every pixel is within
    reach of a border in one direction and even / odd coordinates alternate."""
    rng = np.random.default_rng(404)
    vals = np.concatenate([NEAREST_TIES, np.nextafter(NEAREST_TIES, np.float32(np.inf)),
                           np.nextafter(NEAREST_TIES, np.float32(-np.inf))])
    cases = []
    for shape in ((3, 9, 130), (3, 70, 7)):
        fwd = vals[rng.integers(0, len(vals), size=shape + (2,))]
        bwd = vals[rng.integers(0, len(vals), size=shape + (2,))]
        cases.append(_case(f"nearest{shape[1]}x{shape[2]}", rand_field(rng, shape, smooth=(0.5, 1, 1)), fwd, bwd))
    return cases


def labels_of(case):
    """int32 labels on the grid of `case` (distinct neighbours, some background)."""
    T, H, W = case["data"].shape
    rng = np.random.default_rng(H * 1000 + W)
    lab = rng.integers(1, 1000, size=(T, H, W)).astype(np.int32)
    lab[rng.random((T, H, W)) < 0.3] = 0
    return lab


# ----------------------------------------------------------------------------- (e) far outside
def far_outside():
    """Finite flows up to +-1e6 px on about half of the pixels (every warped tap outside), in-range flows on the rest."""
    rng = np.random.default_rng(505)
    cases = []
    for shape in ((3, 9, 130), (3, 70, 7)):
        flows = []
        for _ in range(2):
            f = rand_flow(rng, shape, 1.5)
            far = rng.random(shape) < 0.5
            mag = (10.0 ** rng.uniform(1.5, 6.0, size=shape + (2,)) * rng.choice([-1.0, 1.0], size=shape + (2,)))
            f[far] = mag.astype(np.float32)[far]
            flows.append(f)
        cases.append(_case(f"far{shape[1]}x{shape[2]}", rand_field(rng, shape, smooth=(0.5, 1, 1)), *flows))
    return cases


# ----------------------------------------------------------------------------- (f) field values
def _sweep_flow(rng, shape):
    return (rng.integers(-96, 97, size=(shape[0], 1, 1, 2)) / 32.0).astype(np.float32) * np.ones(shape + (2,), np.float32)


def field_values():
    """On the sweep shapes, with smooth +-3 px flows: plateaus / exact zeros, infinities, NaNs, extreme magnitudes."""
    rng = np.random.default_rng(606)
    cases = []
    for shape in SWEEP_SHAPES:
        T, H, W = shape
        base = rand_field(rng, shape, smooth=(0.5, 1, 1))

        def flows():
            return rand_flow(rng, shape, 1.5, smooth=1.0), rand_flow(rng, shape, 1.5, smooth=1.0)
        # plateaus: the field is cut into two levels (70 % of it exactly zero) along a smooth contour
        lvl = rand_field(rng, shape, smooth=(2, 3, 3))
        plat = np.where(lvl > np.quantile(lvl, 0.3), np.float32(0), np.float32(2.5))
        plat[rng.random(shape) < 0.004] = 1.0                                          # a few single steps
        cases.append(_case(f"plateau{H}x{W}", plat, *flows()))
        cases.append(_case(f"plateau0flow{H}x{W}", plat, np.zeros(shape + (2,), np.float32), np.zeros(shape + (2,), np.float32)))
        inf = base.copy()
        r = rng.random(shape)
        inf[r < 0.04] = np.inf
        inf[(r >= 0.04) & (r < 0.08)] = -np.inf
        inf[:, H // 2, : min(W, 3)] = (np.inf, -np.inf, np.inf)[: min(W, 3)]           # adjacent: inf - inf
        inf[:, : min(H, 2), W // 2] = np.inf                                           # adjacent: inf - inf of one sign
        cases.append(_case(f"inf{H}x{W}", inf, *flows()))
        nan = base.copy()
        nan[rng.random(shape) < 0.06] = np.nan
        nan[:, H // 3: H // 3 + 3, W // 3: W // 3 + 3] = np.nan                         # a block: NaN centre, NaN taps
        cases.append(_case(f"nan{H}x{W}", nan, *flows()))
        mag = base.copy()
        sel = rng.random(shape)
        mag = np.where(sel < 0.3, base * np.float32(1e-30), np.where(sel < 0.6, base * np.float32(1e30), base))
        mag = np.where(sel > 0.9, np.sign(base) * np.float32(3e38), mag).astype(np.float32)
        cases.append(_case(f"mag{H}x{W}", mag, *flows()))
        cases.append(_case(f"magsweep{H}x{W}", mag, _sweep_flow(rng, shape), _sweep_flow(rng, shape)))
    return cases


def plateau_share(data):
    """Share of the pixels whose whole 3 x 3 x 3 neighbourhood (clipped at the volume's faces) is one value."""
    import scipy.ndimage as ndi
    return float(np.mean(ndi.maximum_filter(data, 3, mode="nearest") == ndi.minimum_filter(data, 3, mode="nearest")))


FAMILIES = {"border_sweep": border_sweep, "bin_ties": bin_ties, "large_coordinates": large_coordinates,
            "nearest_ties": nearest_ties, "far_outside": far_outside, "field_values": field_values}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def family_counts(name, method):
    """count_classes over a whole family, computed once per process"""
    if (name, method) not in _cache:
        _cache[name, method] = count_classes(family(name), method)
    return _cache[name, method]
