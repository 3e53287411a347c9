"""Inputs for the tests of the scipy.ndimage glue (tobac_flow_amd/csrc/morph.hip), and host-side restatements of the
decisions its dispatch takes.

Pure numpy / SciPy: no torch, no GPU.  Nothing here computes an expected VALUE for a GPU test -- those always come from
SciPy or the host numpy functions.  What is restated is which edges the run-based union-find of tf_label selects
(`ccl_model`: k_ccl_init_runs and k_ccl_union<RUNS>) and which kernel form tf_binary_morph picks for a geometry
(`morph_form`), so that the tests can ASSERT that a case reaches the rule or path it is named for before anything is
compared (tests/test_glue_cases_cpu.py without a GPU, tests/test_gpu_glue_paths.py on one).
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

COUNTERS = ("head", "join", "rule3", "rule4", "no_sibling", "union", "plain")


# ----------------------------------------------------------------------------- structures for tf_label
def symmetric_structures():
    """all 8192 centro-symmetric 3 x 3 x 3 structures with the centre on, as a (8192, 3, 3, 3) bool array: bit i of the
    index switches the pair of flat cells (i, 26 - i), i = 0 .. 12 (bit 12 is the x pair, (0, 0, -1) / (0, 0, +1))"""
    k = np.arange(8192)
    flat = np.zeros((8192, 27), bool)
    flat[:, 13] = True
    for i in range(13):
        flat[:, i] = flat[:, 26 - i] = (k >> i) & 1
    return flat.reshape(8192, 3, 3, 3)


def has_x_tap(structure):
    """the structure holds the horizontal tap (0, 0, +1): tf_label takes the run-based kernels"""
    return bool(np.asarray(structure)[1, 1, 2])


def _taps(*offsets):
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for dt, dy, dx in offsets:
        s[1 + dt, 1 + dy, 1 + dx] = s[1 - dt, 1 - dy, 1 - dx] = True
    return s


def _connectivity(c):
    d = np.abs(np.indices((3, 3, 3)) - 1).sum(0)
    return d <= c


def _flat(s):
    s = s.copy()
    s[0] = s[2] = False
    return s


def named_structures():
    """the deterministic subset used on the larger volumes: {name: (3, 3, 3) bool}"""
    out = {}
    for c in (1, 2, 3):
        out[f"conn{c}"] = _connectivity(c)
        out[f"flat{c}"] = _flat(_connectivity(c))
    out["centre_only"] = _taps()
    out["x_only"] = _taps((0, 0, 1))
    out["y_only"] = _taps((0, 1, 0))
    out["t_only"] = _taps((1, 0, 0))
    # diagonals without their axis siblings, alone (no runs) ...
    out["diag_yx"] = _taps((0, 1, 1), (0, 1, -1))
    out["diag_tx"] = _taps((1, 0, 1), (1, 0, -1))
    out["diag_tyx"] = _taps((1, 1, 1), (1, -1, -1), (1, 1, -1), (1, -1, 1))
    out["diag_ty"] = _taps((1, 1, 0), (1, -1, 0))
    # ... and beside the x tap: the run path, rule (iv) must NOT skip them (their sibling bit is clear)
    out["x_diag_yx"] = _taps((0, 0, 1), (0, 1, 1), (0, 1, -1))
    out["x_diag_tx"] = _taps((0, 0, 1), (1, 0, 1), (1, 0, -1))
    out["x_diag_tyx"] = _taps((0, 0, 1), (1, 1, 1), (1, -1, -1), (1, 1, -1), (1, -1, 1))
    out["x_one_diag"] = _taps((0, 0, 1), (0, 1, -1))
    out["x_t"] = _taps((0, 0, 1), (1, 0, 0))
    cube = np.ones((3, 3, 3), bool)
    cube[1, 1, 0] = cube[1, 1, 2] = False
    out["cube_minus_x"] = cube
    rng = np.random.default_rng(8192)
    everything = symmetric_structures()
    for want_x in (True, False):                      # 24 seeded random structures with the x tap, 24 without
        pool = np.nonzero(everything[:, 1, 1, 2] == want_x)[0]
        for k in rng.choice(pool, 24, replace=False):
            out[f"random{'_x' if want_x else ''}_{int(k):04d}"] = everything[k]
    return out


# ----------------------------------------------------------------------------- the edge selection of tf_label
def forward_taps(structure):
    """the taps tf_label keeps: the structure's cells with flat index > 13, in C order, as (dt, dy, dx)"""
    s = np.asarray(structure) != 0
    assert s.shape == (3, 3, 3) and np.array_equal(s, s[::-1, ::-1, ::-1]), "structure must be centro-symmetric"
    return [(i // 9 - 1, (i // 3) % 3 - 1, i % 3 - 1) for i in range(14, 27) if s.flat[i]]


def _pq(d, n):
    """slices of the voxels p and of their neighbours q = p + d along one axis of length n"""
    return slice(max(0, -d), max(0, n - max(0, d))), slice(max(0, d), max(0, n - max(0, -d)))


def ccl_model(mask, structure, seg=64, ignore_sibling=False):
    """Host restatement of the EDGE SELECTION of tf_label: which pairs of voxels k_ccl_init_runs and k_ccl_union<RUNS> join.
    The components of that edge set are then numbered by ascending smallest raster index (what k_ccl_flatten and the
    root ranking do).  Returns (labels int32, n_labels, counts); the labels equal scipy.ndimage.label(mask, structure)
    iff the selected edges connect exactly what the structure connects.  counts:
      head        voxels whose initial parent is the head of their run within the `seg`-lane row segment (rule i)
      join        runs joined across a segment boundary by the thread with threadIdx.x == 0 (rule ii)
      rule3       dx == 0 taps skipped because the left neighbours of p and q are both set (rule iii)
      rule4       dx != 0 taps skipped because (x, y') is set and the structure holds the sibling tap (rule iv)
      no_sibling  dx != 0 taps where (x, y') is set but the sibling is absent: rule (iv) must not skip, a union is made
      union       unions made by k_ccl_union<true>
      plain       unions made by k_ccl_union<false> (structure without the (0, 0, +1) tap)
    ignore_sibling=True models the WRONG rule (iv) that skips whenever (x, y') is set: the CPU tests use it to show that a
    mask tells the two behaviours apart.
    """
    m = np.asarray(mask) != 0
    T, H, W = m.shape
    taps = forward_taps(structure)
    runs = (0, 0, 1) in taps
    idx = np.arange(m.size).reshape(m.shape)
    x = np.arange(W)
    counts = dict.fromkeys(COUNTERS, 0)
    ea, eb = [], []

    def join(sel, a, b):
        ea.append(a[sel])
        eb.append(b[sel])
        return int(np.count_nonzero(sel))

    left = np.zeros_like(m)                              # `left` of k_ccl_union: x > 0 && in[p - 1], for a set voxel p
    left[..., 1:] = m[..., 1:] & m[..., :-1]
    if runs:
        # k_ccl_init_runs: the parent of a set voxel is the nearest voxel at or before it in its segment that starts a run
        start = m & ~(left & (x % seg != 0))
        head = np.maximum.accumulate(np.where(start, idx, -1), axis=2)
        counts["head"] = join(m & ~start, idx, head)
        counts["join"] = join(left & (x % seg == 0), idx, idx - 1)
    for dt, dy, dx in taps:
        if runs and dt == 0 and dy == 0:
            continue                                     # the horizontal tap: done by the runs
        (pt, qt), (py, qy), (px, qx) = _pq(dt, T), _pq(dy, H), _pq(dx, W)
        both = m[pt, py, px] & m[qt, qy, qx]
        skip = np.zeros_like(both)
        if runs and dx == 0:
            skip = both & left[pt, py, px] & left[qt, qy, qx]             # left && in[q - 1]
            counts["rule3"] += int(np.count_nonzero(skip))
        elif runs:
            below = both & m[qt, qy, px]                 # in[q - dx]: the voxel (x, y') under / over p
            if (dt, dy, 0) in taps or ignore_sibling:
                skip = below
                counts["rule4" if (dt, dy, 0) in taps else "no_sibling"] += int(np.count_nonzero(skip))
            else:
                counts["no_sibling"] += int(np.count_nonzero(below))
        counts["union" if runs else "plain"] += join(both & ~skip, idx[pt, py, px], idx[qt, qy, qx])
    n = m.size
    a, b = (np.concatenate(ea), np.concatenate(eb)) if ea else (np.zeros(0, int), np.zeros(0, int))
    _, comp = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(n, n)), directed=False)
    on = np.nonzero(m.ravel())[0]
    labels = np.zeros(n, np.int32)
    if on.size:
        _, first, inv = np.unique(comp[on], return_index=True, return_inverse=True)
        rank = np.empty(first.size, np.int32)
        rank[np.argsort(first)] = np.arange(1, first.size + 1)     # ascending smallest raster index of the component
        labels[on] = rank[inv]
    return labels.reshape(m.shape), int(labels.max(initial=0)), counts


# ----------------------------------------------------------------------------- label masks
# (T, H, W) of the random masks: W in {1, 2, 63, 64, 65, 127, 128, 129, 200} twice each, every (T, H) of {1, 2, 3} x {1, 3, 4, 5}
RANDOM_MASK_SHAPES = ((1, 1, 1), (2, 3, 1), (3, 1, 2), (1, 4, 2), (2, 1, 63), (3, 4, 63), (1, 3, 64), (2, 5, 64), (3, 3, 65),
                      (1, 5, 65), (2, 4, 127), (3, 5, 127), (1, 1, 128), (3, 3, 128), (2, 3, 129), (1, 4, 129), (3, 1, 200),
                      (2, 5, 200))


def _mask_case(name, mask, *claims):
    """claims: (structure name, counters that must be non-zero under it)"""
    return {"name": name, "mask": np.ascontiguousarray(mask, bool), "claims": claims}


def label_masks():
    """Named masks for tf_label.  Each declares, per structure of named_structures(), the counters of ccl_model that it
    is there to make non-zero (tests/test_glue_cases_cpu.py asserts them)."""
    rng = np.random.default_rng(64)
    out = []
    # runs crossing x = 64 k
    m = np.zeros((2, 3, 200), bool)
    m[0, 0, 60:70] = m[0, 1, 120:135] = m[0, 2, 190:200] = True
    m[1, 0, 1:199] = m[1, 2, 63:65] = m[1, 2, 127:129] = m[1, 2, 191:193] = True
    out.append(_mask_case("cross64", m, ("conn1", ("head", "join", "union")), ("conn2", ("join", "rule4"))))
    # runs that start at lane 0 and runs that end at lane 63, without and with a continuation
    m = np.zeros((1, 6, 128), bool)
    m[0, 0, 0:64] = True                                  # lane 0 .. 63, nothing beyond
    m[0, 1, 64:128] = True                                # lane 0 .. 63 of the second segment
    m[0, 2, :] = True                                     # one run over both segments
    m[0, 3, 63:65] = True                                 # starts at lane 63, ends at lane 0
    m[0, 4, 0] = m[0, 4, 63] = m[0, 4, 64] = m[0, 4, 127] = True
    m[0, 5, 62:64] = m[0, 5, 65:67] = True                # ends at lane 63 with lane 0 of the next segment clear
    out.append(_mask_case("lane0_lane63", m, ("conn1", ("head", "join", "rule3", "union")), ("x_only", ("head", "join"))))
    # widths either side of the segment size, few rows, few frames: every W twice, every (T, H) once or twice
    for j, (T, H, W) in enumerate(RANDOM_MASK_SHAPES):
        out.append(_mask_case(f"random{T}x{H}x{W}", rng.random((T, H, W)) < (0.55, 0.8)[j % 2]))
    # checkerboards: n / 2 components under connectivity 1 -- root ranks over many 256-voxel blocks
    cb = (np.indices((3, 5, 70)).sum(0) % 2) == 0
    out.append(_mask_case("checker_partial_block", cb, ("cube_minus_x", ("plain",)), ("conn2", ("union",))))    # 1050 = 4 * 256 + 26
    cb = cb.copy()
    cb.reshape(-1)[-300:] = False                         # the last 256-block (and more) holds no root
    out.append(_mask_case("checker_rootless_tail", cb, ("conn3", ("union",))))
    # staircases for the diagonal taps: thin (only the diagonal tap connects) and thick ((x, y') is set: rule iv).  Under
    # x_diag_yx a non-zero `no_sibling` count does not by itself show that the labels depend on the sibling bit: in the thick
    # dx = +1 staircase the other diagonal still joins the rows.  `pixel_over_run` and `full` are the masks built to tell
    # a rule (iv) that ignores the bit apart (tests/test_glue_cases_cpu.py shows that they do, and most random masks too).
    m = np.zeros((3, 40, 70), bool)
    k = np.arange(40)
    m[0, k, k] = True                                     # thin, dx = +1
    m[0, k, 69 - k] = True                                # thin, dx = -1
    m[1, k, k + 20] = m[1, k, k + 21] = True              # thick, dx = +1
    m[2, k, 60 - k] = m[2, k, 59 - k] = True              # thick, dx = -1
    out.append(_mask_case("staircases_yx", m, ("conn2", ("union", "rule4")), ("x_diag_yx", ("union", "no_sibling")),
                          ("diag_yx", ("plain",))))
    m = np.zeros((5, 5, 66), bool)
    k = np.arange(5)
    m[k, k, 60 + k] = m[k, k, 61 + k] = True              # thick in t, y and x, across x = 64
    m[k, 4 - k, 10 - k] = True                            # thin, the other diagonal
    m[k, 2, 30 + k] = m[k, 2, 31 + k] = True              # dy == 0: the (1, 0, +-1) taps
    out.append(_mask_case("staircases_tyx", m, ("conn3", ("union", "rule4")), ("x_diag_tyx", ("union", "no_sibling")),
                          ("x_diag_tx", ("union", "no_sibling")), ("diag_tyx", ("plain",))))
    # single pixels over / under the first pixel of a run of two or three: under x_diag_yx (no (0, 1, 0) tap) the only tap
    # that joins them is the diagonal one whose (x, y') is set -- skipping it, as rule (iv) does WITH a sibling, splits them
    m = np.zeros((2, 7, 70), bool)
    for t, y, x, n in ((0, 1, 3, 2), (0, 1, 30, 3), (0, 4, 62, 3), (1, 1, 10, 2), (1, 4, 63, 2)):
        m[t, y, x:x + n] = True
        m[t, y - 1 if t == 0 else y + 1, x if t == 0 else x + n - 1] = True
    out.append(_mask_case("pixel_over_run", m, ("x_diag_yx", ("union", "no_sibling")), ("conn2", ("rule4",))))
    # combs whose teeth join through a spine at the far end, so that the root of most voxels changes late
    m = np.zeros((1, 9, 130), bool)
    m[0, ::2, :] = True
    m[0, :, 129] = True
    out.append(_mask_case("comb_spine_right", m, ("conn1", ("head", "join", "union")), ("conn2", ("rule4",))))
    m = np.zeros((2, 8, 65), bool)
    m[:, :, ::2] = True
    m[:, 7, :] = True
    m[1] = m[1, ::-1, ::-1]
    out.append(_mask_case("comb_spine_bottom", m, ("conn1", ("head", "union")), ("y_only", ("plain",))))
    # a square spiral, one pixel wide
    m = np.zeros((1, 21, 67), bool)
    lo_y, hi_y, lo_x, hi_x = 0, 20, 0, 66
    while lo_y <= hi_y and lo_x <= hi_x:
        m[0, lo_y, lo_x:hi_x + 1] = True
        m[0, lo_y:hi_y + 1, hi_x] = True
        if lo_y + 2 <= hi_y:
            m[0, hi_y, lo_x + 2:hi_x + 1] = True
            m[0, lo_y + 2:hi_y + 1, lo_x + 2] = True
        lo_y, hi_y, lo_x, hi_x = lo_y + 2, hi_y - 2, lo_x + 2, hi_x - 2
    m[0, 1, 0] = False
    out.append(_mask_case("spiral", m, ("conn1", ("head", "join", "union"))))
    out.append(_mask_case("full", np.ones((2, 5, 130), bool), ("conn1", ("head", "join", "rule3")), ("conn3", ("rule3", "rule4")),
                          ("x_diag_yx", ("no_sibling", "union")), ("cube_minus_x", ("plain",))))
    out.append(_mask_case("empty", np.zeros((2, 5, 130), bool)))
    # voxel counts either side of the 256-voxel blocks of the root ranking; two of them with n % 4 != 0
    for shape in ((2, 2, 64), (1, 1, 257), (1, 3, 85), (3, 5, 17)):
        n = int(np.prod(shape))
        claims = (("conn1", ("union",)), ("cube_minus_x", ("plain",))) if shape[1] > 1 else (("conn1", ("head",)),)
        out.append(_mask_case(f"blocks_n{n}", rng.random(shape) < 0.5, *claims))
    return out


# ----------------------------------------------------------------------------- binary morphology
# (T, H, W).  uint4 form (W % 16 == 0): n_tiles % 8 in {0, 1, 7} at every T in {1, 2, 5}; word form: W in {4, 260}; byte
# form: W in {1, 45}.  H: 1, 3, 4, 7, 8, 9 and 55 / 57 (8 k -+ 1 with seven / eight tile rows).
MORPH_GEOMETRIES = tuple(
    [(T, H, 16) for T in (1, 2, 5) for H in (8, 55, 57)]
    + [(2, 7, 1024), (1, 3, 1040), (2, 1, 1040), (5, 4, 1040), (1, 28, 1040), (2, 9, 2064), (1, 20, 2064)]
    + [(2, 4, 4), (1, 7, 260), (5, 9, 260), (2, 1, 260)]
    + [(2, 3, 1), (1, 1, 1), (1, 8, 45), (5, 9, 45)])


def morph_form(T, H, W, misalign=0):
    """(kernel form, n_tiles) tf_binary_morph picks for a volume whose buffers all sit `misalign` bytes past a 16-byte
    boundary; n_tiles is that of k_binary_morph16's tile mapping (None for the other forms).  The formulas of
    tf_binary_morph and k_binary_morph16."""
    if W % 16 == 0 and misalign % 16 == 0:
        return "uint4", ((W // 16 + 63) // 64) * ((H + 7) // 8)
    if W % 4 == 0 and misalign % 4 == 0:
        return "word", None
    return "byte", None


def _single(dt, dy, dx):
    s = np.zeros((3, 3, 3), bool)
    s[1 + dt, 1 + dy, 1 + dx] = True
    return s


def morph_structures():
    """{name: (3, 3, 3) bool} for tf_binary_morph: the four structures of test_binary_morphology_matches_scipy, single
    off-centre taps, rows with dxmask 5, a structure without a centre, and 34 seeded random ones (asymmetric included)"""
    out = {}
    conn1 = _connectivity(1)
    out["cross2d"] = _flat(conn1)
    out["cube"] = np.ones((3, 3, 3), bool)
    out["conn1"] = conn1
    skew = np.zeros((3, 3, 3), bool)
    skew[0, 0, 1] = skew[1, 1, 1] = skew[1, 1, 2] = skew[2, 2, 0] = True
    out["skew"] = skew
    for name, d in (("tap_x+", (0, 0, 1)), ("tap_x-", (0, 0, -1)), ("tap_y+", (0, 1, 0)), ("tap_t-", (-1, 0, 0)),
                    ("tap_corner", (1, -1, 1)), ("tap_centre", (0, 0, 0))):
        out[name] = _single(*d)
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 0] = s[1, 1, 2] = True                          # dxmask 5 in the centre row alone
    out["row5"] = s
    s = np.zeros((3, 3, 3), bool)
    s[:, :, 0] = s[:, :, 2] = True                          # dxmask 5 in all nine rows
    out["rows5"] = s
    s = np.ones((3, 3, 3), bool)
    s[1, 1, 1] = False
    out["no_centre"] = s
    rng = np.random.default_rng(27)
    while len(out) < 13 + 34:
        s = rng.random((3, 3, 3)) < rng.uniform(0.1, 0.9)
        if s.any():
            out[f"random{len(out) - 13:02d}"] = s
    return out


# ----------------------------------------------------------------------------- grey morphology
def grey_footprints():
    """{name: (3, 3, 3) bool}: point-symmetric footprints ndimage_dev._grey accepts (not empty, not all 27 cells)"""
    out = {"cross2d": _flat(_connectivity(1)), "conn1": _connectivity(1), "conn2": _connectivity(2)}
    d = np.zeros((3, 3, 3), bool)
    d[0, 0, 0] = d[1, 1, 1] = d[2, 2, 2] = True
    out["diag"] = d
    out["centre_only"] = _taps()
    # first cell in C order off-centre: a NaN there sticks
    for name, offs in (("x_pair", [(0, 0, 1)]), ("corner_pair", [(1, 1, 1)]), ("t_pair", [(1, 0, 0)]), ("y_pair", [(0, 1, 0)]),
                       ("anti_corners", [(1, -1, 1), (1, 1, -1)])):
        s = _taps(*offs)
        s[1, 1, 1] = False
        out[name] = s
    s = np.ones((3, 3, 3), bool)
    s[1, 1, 1] = False
    out["all_but_centre"] = s
    s = np.zeros((3, 3, 3), bool)
    s[1] = True
    out["mid_plane"] = s
    out["conn3_minus_x"] = named_structures()["cube_minus_x"]
    rng = np.random.default_rng(13)
    k = 0
    while k < 32:
        bits = rng.random(14) < rng.uniform(0.15, 0.85)          # 13 pairs and the centre
        s = np.concatenate([bits, bits[:13][::-1]]).reshape(3, 3, 3)
        if s.any() and not s.all():
            out[f"random{k:02d}"] = s
            k += 1
    return out


# ----------------------------------------------------------------------------- elementwise kernels
ELEMENT_COUNTS = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4097)
# both orders; 0.1 / 0.7 / 0.3 are not float32 values and float32(0.7) - float32(0.1) != float32(0.7 - 0.1)
THRESHOLD_PAIRS = ((-15.0, -5.0), (-5.0, -15.0), (0.25, 3.0), (270.0, 250.0), (0.1, 0.7), (0.9, 0.3))


def special_values(lower, upper):
    """float32 vector for the elementwise kernels: NaN, +-inf, +-0, the two thresholds and 0 and 1, each with its
    neighbours one ulp either side"""
    f = np.float32
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    for c in (lower, upper, 0.0, 1.0):
        v += [f(c), np.nextafter(f(c), f(np.inf)), np.nextafter(f(c), f(-np.inf))]
    return np.array(v, f)


def element_vector(n, lower, upper, seed=0):
    """n float32 values: the special values tiled from a seed-dependent phase (so that each of them lands in the quad
    body and in the scalar tail of some count), the rest ordinary values around the thresholds"""
    rng = np.random.default_rng(1000 * seed + n)
    sv = special_values(lower, upper)
    lo, hi = min(lower, upper), max(lower, upper)
    out = rng.uniform(lo - (hi - lo), hi + (hi - lo), n).astype(np.float32)
    k = np.arange(n)
    use = (k % 2 == 0) | (n <= sv.size)
    out[use] = sv[(k[use] // (1 if n <= sv.size else 2) + seed) % sv.size]
    return out
