"""The watershed SET-UP restated in plain NumPy, and the seeded cases that take it down every path of its dispatch.

The set-up (tobac_flow_amd/csrc/watershed.hip, ws_job_begin) classifies the voxels, finds the RELEVANT set -- floodable
voxels plus the markers that have a floodable out-neighbour -- numbers it in tile order, builds the compact neighbour table
and sizes the workspace from the count R (stats[6]).  Restated:

    cls  = 2 where markers != 0, else 1 where mask is None or mask != 0, else 0
    r(a) = 0 where isnan(a) else np.round(a)          (half to even; flow[..., 0] is x, flow[..., 1] is y)
    neighbour i of (t, y, x) = (t + dt, y + dy + s_y, x + dx + s_x),  s = r(fwd[t, y, x]) if dt == +1,
                               r(bwd[t, y, x]) if dt == -1, else 0;  missing if outside the volume
    relevant = (cls == 1) | ((cls == 2) & any_i(cls[neighbour i] == 1))
    R = relevant.sum()

No GPU import here.  tests/test_ws_setup_cases_cpu.py holds the restatement against the oracle's flood (a marker that is
not relevant can be taken out without changing any other label) and states what every case must contain;
tests/test_gpu_ws_setup.py holds the library against both.
"""
import zlib

import numpy as np

from helpers import rand_field

FLOW_VALUES = np.array([-20, -7.5, -2.5, -1.5, -0.5, 0, 0.5, 1.5, 2.5, 3.5, 20], np.float32)
MASK_VALUES = np.array([1, 2, -1, -128], np.int8)            # "set" is != 0, whatever the byte

# shape (T, H, W) -> what it reaches
TINY = [(1, 1, 1), (1, 1, 3)]                 # N < 4: the tail of k_ws_classify4 alone; one padded tile
SHAPES = [(1, 5, 5),                          # N = 25: quads plus a tail; H, W < 16
          (2, 16, 16),                        # exactly one full tile per frame; the 6x4 path
          (3, 17, 20),                        # W % 4 == 0; an edge tile one row high and one four columns wide
          (2, 15, 33), (4, 5, 37),            # W % 4 != 0: generic relevance at connectivity 1; the ragged cid store
          (3, 33, 48)]                        # three tile rows and columns; the 6x4 grid has more lanes than quads


# ---- the restatement ------------------------------------------------------------------------------------------------

def classes(markers, mask):
    floodable = np.ones(markers.shape, bool) if mask is None else np.asarray(mask) != 0
    return np.where(np.asarray(markers) != 0, 2, np.where(floodable, 1, 0)).astype(np.uint8)


def round_flow(a):
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(0), np.round(a)).astype(np.int64)


def nan_to_zero(flow):
    """the flows the oracle is given: it cannot round NaN itself, the library's rule is NaN -> 0"""
    return np.where(np.isnan(flow), np.float32(0), flow).astype(np.float32)


def floodable_neighbours(cls, fwd, bwd, offsets):
    """(n, T, H, W) bool: neighbour i of the voxel exists and is floodable (class 1)"""
    T, H, W = cls.shape
    t, y, x = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    fx, fy, bx, by = round_flow(fwd[..., 0]), round_flow(fwd[..., 1]), round_flow(bwd[..., 0]), round_flow(bwd[..., 1])
    out = np.zeros((len(offsets),) + cls.shape, bool)
    for i, (dt, dy, dx) in enumerate(np.asarray(offsets, np.int64)):
        sy = fy if dt == 1 else by if dt == -1 else 0
        sx = fx if dt == 1 else bx if dt == -1 else 0
        tt, yy, xx = t + dt, y + dy + sy, x + dx + sx
        inside = (tt >= 0) & (tt < T) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        out[i][inside] = cls[tt[inside], yy[inside], xx[inside]] == 1
    return out


def relevant(case, offsets):
    """bool (T, H, W): the relevant set of `case` under the neighbour list `offsets`"""
    cls = classes(case["markers"], case["mask"])
    return (cls == 1) | ((cls == 2) & floodable_neighbours(cls, case["fwd"], case["bwd"], offsets).any(0))


def temporal_only(case, offsets):
    """bool (T, H, W): markers that are relevant ONLY through a flow-displaced t -+ 1 neighbour"""
    cls = classes(case["markers"], case["mask"])
    hit = floodable_neighbours(cls, case["fwd"], case["bwd"], offsets)
    in_time = np.asarray(offsets)[:, 0] != 0
    return (cls == 2) & hit[in_time].any(0) & ~hit[~in_time].any(0)


def relevant_by_loops(case, offsets):
    """the same definition voxel by voxel (a check of the vectorised form above, for small volumes)"""
    cls = classes(case["markers"], case["mask"])
    T, H, W = cls.shape
    out = np.zeros(cls.shape, bool)
    for t in range(T):
        for y in range(H):
            for x in range(W):
                if cls[t, y, x] != 2:
                    out[t, y, x] = cls[t, y, x] == 1
                    continue
                for dt, dy, dx in np.asarray(offsets).tolist():
                    s = case["fwd"][t, y, x] if dt == 1 else case["bwd"][t, y, x] if dt == -1 else np.zeros(2, np.float32)
                    sx, sy = (0 if np.isnan(v) else int(np.round(v)) for v in s)
                    tt, yy, xx = t + dt, y + dy + sy, x + dx + sx
                    if 0 <= tt < T and 0 <= yy < H and 0 <= xx < W and cls[tt, yy, xx] == 1:
                        out[t, y, x] = True
                        break
    return out


# ---- neighbour lists ------------------------------------------------------------------------------------------------

def ten_structure():
    """the structure of test_watershed_custom_structure_and_inf_field: the in-plane 8-neighbourhood + the two temporal ones"""
    st = np.zeros((3, 3, 3), bool)
    st[1] = True
    st[0, 1, 1] = st[2, 1, 1] = True
    return st


def diagonal_structure():
    """six entries that are not the six faces: the four in-plane diagonals + the two temporal neighbours"""
    st = np.zeros((3, 3, 3), bool)
    st[1, ::2, ::2] = True
    st[0, 1, 1] = st[2, 1, 1] = True
    return st


def neighbour_lists():
    """name -> (n, 3) int8 (dt, dy, dx), the same list for the oracle and for watershed_dev"""
    from oracle import ws_oracle
    faces = ws_oracle.neighbour_offsets(1)
    lists = {"conn1": faces, "conn2": ws_oracle.neighbour_offsets(2), "conn3": ws_oracle.neighbour_offsets(3),
             "faces_reversed": faces[::-1], "diagonals6": ws_oracle.neighbour_offsets(diagonal_structure()),
             "custom10": ws_oracle.neighbour_offsets(ten_structure())}
    assert [len(v) for v in lists.values()] == [6, 18, 26, 6, 6, 10]
    return {k: np.ascontiguousarray(v, np.int8) for k, v in lists.items()}


NEIGHBOUR_LISTS = ("conn1", "conn2", "conn3", "faces_reversed", "diagonals6", "custom10")


# ---- the cases ------------------------------------------------------------------------------------------------------

def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _flows(rng, shape, nan_frac):
    out = []
    for _ in range(2):
        f = rng.choice(FLOW_VALUES, size=shape + (2,))
        if nan_frac:
            f[rng.random(f.shape) < nan_frac] = np.nan
        out.append(np.ascontiguousarray(f, np.float32))
    return out


def _case(name, family, shape, field, markers, mask, fwd, bwd):
    return dict(name=name, family=family, shape=shape, field=np.ascontiguousarray(field, np.float32),
                markers=np.ascontiguousarray(markers, np.int32), mask=None if mask is None else np.ascontiguousarray(mask, np.int8),
                fwd=fwd, bwd=bwd)


def _box(shape, cy, cx, r=3):
    return slice(max(cy - r, 0), min(cy + r + 1, shape[1])), slice(max(cx - r, 0), min(cx + r + 1, shape[2]))


def blob_case(shape, zero_flow=False):
    """7 x 7 marker blobs (clipped at the border) whose interiors are irrelevant.  Blobs sit in the corners of the first and of
    the last frame -- every face and corner of the volume is touched where the blobs fit without overlapping -- one more
    runs through ALL frames with zero flow inside (its interior is irrelevant whatever the other flows do), one has a
    negative id, and one lies wholly inside a hole of the mask.  The mask has random holes besides."""
    T, H, W = shape
    name = "blobs_%dx%dx%d%s" % (shape + ("_zero_flow" if zero_flow else "",))
    rng = _rng(name)
    fwd, bwd = [np.zeros(shape + (2,), np.float32)] * 2 if zero_flow else _flows(rng, shape, 0.02)
    fwd, bwd = fwd.copy(), bwd.copy()
    markers = np.zeros(shape, np.int32)
    mask = rng.choice(MASK_VALUES, size=shape)
    mask[rng.random(shape) < 0.12] = 0
    taken = np.zeros(shape, bool)                                # blobs and a one-voxel margin round them
    placed = []

    def place(frames, cy, cx, ident):
        ys, xs = _box(shape, cy, cx)
        my, mx = _box(shape, cy, cx, 4)
        if taken[frames, my, mx].any():
            return False
        markers[frames, ys, xs] = ident
        taken[frames, my, mx] = True
        placed.append((frames, ys, xs))
        return True

    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    ident = 1
    for frame, order in ((0, corners), (T - 1, corners[::-1])):
        for cy, cx in order:
            if place(slice(frame, frame + 1), cy, cx, -7 if ident == 2 else ident):
                ident += 1
    if place(slice(0, T), H // 2, W // 2, ident):                # through all frames, zero flow inside
        frames, ys, xs = placed[-1]
        fwd[frames, ys, xs] = 0
        bwd[frames, ys, xs] = 0
        ident += 1
    for _ in range(20):                                          # one blob wholly outside the mask, where there is room
        cy, cx, t = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(0, T))
        if place(slice(t, t + 1), cy, cx, ident):
            my, mx = _box(shape, cy, cx, 4)
            mask[t, my, mx] = 0
            ident += 1
            break
    return _case(name, "blobs", shape, rand_field(rng, shape), markers, mask, fwd, bwd)


def temporal_case(shape):
    """Every even frame is entirely markers (one id per voxel), every odd frame entirely floodable apart from some masked-out
    voxels: a marker can only be relevant through its flow-displaced t -+ 1 neighbours, which land on a floodable voxel, on a
    masked one or outside.  In k_ws_relevant6x4 all four bytes of every quad go through `need`."""
    T, H, W = shape
    assert T >= 2
    name = "temporal_%dx%dx%d" % shape
    rng = _rng(name)
    fwd, bwd = _flows(rng, shape, 0.0)
    markers = np.zeros(shape, np.int32)
    markers[::2] = np.arange(1, T * H * W + 1, dtype=np.int32).reshape(shape)[::2]
    mask = rng.choice(MASK_VALUES, size=shape)
    mask[rng.random(shape) < 0.15] = 0
    return _case(name, "temporal", shape, rand_field(rng, shape), markers, mask, fwd, bwd)


def tiny_cases():
    out = []
    for name, shape, markers, mask in (("tiny_1x1x1_floodable", (1, 1, 1), [0], None), ("tiny_1x1x1_marker", (1, 1, 1), [4], None),
                                       ("tiny_1x1x3", (1, 1, 3), [5, 0, 0], [1, -1, 0]), ("tiny_1x1x3_masked_marker", (1, 1, 3), [0, 0, -2], [2, 0, 0])):
        rng = _rng(name)
        fwd, bwd = _flows(rng, shape, 0.0)
        out.append(_case(name, "tiny", shape, rand_field(rng, shape), np.array(markers, np.int32).reshape(shape),
                         None if mask is None else np.array(mask, np.int8).reshape(shape), fwd, bwd))
    return out


_CASES = {}


def cases():
    """name -> case (built once; treat as read-only)"""
    if not _CASES:
        for c in tiny_cases() + [blob_case(s) for s in SHAPES] + [blob_case((3, 17, 20), zero_flow=True)] \
                + [temporal_case(s) for s in SHAPES if s[0] >= 2]:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            _CASES[c["name"]] = c
    return _CASES


CASE_NAMES = (["tiny_1x1x1_floodable", "tiny_1x1x1_marker", "tiny_1x1x3", "tiny_1x1x3_masked_marker"]
              + ["blobs_%dx%dx%d" % s for s in SHAPES] + ["blobs_3x17x20_zero_flow"]
              + ["temporal_%dx%dx%d" % s for s in SHAPES if s[0] >= 2])


_ORACLE = {}


def oracle_labels(name, nbr_name):
    """the oracle's labels of a case under a neighbour list (computed once, shared; NaN flows given as 0)"""
    from oracle import ws_oracle
    key = (name, nbr_name)
    if key not in _ORACLE:
        c = cases()[name]
        _ORACLE[key] = ws_oracle.watershed(nan_to_zero(c["fwd"]), nan_to_zero(c["bwd"]), c["field"], c["markers"], c["mask"],
                                           offsets=neighbour_lists()[nbr_name])
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]
