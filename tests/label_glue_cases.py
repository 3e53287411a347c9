"""Cases of the label glue (flat_label, flow_label / flow_link_overlap, make_step_labels, slice_labels, relabel_objects,
remap_labels, find_overlapping_labels, get_step_labels_for_label, the cross-window overlap rule and find_new_labels),
shared by tests/golden/make_label_glue_golden.py, tests/test_label_glue_cases_cpu.py and tests/test_gpu_label_glue.py.

The expected values in tests/golden/label_glue_ref.npz were written by the REFERENCE's own functions
(tobac_flow/utils/label_utils.py, tobac_flow/label.py, tobac_flow/linking.py); this module only builds the inputs, from
integers alone (PCG64 draws, box sums, floor divisions), so every platform generates the same volumes.  The fixture also
stores the inputs: a drifted generator is noticed.

Flows are INTEGER-VALUED (int8): a nearest-neighbour warp by such flows is an exact shift, so `ShiftFlow` below stands
in for the reference's OpenCV-backed Flow.convolve without a rounding question, and tobac_flow_amd's Flow, given the same
vectors as float32, samples the same pixel centres.

The two overlap rules round in opposite directions:
  flow linking    count >= overlap * min(n, size)             a PRODUCT:  0.28 * 25 == 7.000000000000001 > 7: not linked
  window linking  max(count / n, count / size) >= rtol        a QUOTIENT: 7 / 25 == 0.28: linked
`product_edge` / `quotient_edge` sit on those two boundaries with the same pair of regions (25 px and 27 px sharing 7).

What the order of the visit can and cannot change.  flow_label walks the DIRECTED neighbour relation: labels ascending,
an unvisited label opens a group and absorbs every not-yet-visited label reachable from it.  A group is therefore the set
of labels reachable from its root minus the earlier (already closed) groups, and the group numbers follow the roots:
neither depends on whether forward neighbours are visited before backward ones, or breadth before depth -- `group_model`
shows it on `visit_order` for all four orders.  What does change the result is treating the relation as symmetric (a
union-find over the pairs): in `visit_order` C sees B backwards, B does not see C forwards, B < A opens its group first
and stays alone, whereas a symmetric treatment merges B into A's object.  `check_visit_order` asserts both facts."""
import os

import numpy as np
import scipy.ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_glue_ref.npz")

# shape -> the boundary of the kernels it is the smallest to reach
SHAPES = {
    (1, 5, 65): "one frame; runs cross the 64-pixel row segment; H % 4 != 0; n % 4 != 0",
    (2, 7, 130): "three row segments; both warps; n % 256 != 0",
    (3, 33, 67): "n = 6633 crosses a 4096-voxel block; H * W odd: labels[1:] is not 16-byte aligned",
    (5, 48, 64): "everything aligned: the vector paths",
    (4, 31, 37): "odd everything, T > 3",
}
SEEDS = (0, 1, 2)                      # 0: backward = -forward; 1: independent backward; 2: + vectors up to 40 at two borders
FLOW_GRID = ((0, 0), (0.5, 0), (0.5, 4), (0.9, 1), (0.28, 0), (0, 5))          # (overlap, absolute_overlap)
WINDOW_GRID = ((5, 0.5), (0, 0.0), (1, 0.0), (3, 0.9), (0, 0.3))                # (atol, rtol); (5, 0.5) is the reference's own
QUOTIENT_GRID = ((5, 0.27), (5, 0.28), (5, 0.29), (7, 0.28), (8, 0.28), (0, 0.28), (0, 0.0))
LINK_GRID = ((0, 0), (0.5, 4))         # flow_link_overlap on make_step_labels output
FULL = np.ones((3, 3, 3), bool)
UNALIGNED, ALIGNED = (3, 33, 67), (5, 48, 64)


def shape_name(shape):
    return "x".join(str(n) for n in shape)


def grid_name(a, b):
    return f"{a:g}_{b:g}"


def pack(mask):
    """a bool volume as bytes: its shape (three uint16) and then its bits"""
    mask = np.asarray(mask, bool)
    return np.concatenate([np.array(mask.shape, "<u2").view(np.uint8), np.packbits(mask.ravel())])


def unpack(packed):
    shape = tuple(int(n) for n in packed[:6].view("<u2"))
    return np.unpackbits(packed[6:])[:int(np.prod(shape))].astype(bool).reshape(shape)


def pack_flows(forward, backward):
    """(1, T, H, W, 2) where backward == -forward, else (2, T, H, W, 2)"""
    return forward[None] if np.array_equal(backward, -forward) else np.stack([forward, backward])


def unpack_flows(stored):
    return (stored[0], stored[1]) if len(stored) == 2 else (stored[0], (-stored[0]).astype(np.int8))


def lut_of(fine, coarse):
    """the table t with coarse == t[fine], for a labelling `coarse` that is constant on every label of `fine` (both keep
    0): how the fixture stores an object volume next to the step labels it was linked from"""
    fine, coarse = np.asarray(fine), np.asarray(coarse)
    table = np.zeros(int(fine.max(initial=0)) + 1, np.int64)
    table[fine.ravel()] = coarse.ravel()
    assert table[0] == 0 and np.array_equal(table[fine], coarse), "not constant on the labels of the finer volume"
    return table


class ShiftFlow:
    """duck-typed Flow for flow_label: convolve(method="nearest") by integer-valued flows = an exact shift"""

    def __init__(self, forward, backward):
        assert forward.dtype.kind == "i" and backward.dtype.kind == "i"
        self.forward_flow, self.backward_flow, self.shape = forward, backward, forward.shape[:-1]

    @staticmethod
    def _shift(src, flow, fill_value):
        H, W = src.shape
        yy, xx = np.mgrid[:H, :W]
        x, y = xx + flow[..., 0], yy + flow[..., 1]
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, src[np.where(inside, y, 0), np.where(inside, x, 0)], fill_value)

    def convolve(self, data, structure=None, method="linear", fill_value=np.nan, dtype=np.float32, func=None):
        assert method == "nearest" and func is None and data.shape == self.shape
        s = np.asarray(structure) != 0
        assert s[0].sum() == 1 and s[0, 1, 1] and s[2].sum() == 1 and s[2, 1, 1] and not s[1].any()
        T = data.shape[0]
        out = np.full((2,) + data.shape, fill_value, dtype=dtype)
        for t in range(T):
            if t > 0:
                out[0, t] = self._shift(data[t - 1], self.backward_flow[t], fill_value)
            if t < T - 1:
                out[1, t] = self._shift(data[t + 1], self.forward_flow[t], fill_value)
        return out


def warped_labels(flat, forward, backward):
    """(back_labels, forward_labels) as label.py:133-137 asks them of the flow"""
    struct = ndi.generate_binary_structure(3, 1) * np.array([1, 0, 1])[:, None, None]
    return ShiftFlow(forward, backward).convolve(flat, structure=struct, method="nearest", dtype=np.int32, fill_value=0)


# ---- seeded volumes ---------------------------------------------------------------------------------------------------
def seeded_mask(shape, seed):
    """smoothed noise: 3 x 5 x 5 box sums of byte noise (integers only), thresholded a little above the mean"""
    T, H, W = shape
    rng = np.random.default_rng([seed, T, H, W])
    noise = rng.integers(0, 256, (T + 2, H + 4, W + 4))
    box = sum(noise[dt:dt + T, dy:dy + H, dx:dx + W] for dt in range(3) for dy in range(5) for dx in range(5))
    return box > 9562 + 200                                    # mean 75 * 127.5, sigma about 640


def seeded_flows(shape, seed):
    """int8 (T, H, W, 2) forward and backward flows in [-2, 2]: 9 x 9 box sums of integer noise, divided and rounded in
    integers.  seed 0: backward = -forward; seed 1: an independent backward flow; seed 2: independent, and vectors of
    magnitude up to 40 along the left border (forward, -x) and the bottom border (backward, +y), so that whole labels
    sample outside the frame (fill value 0)."""
    T, H, W = shape
    rng = np.random.default_rng([100 + seed, T, H, W])

    def field():
        r = rng.integers(-2, 3, (T, H + 8, W + 8, 2))
        box = sum(r[:, dy:dy + H, dx:dx + W] for dy in range(9) for dx in range(9))          # sigma about 12.7
        return np.clip((box + 5) // 10, -2, 2).astype(np.int8)

    forward = field()
    backward = (-forward).astype(np.int8) if seed == 0 else field()
    if seed == 2:
        wb, hb = max(W // 4, 1), max(H // 4, 1)
        forward[:, :, :wb, 0] = (-40 + np.arange(wb) % 3)[None, None, :]
        backward[:, H - hb:, :, 1] = (40 - np.arange(hb) % 3)[None, :, None]
    return forward, backward


def seeded_name(shape, seed):
    return f"{shape_name(shape)}/seed{seed}"


def tile_labels(shape):
    """an int32 label volume whose connected pieces hold several labels and whose labels span several pieces and steps:
    the seed-0 mask cut into 6 x 9 tiles numbered 1 .. 7"""
    T, H, W = shape
    t, y, x = np.mgrid[:T, :H, :W]
    return np.where(seeded_mask(shape, 0), ((y // 6) * 3 + x // 9 + t) % 7 + 1, 0).astype(np.int32)


def gappy(labels):
    """the same regions under ids with gaps (relabel_objects' input)"""
    return np.where(labels > 0, labels * 3 + 2, 0).astype(np.int32)


def remap_arguments(labels):
    """the three call forms of remap_labels for a volume with ids 1 .. m: {name: (locations, new_labels)}"""
    m = int(labels.max())
    ids = np.arange(1, m + 1)
    picked = ids[::2]
    return {"bool": (ids % 3 != 0, None),
            "int": (picked, (picked[::-1] + 3).astype(labels.dtype)),
            "new": (None, ((ids * 5) % 11).astype(labels.dtype))}


# ---- hand-built volumes -------------------------------------------------------------------------------------------------
def _edge_regions():
    """a 5 x 5 square (25 px) and a connected 27-px region sharing exactly 7 px with it, on a 12 x 9 frame"""
    square, region = np.zeros((12, 9), bool), np.zeros((12, 9), bool)
    square[0:5, 0:5] = True
    region[5:9, 0:5] = True
    region[4, 0:5] = True
    region[3, 0:2] = True
    assert square.sum() == 25 and region.sum() == 27 and (square & region).sum() == 7
    assert ndi.label(region)[1] == 1
    return square, region


def _zero_flows(shape):
    z = np.zeros(tuple(shape) + (2,), np.int8)
    return z, z.copy()


def make_edge_volume():
    square, region = _edge_regions()
    return np.stack([square, region])


def make_visit_order():
    """(3, 12, 20), six step labels.  Frame 0: B = 1, A = 2; frame 1: C = 3 (touches both), E = 4; frame 2: D = 5 (under C),
    F = 6.  All flows are zero except the forward flow on B's pixels, which samples frame 1 twelve pixels to the right,
    where nothing is: B has no forward neighbour, C has B and A as backward neighbours."""
    mask = np.zeros((3, 12, 20), bool)
    mask[0, 1:5, 1:5] = True          # B
    mask[0, 1:5, 8:12] = True         # A
    mask[1, 2:4, 2:11] = True         # C
    mask[1, 8:11, 14:18] = True       # E
    mask[2, 2:4, 5:9] = True          # D
    mask[2, 8:11, 1:4] = True         # F
    forward, backward = _zero_flows(mask.shape)
    forward[0, 1:5, 1:5, 0] = 12
    return mask, forward, backward


def make_gap_ids():
    """flat labels with ids {1, 2, 4, 7} on (2, 12, 9): 1 and 2 in frame 0, 4 and 7 in frame 1; 7 lies under 2, 4 under
    nothing.  The ids 3, 5 and 6 have no pixel: the reference lets each of them open a group and consume a number."""
    flat = np.zeros((2, 12, 9), np.int32)
    flat[0, 0:3, 0:3] = 1
    flat[0, 6:10, 2:8] = 2
    flat[1, 0:3, 5:9] = 4
    flat[1, 7:11, 3:7] = 7
    forward, backward = _zero_flows(flat.shape)
    return flat, forward, backward


GAP_GRID = ((0, 0), (0, 12))           # 2 and 7 share 12 px: linked, and not (the test is the strict >)


def flow_label_cases():
    """{name: (mask, forward, backward, grid of (overlap, absolute_overlap))}: every flow_label case of the fixture"""
    cases = {}
    for shape in SHAPES:
        for seed in SEEDS:
            cases[seeded_name(shape, seed)] = (seeded_mask(shape, seed),) + seeded_flows(shape, seed) + (FLOW_GRID,)
    edge = make_edge_volume()
    cases["product_edge"] = (edge,) + _zero_flows(edge.shape) + (((0.27, 0), (0.28, 0), (0.29, 0)),)
    cases["absolute_edge"] = (edge,) + _zero_flows(edge.shape) + (((0, 6), (0, 7)),)
    cases["visit_order"] = make_visit_order() + (((0, 0), (0.3, 2)),)
    cases["empty/2x7x130"] = (np.zeros((2, 7, 130), bool),) + seeded_flows((2, 7, 130), 1) + (((0, 0), (0.5, 4)),)
    cases["empty/1x1x1"] = (np.zeros((1, 1, 1), bool),) + _zero_flows((1, 1, 1)) + (((0, 0), (0.5, 4)),)
    cases["full/2x7x130"] = (np.ones((2, 7, 130), bool),) + seeded_flows((2, 7, 130), 1) + (((0, 0), (0.5, 4)),)
    return cases


SEEDED = tuple(seeded_name(shape, seed) for shape in SHAPES for seed in SEEDS)
FLAT_CASES = SEEDED + ("empty/2x7x130", "empty/1x1x1", "full/2x7x130")        # flat_label with both structures
OVERLAPPING_CASES = (seeded_name(UNALIGNED, 1), "product_edge")                # find_overlapping_labels, label by label


def overlapping_grid(name):
    return ((0.27, 0), (0.28, 0), (0.29, 0), (0, 6), (0, 7)) if name == "product_edge" else FLOW_GRID


def link_cases(steps):
    """{name: (flat labels, forward, backward, grid)}: every flow_link_overlap case.  The step-label inputs are
    make_step_labels(tile_labels(shape)) as the reference wrote them: `steps` maps a shape's name to that array."""
    cases = {}
    for shape in SHAPES:
        cases[f"steps/{shape_name(shape)}"] = (steps[shape_name(shape)].astype(np.int32),) + seeded_flows(shape, 1) + (LINK_GRID,)
    cases["gap_ids"] = make_gap_ids() + (GAP_GRID,)
    return cases


# ---- window cases ---------------------------------------------------------------------------------------------------------
def _blob_labels(shape, seed):
    return ndi.label(seeded_mask(shape, seed))[0].astype(np.int32)


def window_cases():
    """{name: (left, right, grid of (atol, rtol))}: int32 label volumes of the same frames"""
    cases = {}
    for shape in SHAPES:
        a = _blob_labels(shape, 0)
        cases[f"blobs/{shape_name(shape)}"] = (a, _blob_labels(shape, 1), WINDOW_GRID)
        b = np.roll(a, (1, 2), (1, 2))
        b[b > 0] = (b[b > 0] * 7) % 31 + 1
        cases[f"rolled/{shape_name(shape)}"] = (a, b, WINDOW_GRID)
    square, region = _edge_regions()
    cases["quotient_edge"] = ((square * 3).astype(np.int32)[None], (region * 2).astype(np.int32)[None], QUOTIENT_GRID)
    left, right = np.zeros((1, 12, 9), np.int32), np.zeros((1, 12, 9), np.int32)
    left[0, 0:3, 0:4] = 1             # 12 px, all of them over right == 0: they count towards n, the label links to nothing
    left[0, 6:10, 2:8] = 2
    right[0, 5:11, 1:9] = 1
    cases["over_zero"] = (left, right, WINDOW_GRID)
    left, right = np.zeros((1, 12, 20), np.int32), np.zeros((1, 12, 20), np.int32)
    right[0, 0:8, 0:10] = 1           # 80 px, 12 of them under the left label: count / size = 0.15 over ALL voxels
    left[0, 0:4, 7:17] = 1            # 40 px: count / n = 0.3
    cases["mostly_outside"] = (left, right, WINDOW_GRID)
    return cases


def padded_window(left, right):
    """The frames two consecutive windows share, as find_overlap_between_cores / _anvils see them: the compared frames with
    one more common frame before and after, which linking.py:55-56 drops.  The dropped frames are filled with each side's
    largest id, so that they would link that pair if they were counted."""
    fill = lambda v: np.full((1,) + v.shape[1:], max(int(v.max()), 0), np.int32)
    return np.concatenate([fill(left), left, fill(left)]), np.concatenate([fill(right), right, fill(right)])


def node_ids(x, y, n_left):
    """the graph find_new_labels is given: left ids as they are, right ids behind them (linking.py:182-199 offsets them by
    the running count in the same way)"""
    return np.asarray(x, np.int64), np.asarray(y, np.int64) + n_left


def canonical_partition(component_of):
    """component numbers replaced by the order of first appearance: equal for equal partitions"""
    _, first, inverse = np.unique(np.asarray(component_of), return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse.ravel()]


# ---- the tiny model of the grouping --------------------------------------------------------------------------------------------
def neighbour_lists(flat, forward, backward):
    """label -> (ascending forward neighbours, ascending backward neighbours) with overlap = absolute_overlap = 0"""
    back, fwd = warped_labels(flat, forward, backward)
    out = {}
    for label in range(1, int(flat.max()) + 1):
        at = flat == label
        out[label] = tuple(sorted(set(w[at].tolist()) - {0}) for w in (fwd, back))
    return out


def group_model(neighbours, order):
    """label -> group number.  order: "forward_first" (the reference), "backward_first", "depth_first" (forward first,
    a stack instead of a queue), "depth_backward_first", or "symmetric" (connected components of the undirected relation)."""
    n = len(neighbours)
    if order == "symmetric":
        parent = list(range(n + 1))

        def find(i):
            while parent[i] != i:
                i = parent[i]
            return i
        for a, (f, b) in neighbours.items():
            for m in list(f) + list(b):
                parent[max(find(a), find(m))] = min(find(a), find(m))
        roots = sorted({find(i) for i in range(1, n + 1)})
        return {i: roots.index(find(i)) + 1 for i in range(1, n + 1)}
    seen, group, n_groups = set(), {}, 0
    for root in range(1, n + 1):
        if root in seen:
            continue
        n_groups += 1
        todo = [root]
        seen.add(root)
        while todo:
            cur = todo.pop(-1 if order.startswith("depth") else 0)
            group[cur] = n_groups
            f, b = neighbours[cur]
            for m in (list(b) + list(f) if order.endswith("backward_first") else list(f) + list(b)):
                if m not in seen:
                    seen.add(m)
                    todo.append(m)
    return group


def check_visit_order():
    """the facts of the module docstring on `visit_order`; returns (the reference order's groups, the symmetric ones)"""
    mask, forward, backward = make_visit_order()
    flat = ndi.label(mask, structure=ndi.generate_binary_structure(3, 1) * np.array([0, 1, 0])[:, None, None])[0]
    nb = neighbour_lists(flat, forward, backward)
    assert len(nb) >= 5
    B, A, C = 1, 2, 3
    assert nb[A][0] == [C] and nb[C][1] == [B, A] and nb[B][0] == [] and B < A
    want = group_model(nb, "forward_first")
    for order in ("backward_first", "depth_first", "depth_backward_first"):
        assert group_model(nb, order) == want, order
    symmetric = group_model(nb, "symmetric")
    assert want[B] != want[A] == want[C] and symmetric[B] == symmetric[A] == symmetric[C] and symmetric != want
    return want, symmetric


check_visit_order()


# ---- the fixture -------------------------------------------------------------------------------------------------------------
# Volumes that the reference derives label by label from a finer labelling are stored as tables over the finer ids
# (lut_of; the generator checks that the table reproduces the reference's volume voxel for voxel): flat_label with the
# full structure over flat_label with the default one, flow_label over flat_label, flow_link_overlap over its input.
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(GOLDEN) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def expected_flat(name, structure="default"):
    flat = fixture()[f"flat/{name}"].astype(np.int32)
    return flat if structure == "default" else fixture()[f"flat_full/{name}"].astype(np.int32)[flat]


def expected_flow_label(name, grid):
    """{(overlap, absolute_overlap): int32 volume}"""
    flat, tables = expected_flat(name), fixture()[f"flow_label/{name}"].astype(np.int32)
    assert len(tables) == len(grid)
    return {g: table[flat] for g, table in zip(grid, tables)}


def expected_link(name, flat, grid):
    """{(overlap, absolute_overlap): (int32 volume, number of groups the reference opened)}"""
    tables, groups = fixture()[f"link/{name}"].astype(np.int32), fixture()[f"link_groups/{name}"]
    assert len(tables) == len(groups) == len(grid)
    return {g: (table[flat], int(n)) for g, table, n in zip(grid, tables, groups)}


def expected_overlapping(name, grid):
    """{(overlap, absolute_overlap): rows (direction 0 forward / 1 backward, label, neighbour)}"""
    rows = fixture()[f"overlapping/{name}"].astype(np.int64).reshape(-1, 4)
    return {g: rows[rows[:, 0] == i, 1:] for i, g in enumerate(grid)}


def expected_window(name, grid):
    """{(atol, rtol): (pairs (k, 2) int64, component of every node of node_ids' graph)}"""
    rows = fixture()[f"window/{name}/pairs"].astype(np.int64).reshape(-1, 3)
    components = fixture()[f"window/{name}/components"]
    assert len(components) == len(grid)
    return {g: (rows[rows[:, 0] == i, 1:], components[i].astype(np.int64)) for i, g in enumerate(grid)}


def ragged(store, key):
    """a list of arrays / None stored as values + offsets + a none flag per entry"""
    values, offsets, none = store[key + "/values"], store[key + "/offsets"], store[key + "/none"]
    return [None if none[i] else values[offsets[i]:offsets[i + 1]] for i in range(len(none))]
