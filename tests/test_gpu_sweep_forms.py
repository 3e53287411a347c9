"""Every form of the flood's sweep kernels behind one small flood each: phase A without M1 and the M1 pass after it, the
chain levels 1..3 and the root phase as compile-time forms (connectivity 1), the run-time-k fallback of deeper chains, the
any-neighbour-count forms, and the overflow of the LDS staging buffers into the global queue.  Labels are compared voxel
by voxel with the C twin of the reference's kernel: raster order of equal-valued markers (on_ambiguous="ignore") against
its idealised order (tie_mode 1), reference order against the reference's own semantics (tie_mode 0)."""
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

T, H, W = 6, 40, 48
Y_WALL, X_WALL, XC = 29, 47, 23          # the staircase: rows 30..39, columns 0..46, centre column 23


def _quantised_volume():
    """6 x 40 x 48, four field values, integer flows in [-2, 2], twelve markers.

    Rows 0..28: a smooth random field quantised to four values with ten marker patches, five of them on the lowest value
    (equal-valued markers of different labels), random flows.
    Rows 30..39, walled off by the mask (row 29, column 47): a staircase 0 0 .. 1 1 .. 2 2 .. 3 3 3 .. 2 2 .. 0 0, the same
    in every row and frame, zero flow, markers 101 / 102 of equal value on its two ends.  Both fronts reach the centre
    column with chains that agree on every level: K2, then the keys of the three pushers one level down each, then the
    marker's 0 -- complete at depth 5.  A flood begun at depth 3 (or 1) has to deepen, past the compile-time levels."""
    rng = np.random.default_rng(20241)
    smooth = ndi.gaussian_filter(rng.normal(size=(T, H, W)), (0.5, 3, 3))
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-9)
    field = np.minimum(np.floor(smooth * 4), 3).astype(np.float32)
    markers = np.zeros((T, H, W), np.int32)
    for k in range(10):
        t, y, x = int(rng.integers(0, T)), int(rng.integers(0, Y_WALL - 3)), int(rng.integers(0, W - 3))
        markers[t, y:y + 2, x:x + 3] = k + 1
        if k % 2 == 0:
            field[t, y:y + 2, x:x + 3] = 0.0
    fwd = rng.integers(-2, 3, size=(T, H, W, 2)).astype(np.float32)
    bwd = rng.integers(-2, 3, size=(T, H, W, 2)).astype(np.float32)
    fwd[:, Y_WALL - 1:] = 0
    bwd[:, Y_WALL - 1:] = 0                                        # nothing is displaced across the wall
    mask = np.ones((T, H, W), bool)
    mask[:, Y_WALL, :] = False
    mask[:, Y_WALL:, X_WALL] = False
    stair = 3 - np.minimum(3, np.abs(np.arange(X_WALL) - XC) // 6)
    field[:, Y_WALL + 1:, :X_WALL] = stair[None, None, :].astype(np.float32)
    markers[:, Y_WALL + 1:, 0] = 101
    markers[:, Y_WALL + 1:, X_WALL - 1] = 102
    assert len(np.unique(field)) == 4 and len(np.unique(markers[markers != 0])) == 12
    return fwd, bwd, field, markers, mask


@pytest.fixture(scope="module")
def quantised():
    from oracle import ws_oracle
    fwd, bwd, field, markers, mask = _quantised_volume()
    want = {"ignore": ws_oracle.watershed(fwd, bwd, field, markers, mask, 1, tie_mode=1),
            "reference": ws_oracle.watershed(fwd, bwd, field, markers, mask, 1, tie_mode=0)}
    for w in want.values():
        w.setflags(write=False)
    return (fwd, bwd, field, markers, mask), want


def _flood(case, conn, mode, chain_depth=None):
    import torch
    from tobac_flow_amd import _lib
    from tobac_flow_amd.watershed import neighbour_offsets, watershed_dev
    fwd, bwd, field, markers, mask = case
    st = {}
    kw = {} if chain_depth is None else {"chain_depth": chain_depth}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore" if mode == "ignore" else "error")
        lab = watershed_dev(_lib.to_dev(fwd, torch.float32), _lib.to_dev(bwd, torch.float32), _lib.to_dev(field, torch.float32),
                            _lib.to_dev(markers, torch.int32), None if mask is None else _lib.to_dev(mask.astype(np.int8), torch.int8),
                            neighbour_offsets(conn), stats=st, on_ambiguous=mode, **kw)
    return lab.cpu().numpy(), st


@pytest.mark.parametrize("mode", ["ignore", "reference"])
def test_quantised_volume_through_the_compile_time_levels(quantised, mode):
    """begun at the default depth 3: phase A, the M1 pass, the speculative root phase (K = 1), chain levels 1 and 2, the
    root phase at K = 3, then the deepening to 5 on the run-time forms"""
    case, want = quantised
    got, st = _flood(case, 1, mode)
    print(mode, "sweeps", st["sweeps"], "depth", st["chain_depth"], "ambiguous", st["ambiguous_pixels"], "tie origins", st["marker_tie_origins"])
    assert st["chain_depth"] >= 5, "the staircase did not force the chain past the compile-time levels"
    if mode == "ignore":
        assert st["ambiguous_pixels"] >= T * (H - Y_WALL - 1)             # the staircase's centre column at the least
    assert np.array_equal(got, want[mode]), f"{int((got != want[mode]).sum())} px differ from the reference kernel"


@pytest.mark.parametrize("mode", ["ignore", "reference"])
def test_quantised_volume_begun_at_depth_one(quantised, mode):
    """chain_depth=1: the job deepens 1 -> 3, gives up, and the flood starts again at 4 with room for twelve levels -- chain
    level 4 and the root phase at 5 run on the run-time-k forms from the start"""
    case, want = quantised
    got, st = _flood(case, 1, mode, chain_depth=1)
    print(mode, "sweeps", st["sweeps"], "depth", st["chain_depth"])
    assert st["chain_depth"] >= 5
    assert np.array_equal(got, want[mode]), f"{int((got != want[mode]).sum())} px differ from the reference kernel"


def _plateau(shape, conn):
    """one value everywhere, two markers: the whole front is lowered at once, generation by generation, on the any-count
    forms (connectivity 3) and on the connectivity-1 forms.  256 queue entries x 26 edges could fill a staging buffer, but
    equal candidates collapse in the atomic minimum and only strict lowerings are staged: whether a buffer really
    overflows here is not guaranteed.  _scatter_volume below is the case in which it provably does."""
    t, h, w = shape
    field = np.full(shape, 2.5, np.float32)
    markers = np.zeros(shape, np.int32)
    markers[0, h // 4, w // 4] = 1
    markers[t - 1, (3 * h) // 4, (2 * w) // 3] = 2
    z = np.zeros(shape + (2,), np.float32)
    return (z, z, field, markers, None), conn


@pytest.mark.parametrize("mode", ["ignore", "reference"])
@pytest.mark.parametrize("shape,conn", [((4, 64, 64), 3), ((4, 96, 96), 1)])
def test_single_valued_plateau_overflows_the_staging_buffers(shape, conn, mode):
    from oracle import ws_oracle
    case, conn = _plateau(shape, conn)
    want = ws_oracle.watershed(*case, conn, tie_mode=1 if mode == "ignore" else 0)
    got, st = _flood(case, conn, mode)
    print(shape, conn, mode, "sweeps", st["sweeps"], "depth", st["chain_depth"], "ambiguous", st["ambiguous_pixels"])
    assert np.array_equal(got, want), f"{int((got != want).sum())} px differ from the reference kernel"


def _walled_plateau():
    """3 x 24 x 40, one field value, zero flow, two single-voxel markers of different labels; a box of floodable voxels
    (rows 14..19, columns 26..35, every frame) is cut off from both by a ring the mask takes out: nothing reaches it"""
    shape = (3, 24, 40)
    field = np.full(shape, 1.0, np.float32)
    markers = np.zeros(shape, np.int32)
    markers[0, 5, 7] = 1
    markers[2, 9, 31] = 2
    mask = np.ones(shape, bool)
    mask[:, 13:21, 25:37] = False
    mask[:, 14:20, 26:36] = True
    box = np.zeros(shape, bool)
    box[:, 14:20, 26:36] = True
    z = np.zeros(shape + (2,), np.float32)
    return (z, z, field, markers, mask), box


def test_unreached_voxels_and_the_tie_counts_from_the_oracle():
    """Floodable voxels no front reaches offer nothing to the M1 pass and keep M1 = infinity themselves: they stay 0, and
    the candidate edges of every other voxel are what they were.  The two counts the benchmark reports are derived from
    the oracle's labels.  On a one-valued field with zero flow a voxel's chain is (value, distance) and then the marker's:
    every in-neighbour one step nearer is a fully matching candidate, so a voxel's label set is the union of theirs.
      pixels_depending_on_equal_valued_marker_order (ambiguous_pixels): the voxels whose set holds both labels.  Such a
        voxel takes the label of the marker pushed first, so it is exactly a voxel whose oracle label changes when the
        push order of the two markers is reversed -- the oracle run on the volume mirrored in all three axes.
      marker_tie_points (marker_tie_origins): the voxels where the two sets meet, i.e. those of them with an in-neighbour
        one step nearer that is not among them."""
    from oracle import ws_oracle
    case, box = _walled_plateau()
    fwd, bwd, field, markers, mask = case
    want = ws_oracle.watershed(fwd, bwd, field, markers, mask, 1, tie_mode=1)
    flip = lambda a: np.ascontiguousarray(a[::-1, ::-1, ::-1])
    mirrored = flip(ws_oracle.watershed(fwd, bwd, flip(field), flip(markers), flip(mask), 1, tie_mode=1))
    depends = want != mirrored
    assert depends.any() and not depends[box].any() and not want[box].any()
    # geodesic distance from the markers through the floodable voxels, face neighbours
    reached = markers != 0
    dist = np.where(reached, 0, -1)
    s = ndi.generate_binary_structure(3, 1)
    d = 0
    while True:
        grown = ndi.binary_dilation(reached, structure=s) & mask & ~reached
        if not grown.any():
            break
        d += 1
        dist[grown] = d
        reached |= grown
    assert np.array_equal(reached, want != 0)
    origin = np.zeros_like(depends)
    for axis in range(3):
        for step in (1, -1):
            nearer = np.roll(dist, step, axis) == dist - 1
            clean = ~np.roll(depends, step, axis)
            edge = np.ones_like(depends)
            idx = [slice(None)] * 3
            idx[axis] = 0 if step == 1 else -1
            edge[tuple(idx)] = False                               # np.roll wraps: no neighbour across the border
            origin |= depends & nearer & clean & edge & (dist > 0)
    got, st = _flood(case, 1, "ignore")
    print("ambiguous", st["ambiguous_pixels"], "expected", int(depends.sum()), "tie origins", st["marker_tie_origins"], "expected", int(origin.sum()))
    assert np.array_equal(got, want), f"{int((got != want).sum())} px differ from the oracle"
    assert not got[box].any()
    assert st["ambiguous_pixels"] == int(depends.sum())
    assert st["marker_tie_origins"] == int(origin.sum())
    ref, _ = _flood(case, 1, "reference")
    want0 = ws_oracle.watershed(fwd, bwd, field, markers, mask, 1, tie_mode=0)
    assert np.array_equal(ref, want0), f"{int((ref != want0).sum())} px differ from the reference kernel"


def _scatter_volume():
    """5 x 52 x 52, one field value.  Frame 2 carries a 16 x 16 block of markers (labels 1..256) that is exactly one tile of
    the compact numbering, so the 256 markers are consecutive ids and ONE workgroup takes them in one trip of the first sweep.
    Marker (y, x) has the flow (2x + 1, 2y + 1) forwards and backwards: its neighbours in frames 1 and 3 lie around
    (3y + 1, 3x + 1), three pixels apart from those of the next marker, so no two markers share a neighbour there.
    Every lowering below is of a distinct pixel from infinity, i.e. one staged append each, between two flushes:
      connectivity 3: the trip itself lowers 256 x 9 pixels in frame 3 and as many in frame 1 = 4 608 appends;
      connectivity 1: the trip lowers the 512 centres; the first local round then relaxes those 512, each its four
        in-plane neighbours and its neighbour one frame further on (zero flow there) = 2 560 appends at the least.
    Both exceed a staging buffer of 2 048 entries (the first also one of 4 096): ws_stage's spill to the global queue runs."""
    shape = (5, 52, 52)
    field = np.full(shape, 1.0, np.float32)
    markers = np.zeros(shape, np.int32)
    markers[2, :16, :16] = np.arange(1, 257, dtype=np.int32).reshape(16, 16)
    fwd = np.zeros(shape + (2,), np.float32)
    yy, xx = np.mgrid[:16, :16]
    fwd[2, :16, :16, 0] = 2 * xx + 1
    fwd[2, :16, :16, 1] = 2 * yy + 1
    return fwd, fwd.copy(), field, markers, None


@pytest.mark.parametrize("mode", ["ignore", "reference"])
@pytest.mark.parametrize("conn", [1, 3])
def test_a_front_provably_wider_than_the_staging_buffer(conn, mode):
    from oracle import ws_oracle
    case = _scatter_volume()
    want = ws_oracle.watershed(*case, conn, tie_mode=1 if mode == "ignore" else 0)
    # the construction: the markers' neighbours one frame on are pairwise distinct and all floodable
    near = want[3] != 0
    assert int(near.sum()) == 52 * 52 and len(np.unique(want[3][1:48:3, 1:48:3])) == 256
    got, st = _flood(case, conn, mode)
    print(conn, mode, "sweeps", st["sweeps"], "depth", st["chain_depth"], "ambiguous", st["ambiguous_pixels"])
    assert np.array_equal(got, want), f"{int((got != want).sum())} px differ from the reference kernel"
