"""The scipy.ndimage glue (tobac_flow_amd/csrc/morph.hip) on every path its dispatch can take.

Every comparison is `array_equal` (with `equal_nan` for floats) against SciPy, a host function of tobac_flow_amd.utils /
analysis or plain numpy -- never against the library and never with a tolerance.  The inputs come from
tests/glue_cases.py; tests/test_glue_cases_cpu.py checks without a GPU that they reach the rules and kernel forms they
are named for (DESIGN.md "Dispatch of the ndimage glue" lists which test reaches which kernel).

Tests that go through the C ABI place every operand inside a larger device buffer filled with a sentinel byte: inputs
and outputs can so be moved off their natural alignment (which selects the scalar / byte / word fallbacks), and the
bytes on both sides of every output must be unchanged afterwards.
"""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndi

import glue_cases as gl

pytestmark = pytest.mark.gpu

SENT = 0xA5                           # sentinel byte of the guard zones (and of outputs before a call)
PAD = 64                              # guard bytes on each side of an operand


@pytest.fixture(scope="module")
def L():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib.lib()


@pytest.fixture(scope="module")
def nd():
    from tobac_flow_amd import ndimage_dev
    return ndimage_dev


class Guarded:
    """`count` elements of `dtype` inside a sentinel-filled byte buffer, `off` ELEMENTS past a 16-byte boundary"""

    def __init__(self, count, dtype, off=0, data=None):
        import torch
        self.dtype = np.dtype(dtype)
        self.nbytes = int(count) * self.dtype.itemsize
        self.raw = torch.full((2 * PAD + 16 + off * self.dtype.itemsize + self.nbytes,), SENT, dtype=torch.uint8, device="cuda")
        self.start = PAD + (-(self.raw.data_ptr() + PAD)) % 16 + off * self.dtype.itemsize
        assert (self.raw.data_ptr() + self.start) % 16 == (off * self.dtype.itemsize) % 16
        if data is not None:
            data = np.ascontiguousarray(data, self.dtype)
            assert data.size == count
            self.raw[self.start:self.start + self.nbytes] = torch.from_numpy(data.reshape(-1).view(np.uint8).copy()).cuda()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + self.start)

    def host(self, shape=None):
        """the content; asserts that the guard bytes on both sides still hold the sentinel"""
        raw = self.raw.cpu().numpy()
        assert (raw[:self.start] == SENT).all(), "bytes BEFORE the buffer were overwritten"
        assert (raw[self.start + self.nbytes:] == SENT).all(), "bytes AFTER the buffer were overwritten"
        out = raw[self.start:self.start + self.nbytes].copy().view(self.dtype)
        return out if shape is None else out.reshape(shape)

    def untouched(self):
        return bool((self.raw.cpu().numpy() == SENT).all())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _st(structure):
    return np.ascontiguousarray(np.asarray(structure) != 0, np.uint8)


def _stream():
    from tobac_flow_amd import _lib
    return _lib.stream_ptr()


def _sync():
    import torch
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- tf_label
def test_label_all_8192_symmetric_structures(nd):
    """Every centro-symmetric structure on one 2 x 5 x 70 volume (one segment boundary per row): both k_ccl_union
    instantiations, the centre-only structure without any union kernel, every subset of sibling bits."""
    import torch
    rng = np.random.default_rng(5)
    mask = rng.random((2, 5, 70)) < 0.55
    md = torch.from_numpy(mask).cuda()
    bad = []
    for k, st in enumerate(gl.symmetric_structures()):
        want, n = ndi.label(mask, structure=st)
        got, ng = nd.label(md, st)
        if ng != n or not np.array_equal(got.cpu().numpy(), want):
            bad.append(k)
    assert not bad, f"{len(bad)} of 8192 structures differ from scipy.ndimage.label, first: {bad[:20]}"


@pytest.mark.parametrize("case", gl.label_masks(), ids=lambda c: c["name"])
def test_label_named_structures_on_named_masks(nd, case):
    import torch
    named = gl.named_structures()
    for sname, must in case["claims"]:                                  # the case reaches the rules it is there for
        counts = gl.ccl_model(case["mask"], named[sname])[2]
        assert all(counts[c] > 0 for c in must), (case["name"], sname, counts)
    mask = case["mask"]
    md = torch.from_numpy(mask).cuda()
    for sname, st in named.items():
        want, n = ndi.label(mask, structure=st)
        got, ng = nd.label(md, st)
        got = got.cpu().numpy()
        assert ng == n, f"{case['name']} under {sname}: {ng} labels, SciPy finds {n}"
        assert np.array_equal(got, want), f"{case['name']} under {sname}: {int((got != want).sum())} voxels differ"


def _label_abi(L, mask, st, in_off, out_off, short=0):
    import torch
    T, H, W = mask.shape
    m = Guarded(mask.size, np.uint8, in_off, mask)
    out = Guarded(mask.size, np.int32, out_off)
    need = L.tf_label_workspace_bytes(T, H, W)
    ws = torch.empty(need - short, dtype=torch.uint8, device="cuda")
    n = ctypes.c_int(-7)
    rc = L.tf_label(m.ptr, T, H, W, _p(_st(st)), out.ptr, ctypes.byref(n), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _sync()
    return rc, n.value, out


@pytest.mark.parametrize("shape", [(2, 5, 70), (1, 3, 85), (3, 5, 17), (1, 1, 257), (2, 4, 64)], ids=lambda s: "x".join(map(str, s)))
def test_label_through_the_c_abi_with_any_mask_byte_and_any_alignment(L, shape):
    """Mask bytes from {0, 1, 2, 0x80, 255}; the mask 1 byte and the labels 4 bytes off their alignment: k_ccl_init
    instead of k_ccl_init4 (structures without the x tap) and k_ccl_number instead of k_ccl_number4; n % 4 != 0 runs the
    scalar tails of the *4 forms."""
    rng = np.random.default_rng(sum(shape))
    named = gl.named_structures()
    mask = rng.choice(np.array([0, 0, 0, 1, 2, 0x80, 255], np.uint8), shape)
    random_x = next(k for k in named if k.startswith("random_x_"))
    random_no_x = next(k for k in named if k.startswith("random_") and not k.startswith("random_x_"))
    for sname in ("conn1", "conn3", "cube_minus_x", "y_only", "centre_only", "x_diag_yx", random_x, random_no_x):
        st = named[sname]
        want, n = ndi.label(mask != 0, structure=st)
        for in_off in (0, 1):
            for out_off in (0, 1):
                rc, ng, out = _label_abi(L, mask, st, in_off, out_off)
                got = out.host(shape)
                assert rc == 0 and ng == n, (sname, in_off, out_off, rc, ng, n)
                assert np.array_equal(got, want), f"{sname} in+{in_off} out+{4 * out_off}: {int((got != want).sum())} voxels differ"


def test_label_count_when_the_last_block_holds_no_root_and_short_workspace(L):
    cases = {c["name"]: c["mask"] for c in gl.label_masks()}
    named = gl.named_structures()
    tail = cases["checker_rootless_tail"].astype(np.uint8)
    assert not tail.reshape(-1)[-(tail.size % 256) - 256:].any()
    for sname in ("conn1", "cube_minus_x", "centre_only"):
        want, n = ndi.label(tail, structure=named[sname])
        rc, ng, out = _label_abi(L, tail, named[sname], 0, 0)
        assert rc == 0 and ng == n and np.array_equal(out.host(tail.shape), want), sname
    # a workspace one byte short: TF_ENOMEM, nothing written
    rc, ng, out = _label_abi(L, tail, named["conn1"], 0, 0, short=1)
    assert rc == -2 and b"workspace" in L.tf_last_error() and out.untouched() and ng == -7
    asym = np.zeros((3, 3, 3), np.uint8)
    asym[1, 1, 1] = asym[1, 1, 2] = 1
    rc, ng, out = _label_abi(L, tail, asym, 0, 0)
    assert rc == -1 and out.untouched()


# ----------------------------------------------------------------------------- tf_binary_morph
def _morph_mask(rng, shape):
    """blobs with holes and salt noise: neither operation empties or fills it within four iterations"""
    x = ndi.gaussian_filter(rng.normal(size=shape), (0.5, 1.5, 2.5)) > 0.0
    return np.ascontiguousarray(x ^ (rng.random(shape) < 0.04))


@pytest.mark.parametrize("geometry", gl.MORPH_GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_binary_morphology_every_geometry_structure_border_and_iteration_count(nd, geometry):
    """ndi.binary_erosion / binary_dilation for every structure of glue_cases.morph_structures(), border 0 / 1 and 1 - 4
    iterations (the ping-pong between `out` and `tmp` ends in `out` for even and for odd counts)."""
    import torch
    rng = np.random.default_rng(sum(geometry))
    x = _morph_mask(rng, geometry)
    xd = torch.from_numpy(x).cuda()
    bad = []
    for sname, st in gl.morph_structures().items():
        for border in (0, 1):
            for it in (1, 2, 3, 4):
                got = nd.binary_erosion(xd, st, it, border).cpu().numpy()
                if not np.array_equal(got, ndi.binary_erosion(x, structure=st, iterations=it, border_value=border)):
                    bad.append((sname, "erosion", border, it))
                got = nd.binary_dilation(xd, st, it, border).cpu().numpy()
                if not np.array_equal(got, ndi.binary_dilation(x, structure=st, iterations=it, border_value=border)):
                    bad.append((sname, "dilation", border, it))
    assert not bad, f"{gl.morph_form(*geometry)}: {len(bad)} combinations differ from SciPy, first: {bad[:12]}"


# (in, out, tmp) offsets in bytes, iterations; the form tf_binary_morph must fall back to at W = 1040
MORPH_ALIGNMENTS = [((0, 0, 0), 3, "uint4"), ((0, 0, 0), 2, "uint4"), ((0, 0, None), 1, "uint4"),
                    ((4, 4, 4), 2, "word"), ((4, 4, 4), 3, "word"), ((0, 0, 4), 2, "word"), ((4, 0, None), 1, "word"),
                    ((0, 20, 0), 4, "word"), ((1, 1, 1), 3, "byte"), ((0, 1, 0), 2, "byte"), ((0, 0, 3), 4, "byte"),
                    ((2, 0, None), 1, "byte")]


@pytest.mark.parametrize("offsets,iterations,form", MORPH_ALIGNMENTS,
                         ids=[f"{f}-in{o[0]}-out{o[1]}-tmp{o[2]}-it{i}" for o, i, f in MORPH_ALIGNMENTS])
def test_binary_morphology_through_the_c_abi_alignment_fallbacks_and_any_byte(L, offsets, iterations, form):
    """A width that takes the uint4 form when aligned (1040), with `in` / `out` / `tmp` moved 4 bytes (word form) or 1 - 3
    bytes (byte form) off; input bytes from {0, 1, 2, 0x40, 0x80, 255} (the ABI takes any non-zero byte as set); every
    output byte is 0 or 1 and the guard bytes around `out` and `tmp` survive."""
    T, H, W = 2, 9, 1040
    offs = [o for o in offsets if o is not None]
    assert gl.morph_form(T, H, W, 0 if all(o % 16 == 0 for o in offs) else 4 if all(o % 4 == 0 for o in offs) else 1)[0] == form
    rng = np.random.default_rng(iterations + sum(o or 0 for o in offsets))
    x = _morph_mask(rng, (T, H, W))
    raw = (x * rng.choice(np.array([1, 2, 0x40, 0x80, 255], np.uint8), x.shape)).astype(np.uint8)
    structures = gl.morph_structures()
    for sname in ("cube", "skew", "row5", "rows5", "no_centre", "tap_x-", "random03", "random17"):
        st = structures[sname]
        for op, ref in ((0, ndi.binary_erosion), (1, ndi.binary_dilation)):
            for border in (0, 1):
                src = Guarded(raw.size, np.uint8, offsets[0], raw)
                out = Guarded(raw.size, np.uint8, offsets[1])
                tmp = Guarded(raw.size, np.uint8, offsets[2]) if offsets[2] is not None else None
                rc = L.tf_binary_morph(src.ptr, T, H, W, _p(_st(st)), op, iterations, border, out.ptr,
                                       tmp.ptr if tmp else None, _stream())
                _sync()
                assert rc == 0, L.tf_last_error()
                got = out.host((T, H, W))
                if tmp is not None:
                    tmp.host()                                          # (its guards)
                assert np.array_equal(src.host((T, H, W)), raw)         # the input is not written
                assert got.max() <= 1, f"{sname}: output bytes other than 0 / 1"
                want = ref(x, structure=st, iterations=iterations, border_value=border)
                assert np.array_equal(got.astype(bool), want), f"{sname} op {op} border {border}: {int((got != want).sum())} px differ"


def test_binary_morphology_rejects_bad_arguments_without_writing(L):
    x = np.ones((2, 3, 16), np.uint8)
    src, out = Guarded(x.size, np.uint8, 0, x), Guarded(x.size, np.uint8)
    st = _st(np.ones((3, 3, 3)))
    call = lambda s, op, it, tmp: L.tf_binary_morph(src.ptr, 2, 3, 16, _p(s), op, it, 0, out.ptr, tmp, _stream())     # noqa: E731
    assert call(np.zeros(27, np.uint8), 0, 1, None) == -1               # empty structure
    assert call(st, 2, 1, None) == -1 and call(st, 0, 0, None) == -1    # bad op, no iterations
    assert call(st, 0, 2, None) == -1                                   # two iterations need a tmp buffer
    _sync()
    assert out.untouched()


# ----------------------------------------------------------------------------- the elementwise kernels
def _seeds(n, seed, lower, upper):
    """the short vectors hold few values: with them every special value takes its turn, in the tail of the *4 kernels too"""
    return range(gl.special_values(lower, upper).size) if n <= 7 else (seed,)


def _offsets(n_operands):
    """all aligned, then each operand alone one element off"""
    return [tuple(int(i == k) for i in range(n_operands)) for k in range(-1, n_operands)]


@pytest.mark.parametrize("n", gl.ELEMENT_COUNTS)
def test_linearise_every_count_alignment_and_special_value(L, n):
    from tobac_flow_amd.utils import linearise_field
    for pi, (lo, hi) in enumerate(gl.THRESHOLD_PAIRS):
        for oi, (f_off, o_off) in enumerate(_offsets(2)):
            for seed in _seeds(n, 3 * pi + oi, lo, hi):
                v = gl.element_vector(n, lo, hi, seed)
                with np.errstate(all="ignore"):
                    want = linearise_field(v, lo, hi)
                assert want.dtype == np.float32
                src, out = Guarded(n, np.float32, f_off, v), Guarded(n, np.float32, o_off)
                assert L.tf_linearise(src.ptr, n, lo, hi, out.ptr, _stream()) == 0
                got = out.host()
                diff = [(float(a), float(b), float(c)) for a, b, c in zip(v, got, want) if not (b == c or (b != b and c != c))]
                assert np.array_equal(got, want, equal_nan=True), f"({lo}, {hi}) offsets {f_off, o_off}: (x, got, want) {diff[:6]}"


@pytest.mark.parametrize("n", gl.ELEMENT_COUNTS)
def test_field_masks_every_count_alignment_and_special_value(L, n):
    for oi, offs in enumerate(_offsets(4)):
        for seed in _seeds(n, oi, 0.0, 1.0):
            v = gl.element_vector(n, 0.0, 1.0, seed)
            src = Guarded(n, np.float32, offs[0], v)
            outs = [Guarded(n, np.uint8, o) for o in offs[1:]]
            assert L.tf_field_masks(src.ptr, n, outs[0].ptr, outs[1].ptr, outs[2].ptr, _stream()) == 0
            with np.errstate(all="ignore"):
                wants = (v >= 1, (v <= 0) | np.isnan(v), np.isnan(v))
            for name, o, want in zip(("ge1", "le0_or_nan", "isnan"), outs, wants):
                got = o.host()
                assert got.max() <= 1 and np.array_equal(got.astype(bool), want), f"{name}, offsets {offs}, values {v[:8]}"


@pytest.mark.parametrize("n", gl.ELEMENT_COUNTS)
def test_merge_seeds_every_count_and_alignment(L, n):
    rng = np.random.default_rng(n)
    for offs in _offsets(4):
        for last_bg, last_isn in ((None, None), (2, 0), (0, 255), (0, 0)):      # the last element (the tail's) in every state
            comp = rng.integers(-3, 1000, n).astype(np.int32)
            bg = rng.choice(np.array([0, 0, 0, 1, 2, 0x80], np.uint8), n)
            isn = rng.choice(np.array([0, 0, 0, 0, 1, 255], np.uint8), n)
            if last_bg is not None:
                bg[-1], isn[-1] = last_bg, last_isn
            c, b, i = Guarded(n, np.int32, offs[0], comp), Guarded(n, np.uint8, offs[1], bg), Guarded(n, np.uint8, offs[2], isn)
            out = Guarded(n, np.int32, offs[3])
            assert L.tf_merge_seeds(c.ptr, b.ptr, i.ptr, n, out.ptr, _stream()) == 0
            want = np.where((bg != 0) | (isn != 0), np.int32(-1), comp)
            assert np.array_equal(out.host(), want), f"offsets {offs}, last ({last_bg}, {last_isn})"


@pytest.mark.parametrize("n", gl.ELEMENT_COUNTS)
def test_apply_lut_both_forms_every_count_and_alignment(L, n):
    """tf_apply_lut and tf_apply_lut_keep_nonpositive: labels above n_lut (-> 0), negative labels (-> 0 / kept), label 0."""
    rng = np.random.default_rng(n + 1)
    for n_lut in (1, 7, 300):
        lut = rng.integers(1, 10 ** 6, n_lut).astype(np.int32)
        lut[0] = 5                                                     # tf_apply_lut reads lut[0] for label 0; `keep` never does
        for offs in _offsets(3):
            lab = rng.integers(-4, n_lut + 4, n).astype(np.int32)
            lab[rng.random(n) < 0.1] = np.iinfo(np.int32).max
            lab[rng.random(n) < 0.1] = np.iinfo(np.int32).min
            inside = (lab >= 0) & (lab < n_lut)
            gathered = lut[np.where(inside, lab, 0)]
            src, table = Guarded(n, np.int32, offs[0], lab), Guarded(n_lut, np.int32, offs[1], lut)
            out = Guarded(n, np.int32, offs[2])
            assert L.tf_apply_lut(src.ptr, n, table.ptr, n_lut, out.ptr, _stream()) == 0
            assert np.array_equal(out.host(), np.where(inside, gathered, 0)), f"tf_apply_lut n_lut {n_lut} offsets {offs}"
            out = Guarded(n, np.int32, offs[2])
            assert L.tf_apply_lut_keep_nonpositive(src.ptr, n, table.ptr, n_lut, out.ptr, _stream()) == 0
            want = np.where(lab <= 0, lab, np.where(inside, gathered, 0))
            assert np.array_equal(out.host(), want), f"tf_apply_lut_keep_nonpositive n_lut {n_lut} offsets {offs}"


def test_remap_labels_equals_the_host_function(nd):
    import torch
    from tobac_flow_amd.utils import remap_labels
    rng = np.random.default_rng(9)
    for shape in ((1, 1, 5), (2, 3, 7), (3, 5, 17), (2, 8, 64)):
        lab = rng.integers(0, 40, shape).astype(np.int32)
        lab.flat[0] = 39
        keep = rng.random(39) < 0.5
        assert np.array_equal(nd.remap_labels(torch.from_numpy(lab).cuda(), keep).cpu().numpy(), remap_labels(lab, keep))


# ----------------------------------------------------------------------------- tf_label_filter with zero or one TF_U8 criterion
@pytest.mark.parametrize("shape", [(1, 7, 9), (4, 5, 13), (6, 1, 33), (3, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_label_filter_ignores_foreign_labels_and_sees_the_last_frame(L, shape):
    """Labels above n_labels and negative labels are ignored; no criterion leaves the hit bits zero; T = 1; a label that
    occurs in the last frame only.  The records {tmin, tmax, hits, 0} have n_labels + 1 entries, guarded on both sides."""
    from tobac_flow_amd import _lib
    T, H, W = shape
    rng = np.random.default_rng(sum(shape))
    n_labels = 9
    lab = rng.integers(-2, n_labels + 4, shape).astype(np.int32)
    lab[lab == 7] = 0
    lab[T - 1, H - 1, W - 1] = 7                                        # label 7: one voxel, the last of the volume
    lab[lab == 4] = 0                                                   # label 4: absent
    mask = (rng.random(shape) < 0.15).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), shape)
    for with_mask in (True, False):
        src = Guarded(lab.size, np.int32, 0, lab)
        m = Guarded(lab.size, np.uint8, 1, mask)
        rec = Guarded(4 * (n_labels + 1), np.int32)
        crit = (_lib.LabelCriterion * 1)(_lib.LabelCriterion(m.ptr.value, _lib.TF_U8, 0, 0.0))
        assert L.tf_label_filter(src.ptr, T, H, W, n_labels, crit, int(with_mask), rec.ptr, _stream()) == 0
        want = np.tile(np.array([0x7fffffff, -1, 0, 0], np.int32), (n_labels + 1, 1))
        for l in range(1, n_labels + 1):
            frames = np.nonzero((lab == l).any((1, 2)))[0]
            if frames.size:
                want[l, 0], want[l, 1] = frames[0], frames[-1]
            want[l, 2] = with_mask and bool(((lab == l) & (mask != 0)).any())      # hit = bit 0
        assert np.array_equal(rec.host((n_labels + 1, 4)), want)
        assert want[7, 1] == T - 1 == want[7, 0] and want[4, 1] == -1 and (with_mask or not want[:, 2].any())


def test_label_filter_wrapper_equals_the_host_functions(nd):
    import torch
    from tobac_flow_amd.analysis import find_object_lengths, mask_labels
    rng = np.random.default_rng(21)
    for shape in ((1, 9, 11), (5, 6, 7)):
        lab = ndi.label(rng.random(shape) < 0.4)[0].astype(np.int32)
        msk = rng.random(shape) < 0.1
        lengths, hits, _ = nd.label_filter(torch.from_numpy(lab).cuda(), [torch.from_numpy(msk).cuda()])
        assert np.array_equal(lengths, find_object_lengths(lab)) and np.array_equal(hits[:, 0], mask_labels(lab, msk))
        lengths, hits, _ = nd.label_filter(torch.from_numpy(lab).cuda())
        assert np.array_equal(lengths, find_object_lengths(lab)) and hits.shape == (lab.max(), 0)


# ----------------------------------------------------------------------------- tf_correlate1d_sym
LINE_LENGTHS = (1, 2, 63, 65)


def _line_shape(axis, n):
    shape = [3, 4, 5]
    shape[axis] = n
    return tuple(shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gaussian_filter_at_the_largest_radius(nd, axis, dtype):
    """sigma 16 at truncate 4 is radius 64 = TF_C1D_MAX_RADIUS; lines of 1, 2, 63 and 65 samples are all shorter than the
    kernel's reach, so the reflection wraps more than once."""
    import torch
    assert nd.gaussian_kernel1d(16.0)[1] == 64 and nd.gaussian_kernel1d(16.25)[1] == 65
    for n in LINE_LENGTHS:
        rng = np.random.default_rng(10 * axis + n)
        x = (rng.normal(size=_line_shape(axis, n)) * 10).astype(dtype)
        sigma = [0.0, 0.0, 0.0]
        sigma[axis] = 16.0
        got = nd.gaussian_filter(torch.from_numpy(x).cuda(), sigma).cpu().numpy()
        want = ndi.gaussian_filter(x, sigma)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"n = {n}: {int((got != want).sum())} values differ"
        with pytest.raises(ValueError, match="radius"):
            sigma[axis] = 16.25
            nd.gaussian_filter(torch.from_numpy(x).cuda(), sigma)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gaussian_filter_puts_nan_and_inf_where_scipy_puts_them(nd, dtype):
    import torch
    rng = np.random.default_rng(31)
    x = (rng.normal(size=(4, 21, 67)) * 10).astype(dtype)
    r = rng.random(x.shape)
    x[r < 0.004] = np.nan
    x[(r > 0.004) & (r < 0.008)] = np.inf
    x[(r > 0.008) & (r < 0.012)] = -np.inf
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for sigma in ((0, 0.6, 0.6), (0.5, 1.0, 2.0), (0, 0, 16.0), (1.5, 0, 0)):
            want = ndi.gaussian_filter(x, sigma)
            got = nd.gaussian_filter(torch.from_numpy(x).cuda(), sigma).cpu().numpy()
            assert np.isnan(want).any() and np.isfinite(want).any()
            assert np.array_equal(got, want, equal_nan=True), f"sigma {sigma}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} differ"


@pytest.mark.parametrize("dtype,ty", [(np.float32, 0), (np.float64, 1)])
def test_correlate1d_rejects_radius_65_and_asymmetric_kernels_without_writing(L, nd, dtype, ty):
    rng = np.random.default_rng(65)
    shape = (2, 3, 70)
    x = rng.normal(size=shape).astype(dtype)
    src = Guarded(x.size, dtype, 0, x)
    for axis in (0, 1, 2):
        out = Guarded(x.size, dtype)
        w = np.full(131, 1 / 131)                                       # radius 65, symmetric
        assert L.tf_correlate1d_sym(src.ptr, ty, *shape, axis, _p(w), 65, out.ptr, _stream()) == -1
        assert b"radius" in L.tf_last_error()
        w = np.full(129, 1 / 129)                                       # radius 64, not symmetric in its outermost pair
        w[0] *= 1 + 2.0 ** -52
        assert L.tf_correlate1d_sym(src.ptr, ty, *shape, axis, _p(w), 64, out.ptr, _stream()) == -1
        assert b"symmetric" in L.tf_last_error()
        w = np.array([0.25, 0.5, 0.26])
        assert L.tf_correlate1d_sym(src.ptr, ty, *shape, axis, _p(w), 1, out.ptr, _stream()) == -1
        _sync()
        assert out.untouched()
        # the same call with a symmetric radius-64 kernel goes through, inside its guards, and equals SciPy
        w = nd.gaussian_kernel1d(16.0)[0]
        assert L.tf_correlate1d_sym(src.ptr, ty, *shape, axis, _p(w), 64, out.ptr, _stream()) == 0
        assert np.array_equal(out.host(shape), ndi.correlate1d(x, w, axis=axis, mode="reflect"))


# ----------------------------------------------------------------------------- tf_grey_morph
GREY_SHAPES = ((2, 9, 11), (1, 6, 7), (3, 1, 5), (4, 5, 1), (2, 7, 6), (3, 2, 5), (5, 4, 2), (1, 1, 1), (2, 2, 66))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", GREY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grey_morphology_every_point_symmetric_footprint(nd, shape, dtype):
    """ndi.grey_erosion / grey_dilation for every footprint of glue_cases.grey_footprints() with 8 % NaN in the data: where
    the footprint's first cell in C order is off-centre, a NaN there sticks and a NaN elsewhere is ignored."""
    import torch
    rng = np.random.default_rng(7 + sum(shape))
    x = rng.normal(size=shape).astype(dtype)
    x[rng.random(shape) < 0.08] = np.nan
    xd = torch.from_numpy(x).cuda()
    bad = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fname, fp in gl.grey_footprints().items():
            for name in ("grey_erosion", "grey_dilation"):
                want = getattr(ndi, name)(x, footprint=fp)
                got = getattr(nd, name)(xd, fp).cpu().numpy()
                if got.dtype != want.dtype or not np.array_equal(got, want, equal_nan=True):
                    bad.append((fname, name))
    assert not bad, f"{len(bad)} differ from SciPy: {bad[:12]}"
