"""The watershed set-up on every path its dispatch can take (tobac_flow_amd/csrc/watershed.hip, ws_job_begin): the exact
size of the relevant set (stats[6]) against the NumPy restatement of tests/ws_setup_cases.py, the labels against the
oracle, operand alignment, the NaN rule, the raveled twin and the TF_ENOMEM retry protocol.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import ws_setup_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nbrs():
    return wc.neighbour_lists()


def _from_element(a, skip):
    """`a` on the device as a contiguous view that starts `skip` elements into a larger allocation"""
    import torch
    a = np.array(a, order="C")                                    # (a writable copy: the cases are read-only)
    room = torch.empty(a.size + skip, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    view = room[skip:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous()
    return view


def _operands(c, skip=None, field=None, mask="case"):
    """device operands (fwd, bwd, field, markers, mask) of a case; skip: {operand name: elements past the allocation}"""
    skip = skip or {}
    mask = c["mask"] if isinstance(mask, str) else mask
    src = dict(fwd=c["fwd"].reshape(-1), bwd=c["bwd"].reshape(-1), field=c["field"] if field is None else field,
               markers=c["markers"], mask=mask)
    dev = {k: None if v is None else _from_element(v, skip.get(k, 0)) for k, v in src.items()}
    fwd, bwd = (dev[k].view(c["shape"] + (2,)) for k in ("fwd", "bwd"))
    return fwd, bwd, dev["field"], dev["markers"], dev["mask"]


def _flood(operands, nbr):
    """watershed_dev -> (labels as numpy, stats[6])"""
    from tobac_flow_amd.watershed import watershed_dev
    st = {}
    labels = watershed_dev(*operands, nbr, stats=st)
    return labels.cpu().numpy(), st["sweeps"][6]


@pytest.mark.parametrize("nbr_name", wc.NEIGHBOUR_LISTS)
@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_relevant_count_and_labels(nbrs, name, nbr_name):
    c = wc.cases()[name]
    labels, R = _flood(_operands(c), nbrs[nbr_name])
    want_R = int(wc.relevant(c, nbrs[nbr_name]).sum())
    print(name, nbr_name, "R", R, "restated", want_R)
    assert R == want_R
    want = wc.oracle_labels(name, nbr_name)
    assert labels.dtype == np.int32 and np.array_equal(labels, want), f"{int((labels != want).sum())} px differ"


@pytest.mark.parametrize("name", ["blobs_3x33x48", "blobs_1x5x5", "temporal_4x5x37"])
def test_without_a_mask(nbrs, name):
    """mask = NULL (all ones): the other branch of both classify kernels"""
    from oracle import ws_oracle
    c = dict(wc.cases()[name], mask=None)
    for nbr_name in ("conn1", "conn3"):
        labels, R = _flood(_operands(c, mask=None), nbrs[nbr_name])
        assert R == int(wc.relevant(c, nbrs[nbr_name]).sum())
        want = ws_oracle.watershed(wc.nan_to_zero(c["fwd"]), wc.nan_to_zero(c["bwd"]), c["field"], c["markers"], None, offsets=nbrs[nbr_name])
        assert np.array_equal(labels, want)


ALIGNMENT_VARIANTS = {                       # operand -> (elements skipped, expected data_ptr() residue, modulus)
    "aligned": {},
    "markers": {"markers": (1, 4, 16)},      # one int32 past a 16-byte boundary: the scalar k_ws_classify
    "mask": {"mask": (1, 1, 4)},             # one byte past a 4-byte boundary: the scalar k_ws_classify
    "fwd": {"fwd": (2, 8, 16)},              # one (x, y) pair past a 16-byte boundary: k_ws_relevant<6> instead of 6x4
    "bwd": {"bwd": (2, 8, 16)},
}


@pytest.mark.parametrize("nbr_name", ["conn1", "conn3"])
@pytest.mark.parametrize("name", ["blobs_3x17x20", "blobs_3x33x48", "temporal_3x17x20", "temporal_3x33x48"])
def test_operand_alignment_changes_the_kernels_not_the_result(nbrs, name, nbr_name):
    c = wc.cases()[name]
    want_R, want = int(wc.relevant(c, nbrs[nbr_name]).sum()), wc.oracle_labels(name, nbr_name)
    for variant, spec in ALIGNMENT_VARIANTS.items():
        ops = _operands(c, {k: v[0] for k, v in spec.items()})
        named = dict(zip(("fwd", "bwd", "field", "markers", "mask"), ops))
        for k in ("fwd", "bwd", "markers"):                       # preconditions: the residues the dispatch looks at
            residue, modulus = spec[k][1:] if k in spec else (0, 16)
            assert named[k].data_ptr() % modulus == residue, (variant, k)
        assert named["mask"].data_ptr() % 4 == (spec["mask"][1] if "mask" in spec else 0), variant
        labels, R = _flood(ops, nbrs[nbr_name])
        assert R == want_R, variant
        assert np.array_equal(labels, want), variant


def test_misaligned_flows_fields_and_markers_are_refused_before_any_launch():
    """fwd / bwd not 8-byte aligned, field / markers not 4-byte aligned: TF_EINVAL with a message (the set-up reads a flow
    vector as one float2).  Refusal only: the pointers are never dereferenced."""
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    assert L.tf_version() >= 114                                  # a build with the check
    c = wc.cases()["blobs_2x16x16"]
    T, H, W = c["shape"]
    nbr = wc.neighbour_lists()["conn1"]
    fwd, bwd, field, markers, mask = _operands(c)
    out = torch.zeros(c["shape"], dtype=torch.int32, device="cuda")
    ws = torch.empty(L.tf_watershed_workspace_bytes(T, H, W, len(nbr), 3, 0), dtype=torch.uint8, device="cuda")
    st = np.zeros(16, np.int64)
    base = dict(field=field.data_ptr(), markers=markers.data_ptr(), fwd=fwd.data_ptr(), bwd=bwd.data_ptr())

    def call(**shift):
        p = {k: ctypes.c_void_p(v + shift.get(k, 0)) for k, v in base.items()}
        return L.tf_watershed_ex2(p["field"], p["markers"], _lib.ptr(mask), p["fwd"], p["bwd"], T, H, W, nbr.ctypes.data_as(_lib._P),
                                  len(nbr), 3, 3, 2, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), st.ctypes.data_as(_lib._P), None)

    for shift, word in ((dict(fwd=4), b"fwd and bwd"), (dict(bwd=4), b"fwd and bwd"), (dict(fwd=2), b"fwd and bwd"),
                        (dict(field=2), b"field and markers"), (dict(markers=1), b"field and markers")):
        assert call(**shift) == -1 and word in L.tf_last_error() and b"aligned" in L.tf_last_error(), shift
        assert not out.any() and st[6] == 0
    assert call() == 0 and st[6] == int(wc.relevant(c, nbr).sum())
    assert np.array_equal(out.cpu().numpy(), wc.oracle_labels("blobs_2x16x16", "conn1"))


@pytest.mark.parametrize("shape", [(1, 5, 5), (3, 17, 20)])
def test_nothing_relevant(nbrs, shape):
    """R == 0: a volume that is all markers, and one whose mask is all zero; the labels are the markers"""
    rng = np.random.default_rng(sum(shape))
    from helpers import rand_field, seeds
    z = np.zeros(shape + (2,), np.float32)
    all_markers = rng.integers(1, 9, size=shape).astype(np.int32) * rng.choice(np.array([-1, 1], np.int32), size=shape)
    some = seeds(rng, shape, 3)
    for markers, mask in ((all_markers, None), (all_markers, np.ones(shape, np.int8)), (some, np.zeros(shape, np.int8))):
        c = dict(shape=shape, field=rand_field(rng, shape), markers=markers, mask=mask, fwd=z, bwd=z)
        for nbr_name in ("conn1", "conn3", "custom10"):
            assert not wc.relevant(c, nbrs[nbr_name]).any()
            labels, R = _flood(_operands(c, mask=mask), nbrs[nbr_name])
            assert R == 0 and np.array_equal(labels, markers)


@pytest.mark.parametrize("nbr_name", ["conn1", "conn3"])
def test_field_nan_outside_the_relevant_set_is_accepted(nbrs, nbr_name):
    """field NaN at EVERY irrelevant marker and at every masked-out voxel that is no marker, at once: none of them enters the
    compact arrays, the flood is accepted and the labels are those of the clean field"""
    for name in ("blobs_3x17x20", "blobs_3x33x48"):
        c = wc.cases()[name]
        rel = wc.relevant(c, nbrs[nbr_name])
        marker = c["markers"] != 0
        where = (marker & ~rel) | (~marker & (c["mask"] == 0))
        assert (marker & ~rel).any() and (~marker & (c["mask"] == 0)).any() and not (where & rel).any()
        field = c["field"].copy()
        field[where] = np.nan
        labels, R = _flood(_operands(c, field=field), nbrs[nbr_name])
        assert R == int(rel.sum())
        assert np.array_equal(labels, wc.oracle_labels(name, nbr_name)), name


@pytest.mark.parametrize("nbr_name", ["conn1", "conn3"])
@pytest.mark.parametrize("name", ["temporal_3x17x20", "temporal_2x15x33"])
def test_field_nan_at_a_marker_relevant_only_through_time_is_refused(nbrs, name, nbr_name):
    c = wc.cases()[name]
    only = np.argwhere(wc.temporal_only(c, nbrs[nbr_name]))
    assert len(only)
    field = c["field"].copy()
    field[tuple(only[len(only) // 2])] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        _flood(_operands(c, field=field), nbrs[nbr_name])


@pytest.mark.parametrize("name,nbr_name", [("blobs_3x17x20", "conn1"), ("temporal_2x15x33", "conn3")])
def test_raveled_twin_counts_the_same_relevant_set(nbrs, name, nbr_name):
    """the reference's own arguments (oracle/ws_oracle.prepare: padded, raveled): the padding ring is masked and marker-free,
    so it adds nothing to the relevant set"""
    from oracle import ws_oracle
    from tobac_flow_amd._watershed import watershed_raveled
    c = wc.cases()[name]
    p = ws_oracle.prepare(wc.nan_to_zero(c["fwd"]), wc.nan_to_zero(c["bwd"]), c["field"], c["markers"], c["mask"], offsets=nbrs[nbr_name])
    out = p["out"].ravel().copy()
    st = {}
    watershed_raveled(np.ascontiguousarray(p["field"].ravel()), p["markers"].astype(np.intp), p["nbr"].astype(np.intp), p["fwd_off"],
                      p["bwd_off"], p["fwd_loc"], p["bwd_loc"], p["mask"], p["strides"].astype(np.int32), 0.0, out, False, stats=st)
    assert st["sweeps"][6] == int(wc.relevant(c, nbrs[nbr_name]).sum())
    pd, o = p["pad"], out.reshape(p["out"].shape)
    assert np.array_equal(o[pd[0]:o.shape[0] - pd[0], pd[1]:o.shape[1] - pd[1], pd[2]:o.shape[2] - pd[2]], wc.oracle_labels(name, nbr_name))


@pytest.mark.parametrize("name,nbr_name", [("blobs_3x33x48", "conn1"), ("temporal_3x33x48", "conn3")])
def test_c_abi_reports_the_count_with_enomem_and_accepts_the_retry(nbrs, name, nbr_name):
    """tf_watershed_ex2 with a workspace sized for half the relevant pixels: TF_ENOMEM and stats[6] = the exact count; sized
    for exactly that count: TF_OK and the oracle's labels"""
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    c = wc.cases()[name]
    T, H, W = c["shape"]
    nbr = nbrs[nbr_name]
    R = int(wc.relevant(c, nbr).sum())
    assert R >= 512
    fwd, bwd, field, markers, mask = _operands(c)
    out = torch.zeros(c["shape"], dtype=torch.int32, device="cuda")
    st = np.zeros(16, np.int64)

    def call(max_relevant):
        ws = torch.empty(L.tf_watershed_workspace_bytes(T, H, W, len(nbr), 3, max_relevant), dtype=torch.uint8, device="cuda")
        return L.tf_watershed_ex2(_lib.ptr(field), _lib.ptr(markers), _lib.ptr(mask), _lib.ptr(fwd), _lib.ptr(bwd), T, H, W,
                                  nbr.ctypes.data_as(_lib._P), len(nbr), 3, 3, 2, _lib.ptr(out), None, _lib.ptr(ws), ws.numel(),
                                  st.ctypes.data_as(_lib._P), None)

    assert call(R // 2) == -2 and st[6] == R and b"relevant" in L.tf_last_error()
    assert call(R) == 0 and st[6] == R
    assert np.array_equal(out.cpu().numpy(), wc.oracle_labels(name, nbr_name))


def test_python_retry_and_memo(nbrs, monkeypatch):
    """watershed_begin sizes the workspace from a guess -- 1.5 x floodable + 4096 on the first call of a shape, 1.25 x the
    previous call's count + 4096 afterwards -- and starts again with the exact count when the library answers TF_ENOMEM.
    (4, 64, 64), zero flows, connectivity 1, markers everywhere except [:, ::2, ::2]: floodable 4096, relevant 12288, first
    guess 10240 (tests/test_ws_setup_cases_cpu.py holds these figures).  The library is handed the whole scratch buffer of the
    job's slot, which only grows: each call here starts without one, as the first flood of a process does."""
    import torch
    from helpers import rand_field
    from oracle import ws_oracle
    from tobac_flow_amd import _lib, watershed as W
    shape, nbr = (4, 64, 64), nbrs["conn1"]
    rng = np.random.default_rng(64)
    z = np.zeros(shape + (2,), np.float32)
    field = rand_field(rng, shape)
    dense = (np.arange(np.prod(shape), dtype=np.int32).reshape(shape) % 5 + 1)
    dense[:, ::2, ::2] = 0
    sparse, sparse_mask = np.zeros(shape, np.int32), np.zeros(shape, np.int8)
    sparse[1, 10:13, 10:13] = 3
    sparse_mask[:, 6:16, 6:18] = 1
    cases = [dict(shape=shape, field=field, markers=m, mask=k, fwd=z, bwd=z) for m, k in ((dense, None), (sparse, sparse_mask))]
    want_R = [int(wc.relevant(c, nbr).sum()) for c in cases]
    assert want_R[0] == 12288 and 100 < want_R[1] < 1000 and int(want_R[1] * 1.25) + 4096 < 12288
    want = [ws_oracle.watershed(z, z, field, c["markers"], c["mask"], offsets=nbr) for c in cases]

    L = _lib.lib()
    begin, codes = L.tf_watershed_begin, []

    def recording(*args):
        codes.append(begin(*args))
        return codes[-1]
    monkeypatch.setattr(L, "tf_watershed_begin", recording)
    with W._MEMO_LOCK:
        for key in [k for k in W._relevant_memo if k[:3] == shape]:
            del W._relevant_memo[key]
    key = shape + (len(nbr), W.DEFAULT_CHAIN_DEPTH, torch.cuda.current_stream().cuda_stream)

    for which, expect in ((0, [-2, 0]), (1, [0]), (0, [-2, 0])):
        del codes[:]
        for slot in range(8):                 # the scratch of a flood is grow-only per slot: one left over from a larger flood of
            _lib.release_workspaces("watershed_job%d" % slot)     # this process would be handed over whole and hide the retry
        c = cases[which]
        labels, R = _flood(_operands(c, mask=c["mask"]), nbr)
        assert codes == expect, (which, codes)
        assert R == want_R[which] and W._relevant_memo[key] == want_R[which]
        assert np.array_equal(labels, want[which])
