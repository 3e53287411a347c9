"""The two work layouts of csrc/label_runs.h at their edges, through every entry point that uses them, against the NumPy
restatements of tests/wstats_cases.py, tests/validation_cases.py and tests/label_filter_cases.py and a per-id NumPy pass
for tf_label_props.  Only what no other GPU test reaches is here.

Raveled walker (tf_label_wstats, tf_label_proportions, tf_label_nanmin).  Reached elsewhere: a tail that is no multiple
of 4 and a plane that no lane's four voxels fit (test_gpu_wstats' tie case, 621 voxels, hw = 207), ids beyond n_labels
(its short index), several workgroups and misaligned operands for tf_label_nanmin alone (test_gpu_validation).  Here:
  * n in {1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097}: the tail m < 4, the last lane of a wave's span, the workgroup's end;
  * a lane whose voxels i and i + 256 carry one label while the voxels between them (other lanes') carry another: the
    open run continues across steps; and a lane with a background-only step between two steps of one label: the run is
    flushed and reopened, not counted twice;
  * ids 0, negative and > n_labels next to valid ones (every volume here);
  * plane weights with hw in {1, 3, 5, 6, 8}: straddling the plane's end, wrapping more than once, hw % 4 == 0;
  * every operand as a view that starts one element past a 16-byte boundary (every case, `shifted`).
Row chunks (tf_label_props on lr_walk_row, tf_label_filter on its own loop over the same chunks).  Reached elsewhere: W % 4 != 0 with an aligned base (67), a run that ends
in a row's last voxel and continues in the next row's first (test_label_props_runs_do_not_straddle_rows, the filter's
"odd" volume), W % 4 == 0 with a base 4 bytes off and n_labels == 0 for the filter (its "aligned" and "zero" volumes).
Here: W in {1, 15, 16, 17, 33} for both, each also with the base 4 bytes off (W = 16: the props kernel's W % 4 == 0 case).

Bounds.  Counts, extremes, the errors at them, minima, frame ranges and hit bits are exact.  Fields, errors and weights
are small dyadic rationals, so the sums of pass 1 are exact in double in any order; the record's sum of weights is still
held to the project's bound for a sum in another order, 2 (n - 1) 2^-53 sum|term|, as are the sums of tf_label_props.
Mean, std, uncertainty and combined error are held to test_gpu_wstats' rtol 1e-9 (positive terms, the cancelling sum taken
about the finished mean on both sides), proportions to its rtol 1e-12."""
import numpy as np
import pytest

import label_filter_cases as lc
import validation_cases as vc
import wstats_cases as wc

pytestmark = pytest.mark.gpu

N_LABELS = 9
EDGE_N = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097)
FLAG_VALUES = np.array([2, -1, 40, 0], np.int32)                 # 40 never occurs, 1 occurs and is not listed


def _dev(a, shifted):
    """the array on the device, contiguous; with `shifted` its base is one element past a 16-byte aligned address"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(a))
    if not shifted:
        return src.cuda()
    size, nbytes = src.element_size(), src.numel() * src.element_size()
    raw = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    out = raw[size:size + nbytes].view(src.dtype).view(src.shape)
    out.copy_(src)
    assert out.is_contiguous() and raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == size % 16
    return out


def _sum_bound(terms):
    return 2.0 * max(terms.size - 1, 0) * 2.0 ** -53 * float(np.abs(terms).sum())


# ---- the raveled walker ----------------------------------------------------------------------------------------------
def _labels(n, run=53, gap=37):
    """runs of ids -1 .. 10 with background between them (0, negative and > N_LABELS next to valid ids); the first and the
    last voxel are labelled, so that a tail counts"""
    i = np.arange(n)
    lab = np.where(((i + gap) // gap) % 3 == 0, 0, (i // run + 3) % 12 - 1).astype(np.int32)
    lab[0], lab[-1] = 2, 1
    return lab


def _steps_volume():
    """4096 + 1024 voxels.  In both workgroups, wave 0: lane 0 holds voxels 0-3, 256-259, 512-515, 768-771, all of label 3,
    while every voxel between them is of label 5; lane 1 holds label 4 in its steps 0 and 2 and background in steps 1, 3."""
    lab = np.full(4096 + 1024, 5, np.int32)
    for base in (0, 4096):
        for step in range(4):
            lab[base + 256 * step:base + 256 * step + 4] = 3
            lab[base + 256 * step + 4:base + 256 * step + 8] = 4 if step % 2 == 0 else 0
    return lab


def _operands(n, hw, plane, seed):
    rng = np.random.default_rng(seed)
    x = (200 + rng.integers(0, 64, n)) / 8.0                      # ties on purpose
    r = rng.integers(0, 50, n)
    x[r == 0], x[r == 1], x[r == 2], x[r == 3] = np.nan, np.inf, -np.inf, -0.0
    e = (1 + rng.integers(0, 9, n)) / 16.0
    m = hw if plane else n
    w = (1 + np.arange(m) % 9) / 4.0                              # neighbours differ: a wrong plane index shows
    if m > 12:
        w[rng.integers(0, m, m // 6)] = 0.0
    flags = ((np.arange(n) // 3) % 5 - 1).astype(np.int32)
    wf = w.astype(np.float32)
    if m > 12:
        wf[rng.integers(0, m, m // 10)] = np.nan
    return x, e, w, flags, wf


def _wstats(labels, x, e, w, hw, plane, shifted):
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    code = _lib.TF_F32 if x.dtype == np.float32 else _lib.TF_F64
    lab, xd, ed, wd = (_dev(a, shifted) for a in (labels, x, e, w))
    out = torch.full((N_LABELS, 10), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.tf_label_wstats_workspace_bytes(N_LABELS), dtype=torch.uint8, device="cuda")
    _lib.check(L.tf_label_wstats(_lib.ptr(lab), _lib.ptr(xd), _lib.ptr(ed), _lib.ptr(wd), code, labels.size // hw, hw, int(plane),
                                 N_LABELS, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_wstats")
    return out.cpu().numpy()


def _proportions(labels, flags, wf, hw, plane, shifted):
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    lab, fd, wd = (_dev(a, shifted) for a in (labels, flags, wf))
    K = FLAG_VALUES.size
    out = torch.full((N_LABELS, K), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.tf_label_proportions_workspace_bytes(N_LABELS, K), dtype=torch.uint8, device="cuda")
    _lib.check(L.tf_label_proportions(_lib.ptr(lab), _lib.ptr(fd), _lib.ptr(wd), labels.size // hw, hw, int(plane), N_LABELS,
                                      FLAG_VALUES.ctypes.data, K, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
               "tf_label_proportions")
    return out.cpu().numpy()


def _nanmin(labels, field, ids, shifted):
    import torch
    from tobac_flow_amd import _lib
    L = _lib.lib()
    code = {np.dtype(np.float32): _lib.TF_F32, np.dtype(np.float64): _lib.TF_F64, np.dtype(np.uint8): _lib.TF_U8}[field.dtype]
    lab, fd, idd = _dev(labels, shifted), _dev(field, shifted), _dev(ids, False)
    mins = torch.full((ids.size,), -7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((ids.size,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.tf_label_nanmin_workspace_bytes(N_LABELS), dtype=torch.uint8, device="cuda")
    _lib.check(L.tf_label_nanmin(_lib.ptr(lab), _lib.ptr(fd), code, labels.size, N_LABELS, _lib.ptr(idd), ids.size, _lib.ptr(mins),
                                 _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "tf_label_nanmin")
    return mins.cpu().numpy(), counts.cpu().numpy()


def _check_raveled(labels, hw, plane, shifted, seed):
    n = labels.size
    index = np.arange(1, N_LABELS + 1)
    x, e, w, flags, wf = _operands(n, hw, plane, seed)
    shaped = labels.reshape(n // hw, hw)                          # a (hw,) plane broadcasts against it
    w_all = np.broadcast_to(w, shaped.shape).ravel()
    for dtype in (np.float32, np.float64):                        # the values are exact in float32 too
        xs, es, ws_ = x.astype(dtype), e.astype(dtype), w.astype(dtype)
        got = _wstats(labels, xs, es, ws_, hw, plane, shifted)
        want = wc.restate_stats(shaped, xs.reshape(shaped.shape), es.reshape(shaped.shape), ws_, index)
        what = (n, hw, plane, shifted, np.dtype(dtype).name)
        for k, i in enumerate(index):
            at = (labels == i) & np.isfinite(x)
            assert got[k, 0] == at.sum(), what
            assert abs(got[k, 1] - w_all[at].sum()) <= _sum_bound(w_all[at]), what
        assert np.array_equal(np.isnan(got[:, 2:]), np.isnan(want)), what
        assert np.array_equal(got[:, [4, 5, 8, 9]], want[:, [2, 3, 6, 7]], equal_nan=True), what
        summed, ours = want[:, [0, 1, 4, 5]], got[:, [2, 3, 6, 7]]
        ok = ~np.isnan(summed)
        assert np.all(np.abs(ours[ok] - summed[ok]) <= 1e-9 * np.abs(summed[ok])), what
    got = _proportions(labels, flags, wf, hw, plane, shifted)
    want = wc.restate_proportions(shaped, flags.reshape(shaped.shape), wf, FLAG_VALUES, index)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (n, hw, plane, shifted)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    ids = np.append(index, [N_LABELS + 3, 7]).astype(np.int64)    # one beyond n_labels, one twice
    nan_field = np.where(np.isin(labels, (4,)), np.nan, np.where(np.isneginf(x), np.nan, x))      # label 4 is all NaN
    for field in (nan_field.astype(np.float32), nan_field, (flags > 0).astype(np.uint8)):
        mins, counts = _nanmin(labels, field, ids, shifted)
        want = vc.restate_label_nanmin(labels, field, ids, np.nan).astype(np.float64)
        want[ids > N_LABELS] = np.nan
        assert np.array_equal(mins, want, equal_nan=True), (n, shifted, field.dtype)
        want_counts = [int(np.sum(~np.isnan(field[labels == i].astype(np.float64)))) if i <= N_LABELS and (labels == i).any() else -1
                       for i in ids]
        assert counts.tolist() == want_counts, (n, shifted, field.dtype)


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n", EDGE_N)
def test_raveled_walker_at_tails_and_span_ends(n, shifted):
    _check_raveled(_labels(n), n, False, shifted, seed=n)


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
def test_raveled_walker_keeps_a_run_across_steps_and_reopens_it_after_a_background_step(shifted):
    labels = _steps_volume()
    _check_raveled(labels, labels.size, False, shifted, seed=77)
    # the record itself: lane 1's two steps of label 4 are 8 voxels per workgroup, counted once each
    x = np.full(labels.size, 25.0, np.float32)
    got = _wstats(labels, x, x, x, labels.size, False, shifted)
    assert got[:, 0].tolist() == [0, 0, 32, 16, labels.size - 64, 0, 0, 0, 0]


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw", [1, 3, 5, 6, 8])
def test_raveled_walker_plane_weights_that_straddle_and_wrap(hw, shifted):
    T = 173                                                       # n = 173 hw: odd tails, more than one wave's step
    _check_raveled(_labels(T * hw), hw, True, shifted, seed=hw)


# ---- the row chunks --------------------------------------------------------------------------------------------------
ROW_W = (1, 15, 16, 17, 33)


def _row_volume(W):
    """(2, 3, W): short runs of _labels laid along the rows, so that they end and begin wherever the rows do"""
    return _labels(6 * W, run=7, gap=5).reshape(2, 3, W)


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("W", ROW_W)
def test_row_chunks_label_props_at_row_widths_around_the_chunk(W, shifted):
    from tobac_flow_amd.label import label_props
    labels = _row_volume(W)
    T, H, _ = labels.shape
    rng = np.random.default_rng(W)
    area = 1.0 + rng.random((H, W))
    area[0, 0] = np.nan                                           # under labels[:, 0, 0] == 2
    xs, ys = np.linspace(-0.07, 0.11, W), np.linspace(0.09, -0.04, H)
    lat, lon = rng.normal(size=(H, W)) * 40.0, rng.normal(size=(H, W)) * 140.0
    rank = np.array([1, 0], np.int32)
    got = label_props(_dev(labels, shifted), N_LABELS, area=area, x=xs, y=ys, lat=lat, lon=lon, t_rank=rank)
    assert got.shape == (N_LABELS + 1,) and got["count"][0] == 0
    for i in range(1, N_LABELS + 1):
        tt, yy, xx = np.nonzero(labels == i)
        assert got["count"][i] == tt.size, (W, shifted, i)
        if not tt.size:
            assert got["tmin"][i] == 0x7fffffff and got["tmax"][i] == -1 and got["w"][i] == 0
            continue
        assert got["tmin"][i] == rank[tt].min() and got["tmax"][i] == rank[tt].max(), (W, shifted, i)
        a = area[yy, xx]
        for key, terms in (("area_nansum", a[~np.isnan(a)]), ("w", a), ("wx", a * xs[xx]), ("wy", a * ys[yy]),
                           ("wlat", a * lat[yy, xx]), ("wlon", a * lon[yy, xx])):
            if np.isnan(terms).any():
                assert np.isnan(got[key][i]), (W, shifted, i, key)
            else:
                assert abs(got[key][i] - terms.sum()) <= _sum_bound(terms), (W, shifted, i, key)
    assert np.isnan(got["w"][2]) and not np.isnan(got["area_nansum"][2])


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "shifted"])
@pytest.mark.parametrize("W", ROW_W)
def test_row_chunks_label_filter_at_row_widths_around_the_chunk(W, shifted):
    import torch
    from tobac_flow_amd import _lib
    labels = _row_volume(W)
    T, H, _ = labels.shape
    rng = np.random.default_rng(100 + W)
    fields = dict(m=rng.random(labels.shape) < 0.1, f=rng.normal(size=labels.shape).astype(np.float32), g=rng.normal(size=labels.shape))
    fields["f"][0, 0, 0] = np.nan
    case = dict(fields=fields)
    criteria = [("mask", "m"), ("f", ">=", 1.0), ("g", "<", -1.0), ("f", "<", -3.5)]
    crit = (_lib.LabelCriterion * len(criteria))()
    keep = []
    for k, q in enumerate(criteria):
        if q[0] == "mask":
            keep.append(_dev(fields[q[1]].view(np.uint8), shifted))
            crit[k] = _lib.LabelCriterion(keep[-1].data_ptr(), _lib.TF_U8, 0, 0.0)
        else:
            keep.append(_dev(fields[q[0]], shifted))
            crit[k] = _lib.LabelCriterion(keep[-1].data_ptr(), _lib.TF_F32 if q[0] == "f" else _lib.TF_F64, _lib.CMP_OPS[q[1]], q[2])
    lab = _dev(labels, shifted)
    rec = torch.full((N_LABELS + 1, 4), 12345, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().tf_label_filter(_lib.ptr(lab), T, H, W, N_LABELS, crit, len(criteria), _lib.ptr(rec), _lib.stream_ptr()),
               "tf_label_filter")
    want = lc.restate(labels, N_LABELS, [lc.satisfied(case, q) for q in criteria])
    assert np.array_equal(rec.cpu().numpy(), want), (W, shifted)
