"""The second stage on the GPU: tf_relabel_merge through ctypes against its NumPy statement (linking_cases.np_relabel_merge)
at the shapes where it can go wrong, and tobac_flow_amd/linking.py on device tensors against tests/golden/linking_ref.npz
and against the same calls on NumPy containers.  Integers throughout: every comparison is an equality."""
import ctypes
import itertools

import numpy as np
import pytest

import label_glue_cases as gc
import linking_cases as lc
from test_linking_cases_cpu import _check, _links_dataset

pytestmark = pytest.mark.gpu
CHAINS = lc.chains()


@pytest.fixture(scope="module")
def L():
    from tobac_flow_amd import _lib
    _lib.device()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold():
    return lc.fixture()


def dev(a, odd=False):
    """the array on the device; odd: at an odd element offset of its allocation (4-byte aligned only)"""
    import torch
    a = np.ascontiguousarray(a)
    if not odd:
        return torch.from_numpy(a).cuda()
    base = torch.zeros(a.size + 1, dtype=torch.from_numpy(a.ravel()[:0]).dtype, device="cuda")
    base[1:] = torch.from_numpy(a.ravel()).cuda()
    return base[1:].view(a.shape)


def run(L, own, lut_own, prev=None, next=None, odd=False, in_place=False):
    """tf_relabel_merge; prev / next: None or (volume, table, frame table).  Returns (out, status[0], status[1])."""
    import torch
    from tobac_flow_amd import _lib
    T, hw = own.shape[0], int(np.prod(own.shape[1:]))
    own_d, lut_d = dev(own.astype(np.int32), odd), dev(np.asarray(lut_own, np.int32))
    keep, args = [], []
    for side in (prev, next):
        if side is None:
            args += [None, 0, None, None, 0]
            continue
        vol, lut, frames = side
        assert np.all(np.asarray(frames) < vol.shape[0]) and len(frames) == T and int(np.prod(vol.shape[1:])) == hw
        tensors = [dev(vol.astype(np.int32), odd), dev(np.asarray(frames, np.int32)), dev(np.asarray(lut, np.int32))]
        keep += tensors
        args += [_lib.ptr(tensors[0]), vol.shape[0], _lib.ptr(tensors[1]), _lib.ptr(tensors[2]), len(lut)]
    out_d = own_d if in_place else dev(np.full(own.shape, -7, np.int32), odd)
    status = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rc = L.tf_relabel_merge(_lib.ptr(own_d), T, hw, _lib.ptr(lut_d), len(lut_own), *args, _lib.ptr(out_d), _lib.ptr(status), None)
    assert rc == 0, L.tf_last_error()
    torch.cuda.synchronize()
    bad, bad_frames = (int(v) for v in status.cpu())
    return out_d.cpu().numpy(), bad, bad_frames


def volumes(rng, T, hw, n_lut, share=0.5):
    v = rng.integers(1, n_lut, (T, hw)) if n_lut > 1 else np.ones((T, hw), np.int64)
    return np.where(rng.random((T, hw)) < share, v, 0).astype(np.int32)


def frame_tables(T, T_other):
    """all -1; contiguous from the window's first frame; permuted with a hole and a repeat"""
    none = np.full(T, -1, np.int32)
    contiguous = none.copy()
    contiguous[:min(T, T_other)] = np.arange(min(T, T_other))
    permuted = np.array([(T_other - 1 - 2 * k) % T_other for k in range(T)], np.int32)
    permuted[T // 2] = -1
    return {"none": none, "contiguous": contiguous, "permuted": permuted}


@pytest.mark.parametrize("hw", (1, 15, 9900))
@pytest.mark.parametrize("T", (1, 5))
def test_relabel_merge_equals_its_statement(L, T, hw):
    rng = np.random.default_rng([T, hw])
    n_own, n_prev, n_next = 9, 6, 40
    luts = [np.concatenate([[0], rng.permutation(np.arange(1, n) * 3)]).astype(np.int32) for n in (n_own, n_prev, n_next)]
    own, before, after = volumes(rng, T, hw, n_own), volumes(rng, 4, hw, n_prev, 0.7), volumes(rng, 3, hw, n_next, 0.7)
    for (tp, prev_frames), (tn, next_frames) in itertools.product(frame_tables(T, 4).items(), frame_tables(T, 3).items()):
        for use_prev, use_next in ((True, False), (False, True), (True, True), (False, False)):
            prev = (before, luts[1], prev_frames) if use_prev else None
            nxt = (after, luts[2], next_frames) if use_next else None
            if (not use_prev and tp != "none") or (not use_next and tn != "none"):
                continue                                     # an absent side has one form
            want, bad = lc.np_relabel_merge(own, luts[0], prev, nxt)
            assert bad == 0
            for odd, in_place in ((False, False), (True, False), (False, True), (True, True)):
                got, n_bad, n_bad_frames = run(L, own, luts[0], prev, nxt, odd, in_place)
                assert np.array_equal(got, want) and (n_bad, n_bad_frames) == (0, 0), (T, hw, tp, tn, use_prev, use_next, odd, in_place)


def test_relabel_merge_counts_the_ids_it_consults(L):
    rng = np.random.default_rng(5)
    T, hw = 3, 15
    lut = np.array([0, 4, 2, 9], np.int32)
    own = rng.integers(0, 4, (T, hw)).astype(np.int32)                 # n_lut - 1 = 3 occurs: accepted
    assert (own == 3).any()
    out, bad, _ = run(L, own, lut)
    assert bad == 0 and np.array_equal(out, lut[own])
    own[0, 3], own[1, 7], own[2, 14] = 4, -1, 2 ** 31 - 1             # n_lut, a negative id, the largest int: counted, result 0
    other = np.full((1, hw), 2, np.int32)
    frames = np.array([0, -1, 0], np.int32)
    for odd in (False, True):
        out, bad, _ = run(L, own, lut, odd=odd)
        want, n = lc.np_relabel_merge(own, lut)
        assert n == 3 and bad == 3 and np.array_equal(out, want) and out[0, 3] == out[1, 7] == out[2, 14] == 0
        # a counted voxel is zero so far: the neighbour is asked under it
        out, bad, _ = run(L, own, lut, prev=(other, lut, frames), odd=odd)
        want, n = lc.np_relabel_merge(own, lut, (other, lut, frames))
        assert n == 3 and bad == 3 and np.array_equal(out, want) and out[0, 3] == 2 and out[1, 7] == 0 and out[2, 14] == 2
    # a one-entry table: every id is outside it
    own = volumes(rng, 2, 15, 5)
    out, bad, _ = run(L, own, np.zeros(1, np.int32))
    assert bad == int((own != 0).sum()) and not out.any()
    # an all-zero window takes everything the neighbours have, the previous one first
    zero = np.zeros((2, 15), np.int32)
    a, b = volumes(rng, 2, 15, 4), volumes(rng, 2, 15, 4, 0.9)
    out, bad, _ = run(L, zero, lut, (a, lut, [1, 0]), (b, lut, [0, 1]))
    assert bad == 0 and np.array_equal(out, np.where(lut[a[[1, 0]]] != 0, lut[a[[1, 0]]], lut[b]))
    # a fully labelled window consults nobody: ids outside the neighbours' tables are not seen
    full = rng.integers(1, 4, (2, 15)).astype(np.int32)
    wild = np.full((2, 15), 1000, np.int32)
    out, bad, _ = run(L, full, lut, (wild, lut, [0, 1]), (-wild, lut, [1, 0]))
    assert bad == 0 and np.array_equal(out, lut[full])
    out, bad, _ = run(L, zero, lut, (wild, lut, [0, -1]), (-wild, lut, [1, 0]))
    assert bad == 15 + 30 and not out.any()


def test_relabel_merge_refuses_bad_arguments(L):
    import torch
    from tobac_flow_amd import _lib
    own = torch.zeros(64, dtype=torch.int32, device="cuda")
    lut = torch.zeros(4, dtype=torch.int32, device="cuda")
    frames = torch.zeros(4, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    none = [None, 0, None, None, 0]
    call = lambda *a: L.tf_relabel_merge(*a)
    assert call(p(own), 4, 16, p(lut), 4, *none, *none, p(own), p(status), None) == 0
    assert call(p(own), 0, 16, p(lut), 4, *none, *none, p(own), p(status), None) == -1
    assert call(p(own), 4, 0, p(lut), 4, *none, *none, p(own), p(status), None) == -1
    assert call(p(own), 4, 16, p(lut), 0, *none, *none, p(own), p(status), None) == -1
    assert call(p(own), 4, 16, p(lut), 4, *none, *none, p(own), None, None) == -1
    assert call(p(own), 4, 16, p(lut), 4, p(own), 4, None, p(lut), 4, *none, p(own), p(status), None) == -1       # no frame table
    assert call(p(own), 4, 16, p(lut), 4, p(own), 4, p(frames), p(lut), 4, *none, p(own), p(status), None) == -1  # out overlaps prev
    shifted = ctypes.c_void_p(own.data_ptr() + 16)
    assert call(p(own), 2, 16, p(lut), 4, *none, *none, shifted, p(status), None) == -1                           # out overlaps own
    torch.cuda.synchronize()


def _device_store(plain_store):
    return lc.to_store(plain_store, "cuda")


@pytest.mark.parametrize("case", list(CHAINS))
def test_package_on_device_tensors_equals_the_fixture(L, gold, case):
    import torch
    from tobac_flow_amd import linking
    names, plain_store = CHAINS[case]
    store = _device_store(plain_store)
    results = [linking.find_overlap_between_files(a, b, store) for a, b in zip(names[:-1], names[1:])]
    for i, result in enumerate(results):
        for kind in ("core", "anvil"):
            lo, hi, x, y = result[kind]
            _check(gold, f"{case}/overlap/{i}/{kind}/", {"minmax": np.array([lo, hi]), "x": x, "y": y})
            assert isinstance(x, np.ndarray) and x.dtype == np.int32 and y.dtype == np.int32
    links = linking.process_linking_output(results)
    _check(gold, f"{case}/links", lc.product_arrays(links))
    for j, name in enumerate(names):
        before = {n: store[name][n].clone() for n, _ in lc.VOLUMES}
        for merge, key in ((False, "relabel"), (True, "merge")):
            ds = linking.relabel_and_merge_file(name, links, store, merge=merge)
            assert all(isinstance(ds[n], torch.Tensor) and ds[n].is_cuda and ds[n].dtype == torch.int32 for n, _ in lc.VOLUMES)
            _check(gold, f"{case}/{key}/{j}/", {n: ds[n].cpu().numpy() for n, _ in lc.VOLUMES})
        # the single steps on tensors: relabel, then the two merges (torch.where on the shared frames)
        ds = linking.relabel_cores_and_anvils(lc.to_label_dataset(plain_store[name], "cuda"), name, links)
        _check(gold, f"{case}/relabel/{j}/", {n: ds[n].cpu().numpy() for n, _ in lc.VOLUMES})
        ds = linking.merge_next_file(linking.merge_previous_file(ds, name, links, store), name, links, store)
        assert all(isinstance(ds[n], torch.Tensor) and ds[n].is_cuda for n, _ in lc.VOLUMES)
        _check(gold, f"{case}/merge/{j}/", {n: ds[n].cpu().numpy() for n, _ in lc.VOLUMES})
        assert all(torch.equal(store[name][n], before[n]) for n in before), "a product of the store was written to"
        # a window on the device beside neighbours on the host
        mixed = dict(lc.to_store(plain_store), **{name: store[name]})
        ds = linking.relabel_and_merge_file(name, links, mixed)
        _check(gold, f"{case}/merge/{j}/", {n: ds[n].cpu().numpy() for n, _ in lc.VOLUMES})


def test_relabel_on_the_device_refuses_ids_outside_the_map(L):
    from tobac_flow_amd import linking
    names, plain_store = CHAINS["tiny"]
    links = _links_dataset(lc.np_link_chain(names, plain_store)[1])
    top = linking.get_core_label_map_for_file(names[1], links).size
    for bad in (top + 1, -1):
        store = _device_store(plain_store)
        store[names[1]]["core_label"][0, 0, 0] = bad
        with pytest.raises(ValueError):
            linking.relabel_cores_and_anvils(store[names[1]], names[1], links)
        with pytest.raises(ValueError):
            linking.relabel_and_merge_file(names[1], links, store)
    store = _device_store(plain_store)
    store[names[1]]["core_label"][0, 0, 0] = top
    linking.relabel_and_merge_file(names[1], links, store)


@pytest.mark.parametrize("world", list(lc.WORLDS))
def test_process_file_on_device_and_on_numpy_containers(L, gold, world):
    import torch
    from tobac_flow_amd import linking
    names, plain_store = CHAINS[world]
    links = _links_dataset(lc.np_link_chain(names, plain_store)[1])
    on_device, on_host = _device_store(plain_store), lc.to_store(plain_store)
    processed = []
    for j, name in enumerate(names):
        d, h = linking.process_file(name, links, on_device), linking.process_file(name, links, on_host)
        assert all(isinstance(d[n], torch.Tensor) and d[n].is_cuda for n, _ in lc.VOLUMES)
        assert all(isinstance(h[n], np.ndarray) for n, _ in lc.VOLUMES)
        got_d, got_h = lc.product_arrays(d), lc.product_arrays(h)
        assert set(got_d) == set(got_h) and all(np.array_equal(got_d[k], got_h[k]) for k in got_d), name
        assert all(d.dims.get(k) == h.dims.get(k) for k in d)
        _check(gold, f"{world}/process/{j}", got_d)
        processed.append(d)
    linking.increment_step_coords(processed[1], processed[0])
    _check(gold, f"{world}/increment/", {k: processed[1].coords[k] for k in ("core_step", "thick_anvil_step", "thin_anvil_step")})


@pytest.mark.parametrize("world", list(lc.WORLDS))
def test_three_windows_end_to_end_reproduce_the_global_labelling(L, world):
    from tobac_flow_amd import linking
    names, plain_store, glob = lc.window_products(world)
    store = _device_store(plain_store)
    links = linking.process_linking_output([linking.find_overlap_between_files(a, b, store) for a, b in zip(names[:-1], names[1:])])
    merged = [linking.relabel_and_merge_file(name, links, store) for name in names]
    for n, _ in lc.VOLUMES:
        got = np.concatenate([m[n].cpu().numpy().ravel() for m in merged])
        truth = np.concatenate([glob[n][a:b].ravel() for a, b in lc.WINDOWS])
        assert np.array_equal(gc.canonical_partition(got), gc.canonical_partition(truth)), n
