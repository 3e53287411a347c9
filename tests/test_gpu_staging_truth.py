"""The staging cache from the device side (tobac_flow_amd/_staging.py, csrc/staging.hip): tests/test_gpu_staging.py shows
that equal content hits and that an edited HOST array misses; these tests show that the DEVICE tensor served on a hit
holds the bytes that were presented.

  A  a tensor the caller owns is never served as the twin of the array to_host made from it, whatever the caller does to
     the tensor afterwards;
  B  a pinned pool block is not handed to its next owner while a copy out of it is pending;
  C  TF_HOST_CACHE_VERIFY=1 re-hashes the twin on every hit and refuses a stale one -- and with it switched on, every public
     function that shares or remembers a twin (tests/staging_sweep_cases.py) gives the same arrays recognised as uploaded;
  D  the key keeps dtypes and shapes apart.

Bit-exact work throughout: every comparison is equality.  No test here trims the pinned pool (`_staging.clear(trim=False)`
only): B must never let the pool unmap a block a copy may still have to read."""
import gc
import time

import numpy as np
import pytest

import staging_sweep_cases as sweep

pytestmark = pytest.mark.gpu

SHAPE = sweep.SHAPE


@pytest.fixture
def staging(monkeypatch):
    """the cache switched on at its default budget, verify off, empty before and after"""
    from tobac_flow_amd import _staging
    monkeypatch.delenv("TF_HOST_CACHE_GB", raising=False)
    monkeypatch.delenv("TF_HOST_CACHE_VERIFY", raising=False)
    _staging.clear(trim=False)
    yield _staging
    _staging.clear(trim=False)


def _owned(kind):
    """a device tensor the TEST owns, and the object handed to to_host"""
    import torch
    from tobac_flow_amd.detection import DeviceField
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "int32":
        t = torch.randint(0, 50, SHAPE, dtype=torch.int32, device="cuda", generator=g)
    elif kind == "non_contiguous":                                       # (.contiguous() inside download is a private copy already)
        t = torch.randint(0, 50, (SHAPE[0], SHAPE[2], SHAPE[1]), dtype=torch.int32, device="cuda", generator=g).transpose(1, 2)
        assert tuple(t.shape) == SHAPE and not t.is_contiguous()
    else:
        t = torch.randn(SHAPE, dtype=torch.float32, device="cuda", generator=g)
    return t, (DeviceField(t, np.arange(SHAPE[0]).astype("datetime64[m]")) if kind == "device_field" else t)


@pytest.mark.parametrize("change", ["add", "copy"])
@pytest.mark.parametrize("kind", ["int32", "float32", "device_field", "non_contiguous"])
def test_a_hit_serves_the_presented_bytes_whatever_became_of_the_callers_tensor(staging, kind, change):
    import torch
    import tobac_flow_amd
    from tobac_flow_amd import _lib
    t, handed = _owned(kind)
    host = tobac_flow_amd.to_host(handed)
    kept = host.copy()
    assert torch.equal(t.cpu(), torch.from_numpy(host))
    if change == "add":
        t.add_(1)
    else:
        t.copy_(torch.flip(t, (0,)) * 3 + 7)                            # "the next group"
    assert not torch.equal(t.cpu(), torch.from_numpy(host)) and np.array_equal(host, kept)
    for served in (staging.upload(host), _lib.to_dev(host, share=True), staging.upload(kept)):
        assert served.dtype == t.dtype and tuple(served.shape) == host.shape
        wrong = int((served.cpu() != torch.from_numpy(host)).sum())
        assert wrong == 0, f"{wrong} of {host.size} elements served are not the bytes presented"
        assert served.data_ptr() != t.data_ptr()                         # nobody is handed the caller's own storage


def test_an_entry_point_gets_the_markers_that_were_presented_not_the_zeroed_tensor(staging, monkeypatch):
    import torch
    import tobac_flow_amd
    import tobac_flow_amd.flow as tf
    from helpers import seeds
    edges = sweep._blobs(SHAPE, 3).astype(np.float32)
    flow = tf.Flow(np.zeros(SHAPE + (2,), np.float32), np.zeros(SHAPE + (2,), np.float32))
    seeds_dev = torch.from_numpy(seeds(np.random.default_rng(4), SHAPE, 40)).cuda()
    markers_host = tobac_flow_amd.to_host(seeds_dev)
    assert markers_host.nbytes >= 1 << 20 and int(markers_host.max()) == 40
    seeds_dev.zero_()
    got = flow.watershed(edges, markers_host)
    monkeypatch.setenv("TF_HOST_CACHE_GB", "0")
    want = flow.watershed(edges, markers_host.copy())
    assert int(want.max()) == 40 and np.count_nonzero(want) > 40 * 9     # the flood did flood
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_a_pinned_block_is_not_reused_under_a_pending_copy(staging):
    """An upload out of a pool block behind a long spin on the stream; the block dropped, handed out again and overwritten by
    its new owner at once.  The device tensor must hold what the block held when upload() was called.  The proof needs the
    copy to have been pending while the host steps ran: the event behind the spin had not completed just before the
    upload, and the spin lasted at least five times as long as the host steps take (timed in a dry run)."""
    import torch
    from tobac_flow_amd import _lib, _staging
    shape = (2, 1024, 1024)                                              # 8 MiB of int32: its own size class of the pool
    a = np.arange(np.prod(shape), dtype=np.int32).reshape(shape)
    b = a ^ np.int32(0x5A5A5A5A)                                         # differs from a in every element
    # the pool hands out the OLDEST free block of a size class: every free one of this class is taken out and held for the
    # duration (nothing is trimmed), so that the block dropped below is the one handed out next
    spare = _lib.lib().tf_host_pool_spare(a.nbytes)
    held = [_staging.empty_pinned(shape, np.int32) for _ in range(spare)]
    assert _lib.lib().tf_host_pool_spare(a.nbytes) == 0
    # dry run of the host steps, nothing pending: what they cost, and that the pool does hand the same block out again
    blk = _staging.empty_pinned(shape, np.int32)
    blk[...] = a
    ptr = blk.ctypes.data
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    del blk
    gc.collect()
    blk2 = _staging.empty_pinned(shape, np.int32)
    blk2[...] = b
    host_ms = (time.perf_counter() - t0) * 1e3
    assert blk2.ctypes.data == ptr
    del blk2
    gc.collect()
    # one calibration call of the spin kernel (after a first launch that pays for loading it), timed here
    before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 20_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    before.record()
    torch.cuda._sleep(probe)
    after.record()
    torch.cuda.synchronize()
    probe_ms = before.elapsed_time(after)
    assert probe_ms > 0.0
    target_ms = max(10.0 * host_ms, 100.0)                               # twice what the proof asks for
    cycles = int(probe * target_ms / probe_ms)
    print(f"host steps {host_ms:.2f} ms; {probe} cycles spin {probe_ms:.2f} ms; spinning {cycles} cycles for {target_ms:.0f} ms")
    blk = _staging.empty_pinned(shape, np.int32)
    blk[...] = a
    assert blk.ctypes.data == ptr
    torch.cuda.synchronize()
    before.record()
    torch.cuda._sleep(cycles)
    after.record()
    pending = not after.query()
    d = _staging.upload(blk, fresh=True)
    del blk
    gc.collect()
    blk2 = _staging.empty_pinned(shape, np.int32)
    blk2[...] = b
    torch.cuda.synchronize()
    spin_ms = before.elapsed_time(after)
    print(f"the spin took {spin_ms:.2f} ms; pending before the upload: {pending}")
    assert pending, "the spin had finished before upload() was called: nothing was pending"
    assert spin_ms >= 5.0 * host_ms, (spin_ms, host_ms)
    assert blk2.ctypes.data == ptr                                       # the new owner did get the block the copy read
    wrong = int((d.cpu() != torch.from_numpy(a)).sum())
    assert wrong == 0, f"{wrong} of {a.size} elements are not what the block held when upload() was called"
    assert np.array_equal(blk2, b)                                       # ... and nothing was copied late into the new owner's block
    del held


def test_verify_refuses_a_twin_that_was_written_into_and_uploads_again(staging, monkeypatch):
    import torch
    monkeypatch.setenv("TF_HOST_CACHE_VERIFY", "1")
    a = np.random.default_rng(21).normal(size=SHAPE).astype(np.float32)
    d1 = staging.upload(a)
    assert staging._cache_bytes == a.nbytes and len(staging._CACHE) == 1
    d1.add_(1)
    s0 = dict(staging.stats)
    with pytest.raises(RuntimeError, match=r"float32 array of shape \(6, 300, 400\)"):
        staging.upload(a)
    assert staging._cache_bytes == 0 and not staging._CACHE and not any(staging._SIGS.values())
    assert staging.stats["hits"] == s0["hits"] and staging.stats["verified"] == s0["verified"]
    d2 = staging.upload(a)                                               # no candidate is left: uploaded, and remembered again
    assert d2 is not d1 and staging.stats["uploads"] == s0["uploads"] + 1 and torch.equal(d2.cpu(), torch.from_numpy(a))
    assert staging.upload(a) is d2 and staging._cache_bytes == a.nbytes and len(staging._CACHE) == 1


def test_verify_counts_one_check_per_hit_and_none_when_switched_off(staging, monkeypatch):
    a = np.random.default_rng(22).integers(0, 99, SHAPE).astype(np.int32)
    d = staging.upload(a)
    s0 = dict(staging.stats)
    assert "verified" in s0
    assert staging.upload(a) is d and staging.upload(a.copy()) is d
    assert staging.stats["hits"] == s0["hits"] + 2 and staging.stats["verified"] == s0["verified"]
    monkeypatch.setenv("TF_HOST_CACHE_VERIFY", "1")                      # read per call
    for k in range(1, 4):
        assert staging.upload(a.copy()) is d
        assert staging.stats["verified"] == s0["verified"] + k and staging.stats["hits"] == s0["hits"] + 2 + k
    monkeypatch.setenv("TF_HOST_CACHE_VERIFY", "0")
    assert staging.upload(a) is d and staging.stats["verified"] == s0["verified"] + 3


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind in "mM":
        return np.array_equal(a.view(np.int64), b.view(np.int64))       # (NaT equal to NaT)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.mark.parametrize("name", list(sweep.CASES))
def test_sweep_recognised_arguments_give_what_uploaded_ones_give(staging, monkeypatch, name):
    """The case twice with the cache and verify on -- the second call's arguments are fresh copies, recognised by content,
    every hit re-hashed -- and once with recognition off.  No verify error, at least one verified hit in the second call
    (or the case proves nothing), and the three results equal array for array."""
    case = sweep.CASES[name]
    monkeypatch.setenv("TF_HOST_CACHE_VERIFY", "1")
    first = case()
    s0 = dict(staging.stats)
    second = case()
    verified, hits = staging.stats["verified"] - s0["verified"], staging.stats["hits"] - s0["hits"]
    monkeypatch.setenv("TF_HOST_CACHE_GB", "0")
    s1 = dict(staging.stats)
    plain = case()
    assert staging.stats["hits"] == s1["hits"]
    print(f"sweep {name}: {verified} verified hits in the second call")
    assert verified >= 1 and verified == hits, (name, verified, hits)
    assert set(first) == set(second) == set(plain) and first
    for key in plain:
        assert _same(plain[key], first[key]) and _same(plain[key], second[key]), (name, key)


def test_the_key_keeps_dtypes_and_shapes_apart(staging):
    import torch
    x = np.random.default_rng(23).normal(size=SHAPE).astype(np.float32)
    as_int, turned = x.view(np.int32), x.reshape(SHAPE[1], SHAPE[0], SHAPE[2])
    dx = staging.upload(x)
    s0 = dict(staging.stats)
    di, dt = staging.upload(as_int), staging.upload(turned)
    assert staging.stats["hits"] == s0["hits"] and staging.stats["uploads"] == s0["uploads"] + 2
    assert di.dtype == torch.int32 and tuple(di.shape) == SHAPE and torch.equal(di.cpu(), torch.from_numpy(as_int))
    assert dt.dtype == torch.float32 and tuple(dt.shape) == turned.shape and torch.equal(dt.cpu(), torch.from_numpy(turned))
    assert len({dx.data_ptr(), di.data_ptr(), dt.data_ptr()}) == 3
    assert staging.upload(x) is dx and staging.upload(as_int.copy()) is di and staging.upload(turned.copy()) is dt
    # a bool array travels as its bytes: it may share a twin with the uint8 array of the same bytes, and both come back uint8
    m = np.random.default_rng(24).random((5, 700, 900)) > 0.5
    dm, du = staging.upload(m), staging.upload(m.view(np.uint8).copy())
    for d in (dm, du):
        assert d.dtype == torch.uint8 and tuple(d.shape) == m.shape and torch.equal(d.cpu(), torch.from_numpy(m.view(np.uint8)))
