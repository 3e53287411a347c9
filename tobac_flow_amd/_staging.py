"""Host containers <-> HBM for the entry points that keep the reference's numpy / xarray interface
(/root/reference/tobac_flow/decorators.py:21-61; /root/reference/scripts/dcc_detect_goes.py:164-303 hand every entry point
host arrays and get host arrays back).  Plumbing over the library's staging entry points (include/tobac_flow_hip.h, "host
staging"; csrc/staging.hip):

  * `upload(array)`   host array -> device tensor through the pinned staging ring (host threads + pipelined DMA) -- and at most
    ONCE per content: every upload is remembered by its 128-bit content checksum, and an array presented again -- the same
    object handed to the next entry point (bt to create_flow, then to detect_cores), a label volume this package returned
    coming back as `markers=`, or another temporary with the same values (`wvd - swd` evaluated for get_anvil_markers and
    again for detect_anvils) -- is recognised by hashing it on the host (read-only, no PCIe) and served from HBM.  Content,
    never the address: a mutated or recycled buffer hashes differently and is uploaded.
  * `download(tensor)` device tensor -> numpy array that lives in a pooled PINNED block (DMA at the link's rate, no second
    host copy); the block goes back to the pool when the array and all its views are gone.  The device tensor stays in the
    cache as the array's twin (its checksum computed on the device: the same function, word for word).

The cache holds device memory: at most TF_HOST_CACHE_GB (default 32; 0 switches recognition off), least recently used
first out; `clear()` drops it.  Cached twins are shared, read-only by convention: the recipes never write into their inputs
(the same convention device-resident callers rely on), and `upload(..., fresh=True)` gives a private tensor where one is
going to be written.  Only tensors this package made are remembered: an upload's destination, and a result downloaded with
remember=True (the caller gets the host array, never the tensor).  TF_HOST_CACHE_VERIFY=1 checks the convention: every hit
re-hashes the twin on the device and raises if it no longer holds the content it is remembered by."""
import ctypes
import os
import threading
import time
from collections import OrderedDict

import numpy as np

from tobac_flow_amd import _lib

_MIN_CACHED = 1 << 20                     # arrays below 1 MiB are not worth a checksum
_LOCK = threading.Lock()
_CACHE = OrderedDict()                    # (nbytes, dtype str, shape, device, h0, h1) -> (device tensor, event behind its last write)
_cache_bytes = 0
_SIGS = {}                                # (nbytes, dtype str, shape, device) -> {sample signature: entries with it} (see _sample_sig)
stats = {"uploads": 0, "upload_bytes": 0, "hits": 0, "hit_bytes": 0, "downloads": 0, "download_bytes": 0, "verified": 0,
         "hash_s": 0.0, "upload_s": 0.0, "download_s": 0.0, "pinned_alloc_s": 0.0}      # (host seconds spent in each part)


def _budget():
    return int(float(os.environ.get("TF_HOST_CACHE_GB", "32")) * 1e9)


def _verify():
    """TF_HOST_CACHE_VERIFY=1: every hit re-hashes the twin on the device before it is served (_lookup)"""
    return os.environ.get("TF_HOST_CACHE_VERIFY", "0") not in ("", "0")


def _forget(key):
    """drop one entry and its share of _SIGS and _cache_bytes (called with _LOCK held)"""
    global _cache_bytes
    entry = _CACHE.pop(key, None)
    if entry is None:
        return
    _cache_bytes -= key[0]
    left = _SIGS.get(key[:4], {})
    left[entry[2]] = left.get(entry[2], 1) - 1
    if left.get(entry[2], 0) <= 0:
        left.pop(entry[2], None)


def clear(trim=True):
    """drop every cached device twin (their HBM goes back to torch's allocator) and, with trim, the pinned pool's free blocks"""
    global _cache_bytes
    with _LOCK:
        _CACHE.clear()
        _SIGS.clear()
        _cache_bytes = 0
    if not trim:
        return
    try:
        _lib.lib().tf_host_pool_trim(0)
    except Exception:                     # noqa: BLE001 -- library not built: nothing to trim
        pass


def _sample_sig(addr, nbytes):
    """a signature of 8192 64-bit words spread evenly over a host buffer -- microseconds.  Equal content gives equal
    signatures, so a signature that no remembered twin of this shape has PROVES a miss: the full checksum pass (7 ms per GB)
    is then skipped and the checksum comes out of the upload's copying threads instead.  A matching signature proves nothing:
    the full checksum decides."""
    n64 = nbytes // 8
    if n64 == 0:
        return 0
    v = np.frombuffer((ctypes.c_char * (n64 * 8)).from_address(addr), dtype=np.uint64)
    return hash(v[::max(1, n64 // 8192)][:8192].tobytes())


def _remember(key, tensor, sig):
    """(called with the stream that wrote `tensor` current: the event recorded here is what a later user on another stream
    waits for)"""
    global _cache_bytes
    budget = _budget()
    nbytes = key[0]
    if budget <= 0 or nbytes > budget:
        return
    ev = _lib.torch().cuda.Event()
    ev.record()
    with _LOCK:
        if key in _CACHE:
            _CACHE.move_to_end(key)
            return
        _CACHE[key] = (tensor, ev, sig)
        _cache_bytes += nbytes
        by_sig = _SIGS.setdefault(key[:4], {})
        by_sig[sig] = by_sig.get(sig, 0) + 1
        while _cache_bytes > budget and len(_CACHE) > 1:
            _forget(next(iter(_CACHE)))


def _lookup(key):
    with _LOCK:
        entry = _CACHE.get(key)
        if entry is not None:
            _CACHE.move_to_end(key)
    if entry is None:
        return None
    tensor, ev, _ = entry
    cur = _lib.torch().cuda.current_stream()
    cur.wait_event(ev)                    # (no-op on the stream that produced it; a flood thread's stream waits for the DMA)
    tensor.record_stream(cur)             # the caching allocator must not recycle the block under this stream's kernels
    if _verify():
        # the twin must still hold the bytes whose checksum is its key: somebody wrote into a shared tensor, or a remembered
        # result was a view of scratch that has been overwritten since.  One pass over HBM and a stream synchronisation per hit
        h = np.zeros(2, np.uint64)
        with _lib.torch().cuda.device(tensor.device):
            _lib.check(_lib.lib().tf_hash_dev(_lib.ptr(tensor), key[0], h.ctypes.data_as(_lib._P), _lib.stream_ptr()), "tf_hash_dev")
        if (int(h[0]), int(h[1])) != key[4:6]:
            with _LOCK:
                if _CACHE.get(key) is entry:
                    _forget(key)
            raise RuntimeError("host cache: the device twin of a %s array of shape %s no longer holds the content it is "
                               "remembered by (written into in place, or a view of reused scratch): entry dropped"
                               % (np.dtype(key[1]).name, key[2]))
        stats["verified"] += 1
    return tensor


def _have_candidates(nbytes, dtype, shape, dev, sig):
    with _LOCK:
        return _SIGS.get((nbytes, dtype, shape, dev), {}).get(sig, 0) > 0


def _as_bytes_view(a):
    """C-contiguous array with a plain dtype -> (array to keep alive, address, nbytes, dtype tag)"""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    if a.dtype.byteorder == ">" or a.dtype.hasobject or a.dtype.kind not in "fiub":
        raise TypeError("unsupported array dtype %s" % a.dtype)
    return a, a.ctypes.data, a.nbytes, a.dtype.str


def _torch_dtype(np_dtype):
    t = _lib.torch()
    return {"f4": t.float32, "f8": t.float64, "i4": t.int32, "i8": t.int64, "u1": t.uint8, "i1": t.int8, "i2": t.int16,
            "f2": t.float16}.get(np.dtype(np_dtype).str.lstrip("<|=")[0:2])


def upload(array, fresh=False):
    """host array -> contiguous device tensor of the same dtype and shape on the current device / stream (module docstring).
    fresh=True: a private tensor the caller may write into (always uploaded; not remembered)."""
    t = _lib.torch()
    L = _lib.lib()
    dev = _lib.device()
    a, addr, nbytes, tag = _as_bytes_view(array)
    td = _torch_dtype(a.dtype)
    if td is None or nbytes == 0:          # exotic dtype / empty: torch's own path
        return t.from_numpy(a).to(dev)
    shape = tuple(a.shape)
    cacheable = (not fresh) and nbytes >= _MIN_CACHED and _budget() > 0
    h = np.zeros(2, np.uint64)
    hp = h.ctypes.data_as(_lib._P)
    known = False
    sig = _sample_sig(addr, nbytes) if cacheable else 0
    if cacheable and _have_candidates(nbytes, tag, shape, dev.index, sig):
        # a twin of this shape with this sample signature is remembered: a read-only pass over the host buffer (no PCIe) decides
        t0 = time.perf_counter()
        _lib.check(L.tf_hash_host(ctypes.c_void_p(addr), nbytes, hp), "tf_hash_host")
        stats["hash_s"] += time.perf_counter() - t0
        known = True
        hit = _lookup((nbytes, tag, shape, dev.index, int(h[0]), int(h[1])))
        if hit is not None:
            stats["hits"] += 1
            stats["hit_bytes"] += nbytes
            return hit
    out = t.empty(shape, dtype=td, device=dev)
    t0 = time.perf_counter()
    rc = L.tf_upload(_lib.ptr(out), ctypes.c_void_p(addr), nbytes, hp if (cacheable and not known) else None, _lib.stream_ptr())
    if rc == -3:
        # no pinned staging ring to be had on this system (TF_EHIP: neither hipHostRegister nor hipHostMalloc gave 256 MiB): the
        # runtime's own pageable copy moves the array -- slower, never wrong
        out.copy_(t.from_numpy(a))
        if cacheable and not known:
            _lib.check(L.tf_hash_host(ctypes.c_void_p(addr), nbytes, hp), "tf_hash_host")
    else:
        _lib.check(rc, "tf_upload")
    stats["upload_s"] += time.perf_counter() - t0
    stats["uploads"] += 1
    stats["upload_bytes"] += nbytes
    if cacheable:
        _remember((nbytes, tag, shape, dev.index, int(h[0]), int(h[1])), out, sig)
    return out


class _PinnedBlock:
    """a block of the library's pinned pool, exposed through the array interface: numpy arrays made from it keep it alive
    (`.base`), and the block goes back to the pool when the last of them is gone"""

    def __init__(self, nbytes, shape, typestr):
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().tf_host_alloc(int(max(nbytes, 1)), ctypes.byref(p)), "tf_host_alloc")
        self.ptr = p.value
        self.__array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                _lib.lib().tf_host_free(ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:                  # noqa: BLE001 -- interpreter shutdown
            pass


def empty_pinned(shape, dtype):
    """numpy array of the given shape / dtype in a pooled pinned block"""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    return np.asarray(_PinnedBlock(nbytes, tuple(int(s) for s in shape), dtype.str))


def download(tensor, remember=True):
    """device tensor -> numpy array in a pinned block (module docstring); CPU tensors are converted in place.
    remember=True ASSERTS OWNERSHIP: the tensor itself (not a copy) stays in the cache as the array's twin and is served to
    whoever presents the array's content again, so nobody may write into it afterwards.  That is true of a result this
    package computed and hands out only as the host array (_deliver); it is not true of a tensor a caller holds (to_host)."""
    t = _lib.torch()
    if not isinstance(tensor, t.Tensor):
        return np.asarray(tensor)
    if not tensor.is_cuda:
        return tensor.numpy()
    if tensor.dtype == t.bool:
        return download(tensor.to(t.uint8), remember=False).view(np.bool_)
    src = tensor.contiguous()
    np_dtype = {t.float32: np.float32, t.float64: np.float64, t.int32: np.int32, t.int64: np.int64, t.uint8: np.uint8,
                t.int8: np.int8, t.int16: np.int16, t.float16: np.float16}.get(src.dtype)
    nbytes = src.numel() * src.element_size()
    if np_dtype is None or nbytes < _MIN_CACHED:
        return src.cpu().numpy()
    L = _lib.lib()
    t0 = time.perf_counter()
    try:
        out = empty_pinned(tuple(src.shape), np_dtype)
    except MemoryError:                    # no pinned memory to be had: the runtime's pageable path
        return src.cpu().numpy()
    stats["pinned_alloc_s"] += time.perf_counter() - t0
    with t.cuda.device(src.device):
        t0 = time.perf_counter()
        _lib.check(L.tf_download(ctypes.c_void_p(out.ctypes.data), _lib.ptr(src), nbytes, _lib.stream_ptr()), "tf_download")
        stats["download_s"] += time.perf_counter() - t0      # (includes waiting for the kernels that produce the result)
        stats["downloads"] += 1
        stats["download_bytes"] += nbytes
        if remember and _budget() > 0:
            h = np.zeros(2, np.uint64)
            _lib.check(L.tf_hash_dev(_lib.ptr(src), nbytes, h.ctypes.data_as(_lib._P), _lib.stream_ptr()), "tf_hash_dev")
            _remember((nbytes, np.dtype(np_dtype).str, tuple(src.shape), src.device.index, int(h[0]), int(h[1])), src,
                      _sample_sig(out.ctypes.data, nbytes))
    return out


_COPY_STREAMS = {}


class Prefetch:
    """upload(a) for every array of `arrays` on a background thread and a copy stream of its own, while the calling thread goes
    on enqueuing kernels that do not need them: detect_cores starts on BT while WVD and SWD cross PCIe.  `get(i)` joins,
    makes the caller's current stream wait for the copies and returns the tensor."""

    def __init__(self, arrays):
        t = _lib.torch()
        self.dev = t.cuda.current_device()
        if self.dev not in _COPY_STREAMS:
            _COPY_STREAMS[self.dev] = t.cuda.Stream(device=self.dev)
        self.stream, self.out, self.err, self.ev = _COPY_STREAMS[self.dev], [None] * len(arrays), None, None
        self.thread = threading.Thread(target=self._run, args=(list(arrays),), name="tf-prefetch", daemon=True)
        self.thread.start()

    def _run(self, arrays):
        t = _lib.torch()
        try:
            t.cuda.set_device(self.dev)
            with t.cuda.stream(self.stream):
                for i, a in enumerate(arrays):
                    self.out[i] = upload(a)
                self.ev = t.cuda.Event()
                self.ev.record()
        except BaseException as exc:       # noqa: BLE001 -- re-raised by get() on the calling thread
            self.err = exc

    def get(self, i):
        self.thread.join()
        if self.err is not None:
            raise self.err
        cur = _lib.torch().cuda.current_stream()
        cur.wait_event(self.ev)
        self.out[i].record_stream(cur)
        return self.out[i]


def to_device(*fields):
    """The explicit form for a script that wants the device-resident path with ONE changed line: `bt, wvd, swd =
    tobac_flow_amd.to_device(bt, wvd, swd)` -- every field uploaded once, returned as detection.DeviceField (tensor + the
    `.t` time coordinate the recipes read; `a - b`, `a + b`, `-a` work on them) or, for an array without a time
    coordinate, as a plain device tensor.  Results of the entry points are then device tensors (`.cpu().numpy()` or
    tobac_flow_amd.to_host brings one back)."""
    from tobac_flow_amd.detection import DeviceField, _values
    out = []
    for f in fields:
        if isinstance(f, (DeviceField, _lib.torch().Tensor)):
            out.append(f)
            continue
        d = upload(_values(f))
        coord = getattr(f, "t", None)
        out.append(DeviceField(d, coord.values if hasattr(coord, "values") else coord) if coord is not None and not callable(coord) else d)
    return out[0] if len(out) == 1 else tuple(out)


def to_host(x):
    """device tensor / DeviceField -> numpy array (pinned block); anything else passes through np.asarray.  The tensor is the
    caller's, who may go on writing into it: it is NOT remembered as the array's twin (the array presented to an entry point
    later is uploaded like any other)."""
    inner = getattr(x, "data", None)
    if isinstance(inner, _lib.torch().Tensor) and not isinstance(x, _lib.torch().Tensor):
        x = inner
    return download(x, remember=False)
