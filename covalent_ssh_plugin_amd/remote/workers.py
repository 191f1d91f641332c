"""Dispatcher-side pool of persistent remote workers.

One warm worker process per GPU slot per endpoint (plus a small
round-robin set of CPU workers when no GPU policy is active), launched
over a long-lived transport channel and reused across electrons.  This
removes the per-electron python + HIP-runtime start the classic stub
pays (the reference architecture pays it per task by design —
/root/reference/covalent_ssh_plugin/ssh.py:377-383).

Module-level, keyed per endpoint: all executor instances targeting the
same host share workers, mirroring the transport pool and slot tables.
"""

from __future__ import annotations

import asyncio
import hashlib
import os
import struct
import threading
import weakref
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, Optional, Set, Tuple

import cloudpickle

from ..compat import app_log
from ..transport import native_io
from ..transport.channel import Channel, ChannelClosed, FrameParts

WorkerKey = Tuple[object, ...]


@dataclass
class WorkerHandle:
    channel: Channel
    startup_meta: dict
    key: WorkerKey
    #: content keys of the tensor arguments this worker is believed to hold
    #: in HBM (``cache_tensor_args``).  A new handle starts empty, so a
    #: worker that died or was respawned is assumed to hold nothing.
    resident: Set[str] = field(default_factory=set)
    #: for the packed arenas among them that were sent with
    #: ``patch_tensor_args`` on: key -> ``((segment_key, nbytes), ...)``, what
    #: a later arena of the same layout is compared with to send a delta.
    #: Maintained wherever ``resident`` is.  With ``rebase_tensor_args`` in
    #: order of use, the most recently stored or used arena last.
    resident_arenas: Dict[str, tuple] = field(default_factory=dict)
    #: ``retain_tensor_results``: the worker's names ("r:<op_id>:<index>") of
    #: the result buffers it is believed to hold as argument masters
    retained: Set[str] = field(default_factory=set)
    #: content key -> worker name, for the retained buffers whose bytes have
    #: been keyed: what the wire carries in place of the key
    names: Dict[str, str] = field(default_factory=dict)
    #: keying of retained buffers still running in the background; joined
    #: before a request to this worker is planned
    keying: list = field(default_factory=list)

    @property
    def alive(self) -> bool:
        return self.channel.alive


class WorkerStartupError(RuntimeError):
    pass


_workers: Dict[WorkerKey, WorkerHandle] = {}
_locks: Dict[WorkerKey, Tuple[asyncio.Lock, object]] = {}
_cpu_rr = 0  # round-robin cursor for CPU worker sets


def _lock_for(key: WorkerKey) -> asyncio.Lock:
    loop = asyncio.get_running_loop()
    entry = _locks.get(key)
    if entry is None or entry[1] is not loop:
        entry = (asyncio.Lock(), loop)
        _locks[key] = entry
    return entry[0]


def cpu_worker_index(pool_size: int) -> int:
    global _cpu_rr
    idx = _cpu_rr % max(1, pool_size)
    _cpu_rr += 1
    return idx


def pick_cpu_tag(pool_key, pool_size: int) -> str:
    """Pick a CPU worker tag: prefer an already-running IDLE worker
    (avoids head-of-line blocking behind a long task), else round-robin
    (which also spreads initial spawns across the set)."""
    candidates = [f"cpu{i}" for i in range(max(1, pool_size))]
    for tag in candidates:
        for key, handle in _workers.items():
            if len(key) >= 2 and key[0] == pool_key and key[1] == tag:
                if handle.alive and handle.channel.inflight == 0:
                    return tag
    return f"cpu{cpu_worker_index(pool_size)}"


async def get_worker(key: WorkerKey, launcher, startup_timeout: float = 180.0) -> WorkerHandle:
    """Return the live worker for ``key``, starting it with ``launcher``
    (an async callable returning a Channel) if needed."""
    loop = asyncio.get_running_loop()
    async with _lock_for(key):
        handle = _workers.get(key)
        if handle is not None and handle.alive and handle.channel.loop is loop:
            return handle
        if handle is not None and handle.channel.loop is not loop:
            # worker belongs to a closed event loop: reap it synchronously
            handle.channel.kill()
            _workers.pop(key, None)
        channel = await launcher()
        try:
            ready = await channel.recv_frame(timeout=startup_timeout)
        except (ChannelClosed, asyncio.TimeoutError) as e:
            await channel.close()
            raise WorkerStartupError(f"worker {key} failed to start: {e}") from e
        tag, meta = cloudpickle.loads(ready)
        if tag != "READY" or meta.get("error"):
            await channel.close()
            raise WorkerStartupError(
                f"worker {key} startup failed: {meta.get('error')}"
            )
        handle = WorkerHandle(channel=channel, startup_meta=meta, key=key)
        _workers[key] = handle
        return handle


# --- content identity of cached tensor arguments ----------------------------
#
# The (s0, s1) checksum is linear: adding +1, -2, +1 to three neighbouring
# words changes neither sum.  It guards the transfer, but it cannot say
# which bytes a cache entry holds; that is the job of a cryptographic digest.

ARG_CACHE_CHUNK = 8 << 20  # bytes per chunk digest and per checksum piece
_HASH_THREADS_MAX = 8
_hash_pool: Optional[ThreadPoolExecutor] = None
_hash_pool_lock = threading.Lock()


def hash_threads() -> int:
    return max(1, min(_HASH_THREADS_MAX, os.cpu_count() or 1))


def _pool() -> ThreadPoolExecutor:
    global _hash_pool
    with _hash_pool_lock:
        if _hash_pool is None:
            _hash_pool = ThreadPoolExecutor(
                max_workers=hash_threads(), thread_name_prefix="csp-hash"
            )
        return _hash_pool


def _chunks(nbytes: int, chunk_bytes: int):
    return [(off, min(chunk_bytes, nbytes - off)) for off in range(0, nbytes, chunk_bytes)]


def _map(fn, pieces, threads: Optional[int]):
    if len(pieces) <= 1 or threads == 1:
        return [fn(p) for p in pieces]
    if threads is None:
        return list(_pool().map(fn, pieces))
    with ThreadPoolExecutor(max_workers=threads) as pool:  # measurements only
        return list(pool.map(fn, pieces))


def content_key(buf, chunk_bytes: int = ARG_CACHE_CHUNK, threads: Optional[int] = None) -> str:
    """The cache identity of ``buf``'s bytes: the 16-byte blake2b digest, in
    hex, over the byte count (8 bytes, little endian) followed by the 16-byte
    blake2b digests of its ``chunk_bytes`` chunks in order.  The chunk
    digests are computed on a small thread pool (hashlib releases the GIL).
    The key covers bytes only: two tensors with equal bytes and another dtype
    or shape share it."""
    view = memoryview(buf).cast("B")
    nbytes = view.nbytes

    def digest(piece):
        off, n = piece
        return hashlib.blake2b(view[off : off + n], digest_size=16).digest()

    outer = hashlib.blake2b(struct.pack("<Q", nbytes), digest_size=16)
    for d in _map(digest, _chunks(nbytes, chunk_bytes), threads):
        outer.update(d)
    return outer.hexdigest()


def threaded_checksum(buf, chunk_bytes: int = ARG_CACHE_CHUNK, threads: Optional[int] = None):
    """``native_io.checksum(buf)``, bit for bit, composed from the sums of
    ``chunk_bytes`` pieces computed on the thread pool (ctypes releases the
    GIL).  For a piece that starts at word ``o``: ``s0 = sum s0_c`` and
    ``s1 = sum (s1_c + (o mod 2^32) * s0_c)`` modulo 2^64.  ``chunk_bytes``
    is a power of two that divides 16 GiB, so no piece crosses a 2^32-word
    boundary, where the weight wraps, and only the last piece can have a
    length that is no multiple of 4.  ``None`` when ``libcsp_io.so`` is not
    loaded."""
    if chunk_bytes < 4 or chunk_bytes & (chunk_bytes - 1) or chunk_bytes > (16 << 30):
        raise ValueError("chunk_bytes must be a power of two between 4 and 16 GiB")
    if native_io.load() is None:
        return None
    view = memoryview(buf).cast("B")
    pieces = _chunks(view.nbytes, chunk_bytes)
    if len(pieces) <= 1:
        return native_io.checksum(view)
    mask = (1 << 64) - 1
    s0 = s1 = 0
    sums = _map(lambda p: native_io.checksum(view, p[1], p[0]), pieces, threads)
    for (off, _n), (c0, c1) in zip(pieces, sums):
        s0 += c0
        s1 += c1 + ((off // 4) % (1 << 32)) * c0
    return s0 & mask, s1 & mask


_key_memo: Dict[int, tuple] = {}  # id(tensor) -> (weakref, guard, key)


def tensor_content_key(tensor, view, threads: Optional[int] = None) -> str:
    """:func:`content_key` of ``view``, the contiguous bytes of ``tensor``,
    remembered per tensor object for as long as it lives and its
    ``(data_ptr, nbytes, dtype, _version)`` stay the same: hashing is the
    largest dispatcher cost of a cache hit.  Memory changed behind torch's
    back leaves a stale key; the checksum, computed afresh on every dispatch
    and compared by the worker on every hit, then turns the hit into a miss."""
    guard = (tensor.data_ptr(), len(view), tensor.dtype, tensor._version)
    ident = id(tensor)
    memo = _key_memo.get(ident)
    if memo is not None and memo[0]() is tensor and memo[1] == guard:
        return memo[2]
    key = content_key(view, threads=threads)
    ref = weakref.ref(tensor, lambda _r, ident=ident: _key_memo.pop(ident, None))
    _key_memo[ident] = (ref, guard, key)
    return key


PACKED_MARKER = "__csp_packed_tensor_v1__"
PACKED_KEY_DOMAIN = b"csp-packed-v1"
PACK_ALIGN = 16  # csp_pack_dev's layout rule: every segment starts on a multiple
# A packed argument arena never exceeds this: every arena word index then
# stays far below 2^32, where the checksum's weight wraps, so
# compose_packed_checksum is exact.  A condition, not a measurement.
PACK_ARGS_MAX_BYTES = 4 << 30
#: rebase_tensor_args: how many of the most recently used resident arenas are
#: compared with a new one (bounds the planning cost; not a measurement)
REBASE_CANDIDATES = 8


def compose_packed_checksum(sums, offsets):
    """``native_io.checksum`` of a packed arena, from the checksums of its
    segments alone, so the dispatcher never materialises the arena.

    Segment ``k`` is tensor ``k``'s bytes at ``offsets[k]``, a multiple of
    16, followed by zeros up to the next multiple of 16.  Alone, its
    little-endian words ``w_i`` give ``s0_k = sum w_i`` and
    ``s1_k = sum w_i * (i + 1)``; a last word cut short is zero-extended
    there exactly as the arena's padding extends it.  In the arena word ``i``
    of segment ``k`` has the global index ``offsets[k] / 4 + i``, hence the
    weight ``offsets[k] / 4 + i + 1``, and contributes
    ``w_i * (i + 1) + (offsets[k] / 4) * w_i``.  Padding words are zero and
    contribute nothing.  Summed over the segment and then over all segments,
    modulo 2^64:

        s0 = sum s0_k
        s1 = sum (s1_k + (offsets[k] / 4) * s0_k)

    This needs every word index below 2^32 (the weight is taken modulo 2^32
    before the product): :data:`PACK_ARGS_MAX_BYTES` keeps it below 2^30."""
    mask = (1 << 64) - 1
    s0 = s1 = 0
    for (c0, c1), off in zip(sums, offsets):
        s0 += c0
        s1 += c1 + (off // 4) * c0
    return s0 & mask, s1 & mask


def packed_content_key(segment_keys) -> str:
    """The cache identity of a packed arena: blake2b over a domain tag and
    each segment's ``(content key, byte count)`` in order.  A key of keys:
    the per-tensor memo of :func:`tensor_content_key` makes a repeated set of
    the same tensor objects free to key."""
    outer = hashlib.blake2b(PACKED_KEY_DOMAIN, digest_size=16)
    for key, nbytes in segment_keys:
        outer.update(bytes.fromhex(key))
        outer.update(struct.pack("<Q", nbytes))
    return outer.hexdigest()


def _pack_small_args(args, kwargs, threshold, cache_min_bytes, pack_min_bytes,
                     buffers, buffer_meta, patch_max_fraction=None, rebase=False,
                     retain=False):
    """The ``pack_tensor_args`` half of :func:`extract_arg_buffers`: emit the
    packed entry when the rule in its docstring holds.  Returns
    ``{id(tensor): marker}``, empty when nothing is packed.  Only called with
    the option on, so the per-tensor path pays nothing for it.

    With ``patch_max_fraction`` (``patch_tensor_args``) a cached entry's
    ``"cache"`` also keeps, for the dispatcher alone (:class:`_ArgCacheSend`
    rebuilds ``"cache"`` for the wire), ``"segments"``: the per-segment
    ``(content key, nbytes)``, ``"seg_parts"``: per segment its parts of the
    frame (the tensor's own memory and its zero padding), and the
    fraction; with ``rebase`` (``rebase_tensor_args``) also ``"rebase":
    True``, and with ``retain`` (``retain_tensor_results``) ``"retain":
    True``."""
    import ctypes

    import torch

    packed_markers = {}
    found = {}

    def nbytes_of(t):
        return t.numel() * t.element_size()

    def collect(obj):
        if isinstance(obj, torch.Tensor):
            n = nbytes_of(obj)
            if (
                not obj.is_cuda
                and n < threshold
                and (cache_min_bytes is None or n < cache_min_bytes)
            ):
                found.setdefault(id(obj), obj)
        elif isinstance(obj, dict):
            for v in obj.values():
                collect(v)
        elif isinstance(obj, (tuple, list)):
            for v in obj:
                collect(v)

    collect(list(args))
    collect(dict(kwargs))
    tensors = list(found.values())
    if len(tensors) < 2:
        return packed_markers
    sizes = [nbytes_of(t) for t in tensors]
    offsets = []
    total = 0
    for n in sizes:
        offsets.append(total)
        total += (n + PACK_ALIGN - 1) // PACK_ALIGN * PACK_ALIGN
    if total < pack_min_bytes or total == 0 or total > PACK_ARGS_MAX_BYTES:
        return packed_markers
    srcs = [t.contiguous() for t in tensors]
    parts = []
    views = []
    seg_parts = []
    for src_t, n in zip(srcs, sizes):
        view = (ctypes.c_char * n).from_address(src_t.data_ptr()) if n else b""
        views.append(view)
        parts.append(view)
        seg_parts.append([view])
        if n % PACK_ALIGN:
            parts.append(bytes(PACK_ALIGN - n % PACK_ALIGN))
            seg_parts[-1].append(parts[-1])
    info = {
        "device": True,
        "packed": [
            {"dtype": str(s.dtype).replace("torch.", ""), "shape": list(s.shape),
             "offset": off, "nbytes": n}
            for s, off, n in zip(srcs, offsets, sizes)
        ],
        "nbytes": total,
    }
    # looked up at call time: None when libcsp_io.so is not loaded
    sums = [native_io.checksum(v) if n else (0, 0) for v, n in zip(views, sizes)]
    if all(s is not None for s in sums):
        s0, s1 = compose_packed_checksum(sums, offsets)
        info["sum"] = [int(s0), int(s1)]
        if cache_min_bytes is not None and total >= max(1, cache_min_bytes):
            segment_keys = tuple(
                (tensor_content_key(t, v), n)
                for t, v, n in zip(tensors, views, sizes)
            )
            info["cache"] = {"key": packed_content_key(segment_keys)}
            if patch_max_fraction is not None:
                info["cache"].update(
                    segments=segment_keys, seg_parts=seg_parts,
                    patch_max_fraction=float(patch_max_fraction),
                )
                if rebase:
                    info["cache"]["rebase"] = True
                if retain:
                    info["cache"]["retain"] = True
    # the source tensors stay alive until the frame is drained
    buffers.append((FrameParts(parts), srcs))
    buffer_meta.append(info)
    index = len(buffers) - 1
    for j, t in enumerate(tensors):
        packed_markers[id(t)] = (PACKED_MARKER, index, j)
    return packed_markers


def extract_arg_buffers(
    args, kwargs, threshold: int, to_device: bool = False,
    cache_min_bytes: Optional[int] = None,
    pack_min_bytes: Optional[int] = None,
    patch_max_fraction: Optional[float] = None,
    rebase: bool = False,
    retain: bool = False,
):
    """Pull large contiguous CPU torch tensors out of (args, kwargs) and
    replace them with out-of-band buffer markers (the request-direction
    mirror of the worker's result staging).  Returns
    (new_args, new_kwargs, buffer_meta, buffers); no-op (and no torch
    import) unless torch is already loaded in the dispatcher.

    ``cache_min_bytes`` (the executor's ``cache_tensor_args``; ``None`` is
    off) with ``to_device``: a tensor of at least that many bytes also
    carries ``"cache": {"key": <hex>}``, its :func:`content_key`, and its
    checksum comes from :func:`threaded_checksum`.  :func:`run_task` decides
    per worker whether the bytes or only the key travel.  Without
    ``libcsp_io.so`` there is no checksum and so no cache entry: a hit could
    not be verified.

    ``to_device`` (the executor's ``device_tensor_args``): EVERY CPU tensor
    is extracted whatever its size, so an electron never gets a mix of CPU
    and CUDA tensors that depends on a threshold.  Each meta entry is
    marked ``"device": True`` (the worker lands it in HBM) and, when the
    native I/O library is loaded, carries ``"sum": [s0, s1]``, the checksum
    of the contiguous bytes that will be sent (the worker recomputes it on
    the GPU and compares).

    ``pack_min_bytes`` (the executor's ``pack_tensor_args``; ``None`` is off)
    with ``to_device``: the CPU tensors below ``threshold`` (and, with the
    cache on, below ``cache_min_bytes``: a tensor at or above it keeps its
    own key and master) travel as ONE frame when at least two distinct
    tensor objects qualify and their arena (each tensor at the next multiple
    of 16 bytes, ``csp_pack_dev``'s layout) is at least ``pack_min_bytes``
    and at most :data:`PACK_ARGS_MAX_BYTES`.  The entry is ``{"device": True,
    "packed": [{dtype, shape, offset, nbytes}, ...], "nbytes": total,
    "sum": [s0, s1]}``, its buffer a :class:`FrameParts` over the tensors'
    own memory and the zero padding (no host arena), its checksum composed by
    :func:`compose_packed_checksum`, and each tensor becomes
    ``("__csp_packed_tensor_v1__", i, j)``: one tensor object met twice is
    one segment and one marker.  With the cache on and
    ``total >= cache_min_bytes`` the entry carries ``"cache": {"key"}`` from
    :func:`packed_content_key`.  Otherwise every tensor takes the per-tensor
    path, exactly as without the option.

    ``patch_max_fraction`` (the executor's ``patch_tensor_args`` and
    ``patch_args_max_fraction``; ``None`` is off): a cached packed entry also
    keeps its per-segment keys and parts on the dispatcher side, so that
    :func:`run_task` can send it as a delta against an arena of the same
    layout that the worker holds (:class:`_ArgCacheSend`).  Nothing of it
    reaches the wire.

    ``rebase`` (the executor's ``rebase_tensor_args``, with
    ``patch_max_fraction``): such an entry is instead planned against ANY
    arena the worker holds, whatever its layout, and built there as a new
    master that leaves the base in the cache (:meth:`_ArgCacheSend._plan_rebase`).

    ``retain`` (the executor's ``retain_tensor_results``, with ``rebase``):
    such an entry may also be rebased with an EMPTY delta, the case of a
    subset or a reordering of what a retained result arena holds."""
    import sys

    if "torch" not in sys.modules:
        return args, kwargs, [], []
    import ctypes

    import torch

    buffer_meta = []
    buffers = []
    packed_markers = None  # id(tensor) -> marker, with pack_tensor_args
    if to_device and pack_min_bytes is not None:
        packed_markers = _pack_small_args(
            args, kwargs, threshold, cache_min_bytes, pack_min_bytes, buffers, buffer_meta,
            patch_max_fraction=patch_max_fraction, rebase=rebase, retain=retain,
        )

    def extract(t):
        if packed_markers and id(t) in packed_markers:
            return packed_markers[id(t)]
        src_t = t.contiguous()
        nbytes = src_t.numel() * src_t.element_size()
        view = (ctypes.c_char * nbytes).from_address(src_t.data_ptr())
        buffers.append((view, src_t))  # keep tensor alive until sent
        info = {"dtype": str(src_t.dtype).replace("torch.", ""), "shape": list(src_t.shape)}
        if to_device:
            info["device"] = True
            cacheable = cache_min_bytes is not None and nbytes >= max(1, cache_min_bytes)
            # looked up at call time: None when libcsp_io.so is not loaded
            sums = threaded_checksum(view) if cacheable else native_io.checksum(view)
            if sums is not None:
                info["sum"] = [int(sums[0]), int(sums[1])]
                if cacheable:
                    info["cache"] = {"key": tensor_content_key(t, view)}
        buffer_meta.append(info)
        return ("__csp_tensor_buffer_v1__", len(buffers) - 1)

    def walk(obj):
        if isinstance(obj, torch.Tensor):
            if not obj.is_cuda and (
                to_device or obj.numel() * obj.element_size() >= threshold
            ):
                return extract(obj)
            return obj
        if isinstance(obj, dict):
            return {k: walk(v) for k, v in obj.items()}
        if isinstance(obj, tuple):
            vals = [walk(v) for v in obj]
            return type(obj)(*vals) if hasattr(obj, "_fields") else tuple(vals)
        if isinstance(obj, list):
            return [walk(v) for v in obj]
        return obj

    new_args = walk(list(args))
    new_kwargs = walk(dict(kwargs))
    return new_args, new_kwargs, buffer_meta, buffers


def verify_result_buffers(buffer_meta, buffers) -> int:
    """Check every received result buffer whose meta entry carries
    ``"sum": [s0, s1]`` (the worker's on-GPU checksum of the bytes it sent)
    against ``native_io.checksum`` of the bytes that arrived.  Returns how
    many were checked: 0 when ``libcsp_io.so`` is not loaded, as on the
    argument side.  A mismatch raises ``RuntimeError``; the frames have all
    been consumed by then, so the channel stays usable."""
    verified = 0
    for i, info in enumerate(buffer_meta):
        if "sum" not in info or i >= len(buffers):
            continue
        # looked up at call time: None when libcsp_io.so is not loaded.  A
        # retained buffer may be a whole large tensor: the same two numbers,
        # from pieces summed on the thread pool
        if "retained" in info:
            sums = threaded_checksum(buffers[i])
        else:
            sums = native_io.checksum(buffers[i])
        if sums is None:
            continue
        verified += 1
        got = [int(sums[0]), int(sums[1])]
        want = [int(info["sum"][0]), int(info["sum"][1])]
        if got != want:
            raise RuntimeError(
                f"result buffer {i} failed its integrity check: the worker "
                f"sent checksum {want}, the {memoryview(buffers[i]).nbytes} "
                f"bytes received give {got}"
            )
    return verified


def _reconstruct(result, buffer_meta, buffers, rebuilt_out=None):
    """Replace out-of-band tensor-buffer markers with rebuilt torch
    tensors (workers ship large tensors as raw frames; see
    remote/worker_template.py protocol note).  ``rebuilt_out`` (a dict,
    ``retain_tensor_results``) gets the rebuilt tensors: ``i -> tensor`` for a
    tensor buffer, ``(i, j) -> tensor`` for segment ``j`` of a packed one.

    A packed marker ``("__csp_packed_tensor_v1__", i, j)`` becomes tensor
    ``j`` of buffer ``i``: a zero-copy ``torch.frombuffer`` view at its
    ``offset`` into the received buffer.  All tensors of one packed buffer
    share that buffer, which stays alive as long as any of them does (so one
    small survivor keeps the whole frame in memory; ``clone()`` it to let
    go).  Their byte ranges do not overlap.  A marker met twice gives the
    same tensor object, as the worker had it."""
    import torch

    writable = {}  # buffer index -> the one writable object its views share
    rebuilt = {}  # (i, j) -> tensor

    def shared(i: int):
        if i not in writable:
            raw = buffers[i]
            writable[i] = bytearray(raw) if isinstance(raw, bytes) else raw
        return writable[i]

    def build_packed(i: int, j: int):
        if (i, j) not in rebuilt:
            info = buffer_meta[i]["packed"][j]
            dtype = getattr(torch, info["dtype"])
            count = 1
            for dim in info["shape"]:
                count *= int(dim)
            if count == 0:
                t = torch.empty(info["shape"], dtype=dtype)
            else:
                t = torch.frombuffer(
                    shared(i), dtype=dtype, count=count, offset=int(info["offset"])
                ).reshape(info["shape"])
            rebuilt[(i, j)] = t
        return rebuilt[(i, j)]

    def build(i: int):
        info = buffer_meta[i]
        dtype = getattr(torch, info["dtype"])
        raw = buffers[i]
        # large frames arrive in a preallocated writable buffer (zero-copy
        # here); small ones as bytes (copy once into writable memory)
        data = bytearray(raw) if isinstance(raw, bytes) else raw
        t = torch.frombuffer(data, dtype=dtype).reshape(info["shape"])
        if rebuilt_out is not None:
            rebuilt_out[i] = t
        return t

    def walk(obj):
        if (
            isinstance(obj, tuple)
            and len(obj) == 2
            and obj[0] == "__csp_tensor_buffer_v1__"
        ):
            return build(obj[1])
        if (
            isinstance(obj, tuple)
            and len(obj) == 3
            and isinstance(obj[0], str)
            and obj[0] == "__csp_packed_tensor_v1__"
        ):
            return build_packed(obj[1], obj[2])
        if isinstance(obj, dict):
            return {k: walk(v) for k, v in obj.items()}
        if isinstance(obj, tuple):
            vals = [walk(v) for v in obj]
            return type(obj)(*vals) if hasattr(obj, "_fields") else tuple(vals)
        if isinstance(obj, list):
            return [walk(v) for v in obj]
        return obj

    out = walk(result)
    if rebuilt_out is not None:
        rebuilt_out.update(rebuilt)
    return out


# --- CUDA results kept in worker HBM (retain_tensor_results) ----------------
#
# The worker names a result buffer it keeps ("r:<op_id>:<index>", never a
# 32-hex content key).  The dispatcher addresses cached arguments by content,
# so that a result that went through other hands (a deep copy, covalent's own
# serialisation) still hits: it keys the bytes it received, in the background,
# and remembers which name holds them.


def _forget_key(handle: WorkerHandle, key: str) -> None:
    """``key``, a content key, is no longer believed held."""
    handle.resident.discard(key)
    handle.resident_arenas.pop(key, None)
    # _ArgCacheSend is also driven with handle-like objects that carry the
    # two resident tables alone
    names = getattr(handle, "names", None)
    name = names.pop(key, None) if names else None
    if name is not None:
        handle.retained.discard(name)


def _forget_name(handle: WorkerHandle, name: str) -> None:
    """``name``, a worker name, is no longer believed held (whether or not
    its bytes have been keyed yet)."""
    handle.retained.discard(name)
    for key in [k for k, n in handle.names.items() if n == name]:
        _forget_key(handle, key)


def _tensor_view(t):
    import ctypes

    nbytes = t.numel() * t.element_size()
    return (ctypes.c_char * nbytes).from_address(t.data_ptr()) if nbytes else b""


def _key_retained(items):
    """Runs on a thread: the content keys of retained buffers, computed as
    :func:`extract_arg_buffers` will compute them for the same tensors (so the
    per-tensor memo is seeded).  ``items``: ``(name, tensor)`` for a tensor
    buffer, ``(name, [tensor, ...])`` for a packed one.  Returns ``[(name,
    key, segments or None)]``.

    The caller already owns these tensors.  One that torch changed in place
    while it was hashed (its ``_version`` moved) would be registered under a
    key of bytes that the worker's master does not hold, and only the linear
    checksum on the reference would stand between that and a wrong hit: such a
    buffer is left out, and is then simply never hit."""
    out = []
    for name, what in items:
        tensors = what if isinstance(what, list) else [what]
        before = [t._version for t in tensors]
        if isinstance(what, list):
            # one segment per pool thread, each hashed on that thread alone
            # (a pool task that waited for pool tasks could starve the pool)
            pairs = [(t, _tensor_view(t)) for t in what]
            keys = _map(lambda p: tensor_content_key(p[0], p[1], threads=1), pairs, None)
            segments = tuple((key, len(view)) for key, (_t, view) in zip(keys, pairs))
            keyed = (name, packed_content_key(segments), segments)
        else:
            keyed = (name, tensor_content_key(what, _tensor_view(what)), None)
        if [t._version for t in tensors] == before:
            out.append(keyed)
    return out


async def _register_retained(handle: WorkerHandle, items, keep_segments: bool):
    """Key ``items`` off the event loop (the chunk digests run on the hash
    pool) and, for every name the worker is still believed to hold, make its
    bytes addressable by content."""
    loop = asyncio.get_running_loop()
    try:
        keyed = await loop.run_in_executor(None, _key_retained, items)
    except Exception:  # noqa: BLE001 - an unkeyed result is only never hit
        app_log.debug("keying a retained result failed", exc_info=True)
        return
    for name, key, segments in keyed:
        if name not in handle.retained:
            continue  # reported evicted, or forgotten, in the meantime
        stale = handle.names.get(key)
        if stale is not None and stale != name:
            handle.retained.discard(stale)  # the same bytes, held twice
        handle.names[key] = name
        handle.resident.add(key)
        if segments is not None and keep_segments:
            handle.resident_arenas.pop(key, None)  # most recent: last
            handle.resident_arenas[key] = segments


def retain_results(handle: WorkerHandle, meta, rebuilt, keep_segments: bool,
                   stats: Optional[dict] = None) -> None:
    """After a verified reply: forget what the worker's retention pushed out
    (``meta["retained"]["evicted"]``, so that it costs a plain store later,
    not a miss and a resend), then note every buffer the reply marks
    ``"retained"`` and start keying it in the background."""
    report = meta.get("retained") or {}
    for gone in report.get("evicted") or ():
        if gone in handle.retained:
            _forget_name(handle, gone)
        else:
            _forget_key(handle, gone)
    items = []
    for i, info in enumerate(meta.get("buffers") or ()):
        name = info.get("retained")
        if name is None:
            continue
        if "packed" in info:
            tensors = [rebuilt.get((i, j)) for j in range(len(info["packed"]))]
            if any(t is None for t in tensors):
                continue  # a segment nobody rebuilt: cannot be keyed as B will
            nbytes = int(info["nbytes"])
            items.append((name, tensors))
        else:
            t = rebuilt.get(i)
            if t is None:
                continue
            nbytes = t.numel() * t.element_size()
            items.append((name, t))
        _forget_name(handle, name)  # an op_id used twice: other bytes now
        handle.retained.add(name)
        if stats is not None:
            stats["results_retained"] = stats.get("results_retained", 0) + 1
            stats["results_retained_bytes"] = (
                stats.get("results_retained_bytes", 0) + nbytes
            )
    if items:
        handle.keying[:] = [task for task in handle.keying if not task.done()]
        handle.keying.append(
            asyncio.ensure_future(_register_retained(handle, items, keep_segments))
        )


async def join_retained_keying(handle: Optional[WorkerHandle] = None) -> None:
    """Wait for the background keying of retained results: of ``handle``, or
    of every worker of the running loop.  Afterwards their bytes are
    addressable by content and the per-tensor key memo is seeded."""
    loop = asyncio.get_running_loop()
    handles = [handle] if handle is not None else list(_workers.values())
    for h in handles:
        pending = [t for t in h.keying if not t.done() and t.get_loop() is loop]
        h.keying[:] = pending
        if pending:
            await asyncio.gather(*pending, return_exceptions=True)
            h.keying[:] = [t for t in h.keying if not t.done()]


def _view_nbytes(view) -> int:
    """Bytes of one argument frame: a buffer, or the parts of a packed one."""
    return view.nbytes if isinstance(view, FrameParts) else memoryview(view).nbytes


class _ArgCacheSend:
    """The ``cache_tensor_args`` side of one :func:`run_task`: which cached
    entries travel as a reference, decided while the request is being sent,
    and what the worker's report means for ``handle.resident``."""

    def __init__(self, handle, base, entries, views, cache_stats):
        self.handle = handle
        self.base = base
        self.entries = entries
        self.views = views
        self.cache_stats = cache_stats
        self.keys = [(info.get("cache") or {}).get("key") for info in entries]
        self.refs = [False] * len(entries)
        #: per entry ``(base key, changed segment indices, delta FrameParts)``
        #: when the last :meth:`frames` sent it as a patch, else None
        self.patches = [None] * len(entries)
        #: per entry ``(base key, base arena bytes, per-segment base offset or
        #: -1, delta FrameParts)`` when the last :meth:`frames` sent it as a
        #: rebase, else None
        self.rebases = [None] * len(entries)
        #: worker name -> content key, for every name the last :meth:`frames`
        #: put on the wire in place of a key (``retain_tensor_results``)
        self.sent_as = {}

    def _wire(self, key):
        """What the worker holds ``key``'s bytes under: its own name for a
        retained result, else the key."""
        names = getattr(self.handle, "names", None)  # see _forget_key
        name = names.get(key) if names else None
        if name is None:
            return key
        self.sent_as[name] = key
        return name

    def _plan_patch(self, cache):
        """``patch_tensor_args``: the delta that turns an arena the worker
        holds into this one, or None.  Among the resident arenas with the
        same byte counts in the same order, the one with the fewest changed
        rounded bytes; a patch only when they are more than none and at most
        ``patch_max_fraction`` of the arena."""
        segments = cache["segments"]
        sizes = [n for _key, n in segments]
        best = None
        for base, held in self.handle.resident_arenas.items():
            if base not in self.handle.resident or len(held) != len(segments):
                continue
            if any(n != m for n, (_key, m) in zip(sizes, held)):
                continue
            changed = [j for j, (new, old) in enumerate(zip(segments, held)) if new[0] != old[0]]
            nbytes = sum(-(-sizes[j] // PACK_ALIGN) * PACK_ALIGN for j in changed)
            if best is None or nbytes < best[0]:
                best = (nbytes, base, changed)
        if best is None:
            return None
        nbytes, base, changed = best
        total = sum(-(-n // PACK_ALIGN) * PACK_ALIGN for n in sizes)
        if not 0 < nbytes <= cache["patch_max_fraction"] * total:
            return None
        # cut from the tensors' own memory and the zero padding: no host copy
        delta = FrameParts([p for j in changed for p in cache["seg_parts"][j]])
        return base, changed, delta

    def _plan_rebase(self, cache):
        """``rebase_tensor_args``: the held arena and the delta that this
        arena is built from on the worker, or None.  Candidates are the
        resident arenas, the :data:`REBASE_CANDIDATES` most recently stored
        or used (a bound on the planning cost, not a measurement).  A segment
        is reusable when the candidate holds one with the same ``(content
        key, nbytes)``, wherever it lies; duplicates share one source.  The
        candidate that leaves the fewest rounded delta bytes wins, a tie goes
        to the most recent; a rebase only when they are more than none and at
        most ``patch_max_fraction`` of the arena.  With ``retain_tensor_results``
        (``cache["retain"]``) none is enough: a subset or a reordering of a
        held arena travels as an empty delta."""
        segments = cache["segments"]
        arenas = self.handle.resident_arenas
        recent = [k for k in reversed(list(arenas)) if k in self.handle.resident]
        best = None
        for base in recent[:REBASE_CANDIDATES]:
            where = {}
            offset = 0
            for seg in arenas[base]:
                where.setdefault(tuple(seg), offset)
                offset += -(-seg[1] // PACK_ALIGN) * PACK_ALIGN
            sources = [where.get(tuple(seg), -1) for seg in segments]
            nbytes = sum(
                -(-seg[1] // PACK_ALIGN) * PACK_ALIGN
                for seg, src in zip(segments, sources) if src < 0
            )
            if best is None or nbytes < best[0]:
                best = (nbytes, base, offset, sources)
        if best is None:
            return None
        nbytes, base, base_nbytes, sources = best
        total = sum(-(-n // PACK_ALIGN) * PACK_ALIGN for _key, n in segments)
        if nbytes == 0 and not cache.get("retain"):
            return None
        if not 0 <= nbytes <= cache["patch_max_fraction"] * total:
            return None
        # cut from the tensors' own memory and the zero padding: no host copy
        delta = FrameParts(
            [p for j, src in enumerate(sources) if src < 0 for p in cache["seg_parts"][j]]
        )
        return base, base_nbytes, sources, delta

    def _touch(self, key):
        """``rebase_tensor_args``: ``key`` was used, so it is the most recent
        of ``resident_arenas``."""
        arenas = self.handle.resident_arenas
        if key in arenas:
            arenas[key] = arenas.pop(key)

    def _now_resident(self, index, key):
        """``key``'s frame has been written: the worker holds it from here on
        as far as later requests on this channel are concerned."""
        self.handle.resident.add(key)
        cache = self.entries[index].get("cache") or {}
        segments = cache.get("segments")
        if segments is not None:
            if cache.get("rebase"):
                self.handle.resident_arenas.pop(key, None)  # most recent: last
            self.handle.resident_arenas[key] = segments

    def _forget(self, key):
        _forget_key(self.handle, key)

    def frames(self, full: bool):
        """The request's frames.  A generator: the channel runs it frame by
        frame under its write lock, so the decisions are taken in send
        order.  ``full``: no references and no patches, every entry with its
        frame."""
        resident = self.handle.resident
        self.refs = [
            key is not None and not full and key in resident for key in self.keys
        ]
        self.patches = [None] * len(self.entries)
        self.rebases = [None] * len(self.entries)
        self.sent_as = {}
        wire = []
        for index, (info, key, ref) in enumerate(zip(self.entries, self.keys, self.refs)):
            if key is not None:
                cache = info["cache"]
                info = dict(info)
                if ref and cache.get("rebase"):
                    self._touch(key)
                if not ref and not full and cache.get("segments") is not None:
                    if cache.get("rebase"):
                        self.rebases[index] = self._plan_rebase(cache)
                    else:
                        self.patches[index] = self._plan_patch(cache)
                patch = self.patches[index]
                rebase = self.rebases[index]
                if rebase is not None:
                    info["cache"] = {
                        "key": key,
                        "rebase": {"base": self._wire(rebase[0]), "base_nbytes": rebase[1],
                                   "sources": rebase[2]},
                    }
                    info["rebase_nbytes"] = rebase[3].nbytes
                elif patch is not None:
                    info["cache"] = {
                        "key": key,
                        "patch": {"base": self._wire(patch[0]), "segments": patch[1]},
                    }
                    info["patch_nbytes"] = patch[2].nbytes
                else:
                    info["cache"] = (
                        {"key": self._wire(key), "ref": True} if ref
                        else {"key": key, "store": True}
                    )
            wire.append(info)
        yield cloudpickle.dumps(dict(self.base, arg_buffers=wire))
        for index, (view, key, ref) in enumerate(zip(self.views, self.keys, self.refs)):
            if ref:
                continue
            patch = self.patches[index]
            rebase = self.rebases[index]
            if rebase is not None:
                yield rebase[3]
                self._touch(rebase[0])  # the base stays, and was used
            else:
                yield view if patch is None else patch[2]
            if patch is not None:
                self._forget(patch[0])  # patched in place: the base is gone
            if key is not None:
                self._now_resident(index, key)  # its frame has been written

    def reconcile(self, meta) -> bool:
        """Bring ``handle.resident`` in line with the worker's report and
        count; returns whether the worker missed a reference or the base of
        a patch."""
        report = meta.get("arg_cache") or {}
        back = self.sent_as  # the worker reports what it was sent: names
        held = {
            back.get(k, k)
            for k in list(report.get("stored") or ()) + list(report.get("hits") or ())
        }
        for key in self.keys:
            if key is not None and key not in held:
                self._forget(key)
        missed = [i for i in (report.get("miss") or ()) if 0 <= i < len(self.keys)]
        for i in missed:
            if self.patches[i] is not None:
                # a failed patch in place: the worker let the base go
                self._forget(self.patches[i][0])
            if self.rebases[i] is not None:
                # nobody can tell whether the base or the delta was wrong
                self._forget(self.rebases[i][0])
        done = {(back.get(b, b), n) for b, n in (report.get("patched") or ())}
        stats = self.cache_stats
        if stats is not None:
            for view, key, patch in zip(self.views, self.keys, self.patches):
                if patch is not None and (patch[0], key) in done:
                    stats["arg_cache_patches"] = stats.get("arg_cache_patches", 0) + 1
                    stats["arg_cache_bytes_saved"] = (
                        stats.get("arg_cache_bytes_saved", 0)
                        + _view_nbytes(view) - patch[2].nbytes
                    )
            rebased = {(back.get(b, b), n) for b, n in (report.get("rebased") or ())}
            for view, key, rebase in zip(self.views, self.keys, self.rebases):
                if rebase is not None and (rebase[0], key) in rebased:
                    stats["arg_cache_rebases"] = stats.get("arg_cache_rebases", 0) + 1
                    stats["arg_cache_bytes_saved"] = (
                        stats.get("arg_cache_bytes_saved", 0)
                        + _view_nbytes(view) - rebase[3].nbytes
                    )
            for view, key, ref in zip(self.views, self.keys, self.refs):
                if ref and key in held:
                    stats["arg_cache_hits"] = stats.get("arg_cache_hits", 0) + 1
                    stats["arg_cache_bytes_saved"] = (
                        stats.get("arg_cache_bytes_saved", 0) + _view_nbytes(view)
                    )
            stats["arg_cache_misses"] = stats.get("arg_cache_misses", 0) + len(missed)
        return bool(missed)


async def run_task(
    handle: WorkerHandle,
    op_id: str,
    workdir: str,
    function_blob: bytes,
    timeout: Optional[float] = None,
    arg_buffer_meta=None,
    arg_buffers=None,
    ack_state: Optional[dict] = None,
    cache_stats: Optional[dict] = None,
    retain_segments: bool = False,
):
    """One electron through a worker.  Returns (result, exception, meta).

    ``ack_state`` (a mutable dict) gets ``{"started": True}`` the moment
    the worker's A1 ack arrives — i.e. once user code may have begun.
    On ChannelClosed the caller reads it to decide whether a retry could
    re-execute a partially-run task.

    Result buffers whose meta carries a checksum are verified before any
    tensor is rebuilt (:func:`verify_result_buffers`); the count goes to
    ``meta["result_integrity"]``.  A mismatch raises ``RuntimeError``.

    Argument entries that carry ``"cache": {"key"}`` (``cache_tensor_args``)
    are decided while the request is being sent, under the channel's write
    lock and so in send order: a key in ``handle.resident`` travels as
    ``{"key", "ref": true}`` with no frame, any other as
    ``{"key", "store": true}`` with its frame, and is resident from the
    moment that frame has been written, so electrons queued behind it on
    this worker already refer to it.  The worker's ``meta["arg_cache"]``
    reconciles the set.  When it reports a miss, user code has not run: the
    task is sent once more with full frames.  ``cache_stats`` (a mutable
    dict, the executor's counters) gets ``arg_cache_hits``,
    ``arg_cache_misses`` and ``arg_cache_bytes_saved``.

    A packed entry that keeps its per-segment keys (``patch_tensor_args``)
    and whose key is not resident is compared, in the same place, with the
    arenas of the same layout in ``handle.resident_arenas``: when at most
    ``patch_max_fraction`` of its bytes differ from one of them it travels
    as ``{"key", "patch": {"base", "segments"}}`` with a frame of only the
    changed segments, the worker patches the held arena in place, and from
    the moment that frame has been written the base is no longer resident
    and the new key is.  A missing base is a miss like a missing reference;
    the resend never patches.  ``cache_stats`` also gets
    ``arg_cache_patches``, and ``arg_cache_bytes_saved`` grows by the arena
    bytes that the delta left out.

    With ``rebase_tensor_args`` such an entry is instead compared with the
    most recently used resident arenas of ANY layout
    (:meth:`_ArgCacheSend._plan_rebase`) and travels as ``{"key", "rebase":
    {"base", "base_nbytes", "sources"}}`` with a frame of only the segments
    the base lacks.  The worker builds a new master and keeps the base, so
    once that frame has been written both keys are resident.  A miss on a
    rebase forgets both; the new key in ``not_stored`` forgets it alone; the
    resend never rebases.  ``cache_stats`` gets ``arg_cache_rebases``.

    A verified reply whose buffers carry ``"retained"`` (the worker's
    ``retain_tensor_results``) is noted in ``handle.retained`` and keyed in
    the background (:func:`retain_results`); the result is handed back without
    waiting for the hash.  Every request waits for this handle's keying before
    it is planned, so :class:`_ArgCacheSend` sees finished names, and puts the
    worker's name on the wire wherever it names something held: a ``ref``
    key, the base of a patch, the base of a rebase.  ``retain_segments`` (the
    executor's ``patch_tensor_args``): a retained arena also becomes a base
    for patches and rebases.  ``cache_stats`` gets ``results_retained`` and
    ``results_retained_bytes``.
    """
    if handle.keying:
        await join_retained_keying(handle)
    entries = arg_buffer_meta or []
    cache = None
    if entries and any("cache" in info for info in entries):
        cache = _ArgCacheSend(
            handle,
            {"op_id": op_id, "workdir": workdir, "function_blob": function_blob},
            entries,
            [view for view, _keep in (arg_buffers or [])],
            cache_stats,
        )
    else:
        request = cloudpickle.dumps(
            {
                "op_id": op_id,
                "workdir": workdir,
                "function_blob": function_blob,
                "arg_buffers": entries,
            }
        )
        frames = [request] + [view for view, _keep in (arg_buffers or [])]
    parsed = {}

    def reply_frames(main: bytes):
        decoded = cloudpickle.loads(main)
        if decoded[0] == "A1":
            if ack_state is not None:
                ack_state["started"] = True
            return None  # control frame: the R1 reply follows
        tag, result_blob, meta, nbuf = decoded
        assert tag == "R1", f"unexpected worker response tag {tag!r}"
        parsed["value"] = (result_blob, meta, nbuf)
        return nbuf

    resent = False
    while True:
        # pipelined: the channel's write lock is held only while sending, so
        # queued electrons on one worker overlap their wire round trips
        _main, buffers = await handle.channel.exchange(
            frames if cache is None else cache.frames(full=resent),
            reply_frames,
            timeout=timeout,
        )
        assert "value" in parsed, "worker reply ended at the ack frame"
        result_blob, meta, nbuf = parsed.pop("value")
        if cache is None:
            break
        missed = cache.reconcile(meta)
        if resent:
            meta.setdefault("arg_cache", {})["resent"] = True
        if resent or not missed:
            break
        # the worker no longer holds what a reference named.  It ran no user
        # code, so the task goes once more, every argument with its frame
        resent = True
        if ack_state is not None:
            ack_state["started"] = False
    buffer_meta = meta.get("buffers", [])
    if nbuf and any("sum" in info for info in buffer_meta):
        meta["result_integrity"] = {
            "verified": verify_result_buffers(buffer_meta, buffers)
        }
    result, exception = cloudpickle.loads(result_blob)
    retained = "retained" in meta
    rebuilt = {} if retained else None
    if nbuf:
        result = _reconstruct(result, buffer_meta, buffers, rebuilt)
    if retained:
        retain_results(handle, meta, rebuilt, retain_segments, cache_stats)
    return result, exception, meta


def drop(key: WorkerKey) -> None:
    _workers.pop(key, None)


async def kill(key: WorkerKey) -> None:
    """Hard-kill the worker for ``key`` (task cancellation): its
    in-flight request fails with ChannelClosed; the next electron for
    the key spawns a fresh worker."""
    handle = _workers.pop(key, None)
    if handle is not None:
        handle.channel.kill()


async def close_all() -> None:
    handles = list(_workers.values())
    _workers.clear()
    _locks.clear()
    for h in handles:
        try:
            await h.channel.close()
        except Exception:  # noqa: BLE001
            app_log.debug("worker close failed", exc_info=True)


def reset() -> None:
    """Synchronous test hook (leaks processes if any are live — tests
    that start workers must close them)."""
    _workers.clear()
    _locks.clear()
