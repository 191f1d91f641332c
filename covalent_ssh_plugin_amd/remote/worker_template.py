"""Persistent remote worker for the MI355X SSH executor.

Like stub_template.py this file is NEVER imported by the plugin: it is
rendered (CSP token substitution) and shipped to the remote host once
per endpoint (content-addressed), then launched once per GPU slot over a
long-lived transport channel.  Where the classic stub pays a fresh
python + HIP-runtime start per electron (the reference's architecture,
/root/reference/covalent_ssh_plugin/exec.py), a worker pays it once:

  * starts, optionally runs the CDNA4 warm-up/device-probe prologue on
    its pinned GPU (the launcher injects CSP_GPU_SLOT; _resolve_gpu_slot
    maps it into the ambient HIP_VISIBLE_DEVICES),
  * then serves electrons over a length-framed binary protocol on
    stdin/stdout: each request carries the cloudpickled
    ``(fn, args, kwargs)`` and a workdir; each reply carries the pickled
    ``(result, exception)`` 2-tuple (same payload contract as the
    result file) plus a meta JSON dict.

Protocol (all frames: 8-byte big-endian length + payload):
  request  = pickle dict {"op_id", "workdir", "function_blob",
             "arg_buffers": [{dtype, shape}, ...]} followed by one RAW
             frame per entry (large CPU-tensor arguments, mirrored from
             the dispatcher without pickle copies).  An entry marked
             {"device": true} (executor option device_tensor_args) is not
             read into host memory at all: csp_h2d_stream_fd takes its
             frame off stdin chunk by chunk through the pinned ring, each
             chunk's H2D copy running while the next is read, and the
             electron gets a CUDA tensor.  When the entry carries
             "sum": [s0, s1], csp_checksum_dev recomputes the checksum
             over the bytes in HBM and a mismatch fails the task.  With
             the executor option cache_tensor_args an entry may also carry
             "cache": {"key", "store": true} (its frame lands in a master
             buffer that stays in HBM under the key, and the electron's
             tensor is a copy made and checksummed in one pass by
             csp_copy_checksum_dev) or {"key", "ref": true} (NO frame: the
             tensor is such a copy of the master already held; when the
             key is gone, or the checksum of the copy is not "sum", the
             argument fails, meta["arg_cache"]["miss"] names the entry and
             the dispatcher sends the task again with full frames).
             With the executor option pack_tensor_args the small tensor
             arguments of one electron share ONE entry {"device": true,
             "packed": [{dtype, shape, offset, nbytes}, ...], "nbytes":
             total, "sum": [s0, s1]} and ONE frame of total bytes (each
             tensor at its offset, a multiple of 16, zero padded); in
             (args, kwargs) each is ("__csp_packed_tensor_v1__", i, j).  The
             frame lands in HBM as one arena, csp_unpack_checksum_dev
             scatters it into a private tensor per segment and yields the
             arena's checksum in the same pass.  Such an entry may carry
             "cache" like any other: the arena is then the master.  With
             the executor option patch_tensor_args it may instead carry
             "cache": {"key": NEW, "patch": {"base": BASE, "segments":
             [j, ...]}} and "patch_nbytes": its ONE frame is then a delta
             arena of patch_nbytes bytes, the named segments in order in
             the same layout, and csp_patch_unpack_checksum_dev writes them
             over the master held under BASE in place, scatters the whole
             new arena and yields its checksum in one pass; the master is
             then held under NEW and meta["arg_cache"]["patched"] lists
             [BASE, NEW].  An absent BASE or a wrong checksum is a miss
             like a missed "ref", and the master goes.  With the executor
             option rebase_tensor_args it carries instead "cache": {"key":
             NEW, "rebase": {"base": BASE, "base_nbytes": N, "sources":
             [...]}} and "rebase_nbytes": sources[j] is segment j's offset
             in the arena of N bytes held under BASE, whatever that
             arena's layout, or -1 when its bytes are in the ONE frame, a
             delta arena of rebase_nbytes bytes with those segments in
             order.  csp_rebase_unpack_checksum_dev builds a NEW master
             from both, scatters it and yields its checksum in one pass;
             BASE stays in the cache and meta["arg_cache"]["rebased"]
             lists [BASE, NEW].  When the budget cannot hold both, no
             master is written and NEW is in "not_stored".  An absent
             BASE or a wrong checksum is a miss, and BASE goes.
  ack    = pickle tuple ("A1", op_id) — written as soon as the request
             (and its arg frames) has been fully received, BEFORE any
             user code runs.  The dispatcher uses it to distinguish
             "worker died before starting the task" (safe to retry on a
             fresh worker) from "worker died mid-execution" (retrying
             would re-run a possibly non-idempotent task — surfaced as
             an error instead, unless retry_on_worker_death opts in)
  response = pickle tuple ("R1", result_blob: bytes, meta: dict, nbuf: int)
             followed by nbuf RAW tensor-buffer frames.  Large tensors in
             the result are replaced by ("__csp_tensor_buffer_v1__", i)
             markers and shipped out-of-band as raw frames — CUDA tensors
             streamed by csp_d2h_stream_fd (their D2H copy runs chunk by
             chunk through a small hipHostMalloc-pinned ring WHILE the
             frame is being written), large CPU tensors zero-copy from
             their own storage — skipping both pickle copies on the
             payload.  meta["buffers"][i] carries
             dtype/shape.  With the executor option pack_tensor_results the
             CUDA tensors BELOW the staging threshold do not stay in the
             pickle either: csp_pack_dev gathers them into one device arena
             (each at a multiple of 16 bytes, zero padded), the arena goes
             out as one more streamed frame, each tensor becomes
             ("__csp_packed_tensor_v1__", i, j), and meta["buffers"][i] is
             {"packed": [{dtype, shape, offset, nbytes}, ...], "nbytes",
             "sum": [s0, s1]} with csp_checksum_dev's checksum of the arena,
             which the dispatcher verifies.  With the executor option
             retain_tensor_results the worker keeps CUDA result buffers in
             HBM as argument masters of the cache above: a CUDA tensor of at
             least min(STAGING_THRESHOLD, arg_cache_min_bytes) bytes is its
             own buffer, smaller ones share the packed arena, and for each
             ONE csp_pack_checksum_dev call gathers it into a new master
             (within ARG_CACHE_BYTES) and yields its checksum; the frame is
             streamed from the master, which stays under the worker's name
             "r:<op_id>:<buffer index>".  meta["buffers"][i] then carries
             "sum" and "retained": name, and meta["retained"] is {"stored",
             "not_stored", "evicted"} (every key retention pushed out).  The
             dispatcher later names such a master wherever a request refers
             to something held: the key of a "ref", the base of a "patch" or
             a "rebase" (whose delta may then be empty).  A buffer that
             cannot be retained takes the path above and
             meta["staging"]["retain_fallback"] says why.  A zero-length
             request frame means: shut down.

The worker's REAL stdout is reserved for the protocol; fd 1 is
re-pointed at stderr before any user code runs, so user prints cannot
corrupt frames.
"""


import collections
import json
import os
import struct
import sys
import time

GPU_LIB = "__CSP_GPU_LIB__"
DO_WARMUP = bool(__CSP_WARMUP__)
STAGING_THRESHOLD = int(__CSP_STAGING_THRESHOLD__)
# bytes per pinned ring chunk when a CUDA result is streamed to the channel
STREAM_CHUNK = int(__CSP_STREAM_CHUNK__)
IDLE_TIMEOUT = float(__CSP_IDLE_TIMEOUT__)  # seconds; 0 = never exit
# Pack the CUDA tensors of a result that are below STAGING_THRESHOLD into
# one device arena sent as a single streamed, checksummed frame, when they
# total at least PACK_MIN_BYTES.
PACK_RESULTS = bool(__CSP_PACK_RESULTS__)
PACK_MIN_BYTES = int(__CSP_PACK_MIN_BYTES__)
# Budget in bytes for the masters of repeated tensor arguments kept in HBM
# (executor option cache_tensor_args); 0 = no cache.
ARG_CACHE_BYTES = int(__CSP_ARG_CACHE_BYTES__)
# Keep CUDA result buffers as argument masters in that cache (executor option
# retain_tensor_results): the executor's arg_cache_min_bytes, so that results
# are split into buffers where the argument side splits them; -1 = off.
RETAIN_MIN_BYTES = int(__CSP_RETAIN_MIN_BYTES__)
# Fork-isolation mode: the worker is a warm ZYGOTE (python + cloudpickle
# imported, HIP **not** initialized — initializing HIP pre-fork would
# break the children) and every electron executes in a freshly forked
# child that does its own GPU prologue.  Fresh-process semantics at fork
# cost instead of a full interpreter + import start per task.
ISOLATE = bool(__CSP_ISOLATE__)
# What the zygote binds before forking.  "torch": children inherit a
# loaded torch — saves the multi-second import for torch-using electrons
# but makes each fork copy the torch-ROCm address space (measured
# ~250 ms/fork on MI355X vs ~ms without).  "none": cheap forks; torch
# electrons pay their own import.  Choose per workload.
ISOLATE_PRELOAD = "__CSP_ISOLATE_PRELOAD__"
# Per-task GPU telemetry: sample HBM occupancy (hipMemGetInfo) every Nth
# electron into the task meta.  0 = off (the hot no-op path stays
# syscall-minimal); enable for GPU-heavy workloads where ~0.1 ms of
# sampling is noise.
TELEMETRY_EVERY = int(__CSP_TELEMETRY_EVERY__)
_last_mem = None

if GPU_LIB:
    GPU_LIB = os.path.abspath(os.path.expanduser(GPU_LIB))


def _resolve_gpu_slot():
    """Map CSP_GPU_SLOT to HIP_VISIBLE_DEVICES within the ambient
    visibility list (composes with pod GPU isolation).  Must run before
    any HIP/torch initialization."""
    slot = os.environ.get("CSP_GPU_SLOT")
    if slot is None:
        return None
    ambient = os.environ.get("HIP_VISIBLE_DEVICES") or ""
    ids = [x for x in ambient.split(",") if x.strip() != ""]
    if ids:
        os.environ["HIP_VISIBLE_DEVICES"] = ids[int(slot) % len(ids)]
    else:
        os.environ["HIP_VISIBLE_DEVICES"] = slot
    return slot


GPU_SLOT = _resolve_gpu_slot()

# --- claim the protocol channel, push user stdout to stderr ---------------
_proto_fd = os.dup(1)
os.dup2(2, 1)
sys.stdout = sys.stderr

# widen the protocol pipes (default 64 KiB caps large-tensor frames)
try:
    import fcntl

    F_SETPIPE_SZ = 1031  # linux
    for _fd in (0, _proto_fd):
        try:
            fcntl.fcntl(_fd, F_SETPIPE_SZ, 1 << 20)
        except OSError:
            pass
except ImportError:
    pass

import cloudpickle as pickle  # noqa: E402  (after fd surgery on purpose)

_gpu_lib = None
_gpu_info = None
_served = 0  # electrons completed by this worker (observability)


def _ensure_torch_runtime_first():
    """One process can host only ONE HSA runtime.  torch bundles its own
    ROCm runtime; if our ctypes library initializes the system runtime
    first, a later torch.cuda init finds no agents ("No HIP GPUs are
    available").  So when torch is installed, import it (binding its
    runtime) BEFORE loading the CDNA4 library — the library then resolves
    libamdhip64.so.7 to torch's already-loaded copy (soname dedup) and
    both share one runtime.  Measured on-box: probe-then-torch breaks,
    torch-then-probe runs the probe at full rate."""
    import importlib.util

    if importlib.util.find_spec("torch") is None:
        return
    import torch

    if torch.cuda.is_available():
        torch.cuda.init()


def _load_gpu_lib():
    import ctypes

    _ensure_torch_runtime_first()

    lib = ctypes.CDLL(GPU_LIB)
    lib.csp_probe_json.restype = ctypes.c_int
    lib.csp_probe_json.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.csp_warmup.restype = ctypes.c_int
    lib.csp_warmup.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.csp_staging_alloc.restype = ctypes.c_void_p
    lib.csp_staging_alloc.argtypes = [ctypes.c_size_t]
    lib.csp_staging_release_all.restype = ctypes.c_int
    lib.csp_memcpy_d2h.restype = ctypes.c_int
    lib.csp_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.csp_d2h_stream_fd.restype = ctypes.c_int
    lib.csp_d2h_stream_fd.argtypes = [
        ctypes.c_int,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_h2d_stream_fd.restype = ctypes.c_int
    lib.csp_h2d_stream_fd.argtypes = [
        ctypes.c_int,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_size_t,
        ctypes.c_int,
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_checksum_dev.restype = ctypes.c_int
    lib.csp_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
    ]
    lib.csp_copy_checksum_dev.restype = ctypes.c_int
    lib.csp_copy_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
    ]
    lib.csp_pack_dev.restype = ctypes.c_int
    lib.csp_pack_dev.argtypes = [
        ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_unpack_checksum_dev.restype = ctypes.c_int
    lib.csp_unpack_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    if RETAIN_MIN_BYTES >= 0:
        lib.csp_pack_checksum_dev.restype = ctypes.c_int
        lib.csp_pack_checksum_dev.argtypes = [
            ctypes.POINTER(ctypes.c_void_p),
            ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ctypes.c_uint64),
            ctypes.c_size_t,
            ctypes.c_void_p,
            ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_uint64),
            ctypes.POINTER(ctypes.c_double),
        ]
    lib.csp_patch_unpack_checksum_dev.restype = ctypes.c_int
    lib.csp_patch_unpack_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_rebase_unpack_checksum_dev.restype = ctypes.c_int
    lib.csp_rebase_unpack_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_mem_info.restype = ctypes.c_int
    lib.csp_mem_info.argtypes = [
        ctypes.c_int,
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_last_error.restype = ctypes.c_char_p
    return lib


def _sample_hbm():
    """Cheap HBM occupancy sample for the task meta (telemetry row in
    SURVEY.md §5; sampled every TELEMETRY_EVERY electrons)."""
    global _last_mem
    if _gpu_lib is None:
        return
    import ctypes

    free_gb = ctypes.c_double()
    total_gb = ctypes.c_double()
    if _gpu_lib.csp_mem_info(0, ctypes.byref(free_gb), ctypes.byref(total_gb)) == 0:
        _last_mem = {
            "hbm_free_gb": round(free_gb.value, 2),
            "hbm_total_gb": round(total_gb.value, 2),
            "sampled_at_serial": _served,
        }


def _prologue():
    """One-time GPU warm-up + probe for this worker's pinned device."""
    global _gpu_lib, _gpu_info
    import ctypes

    _gpu_lib = _load_gpu_lib()
    buf = ctypes.create_string_buffer(8192)
    rc = _gpu_lib.csp_probe_json(0, buf, len(buf))
    if rc != 0:
        raise RuntimeError(
            "csp_probe_json failed: %s"
            % _gpu_lib.csp_last_error().decode(errors="replace")
        )
    _gpu_info = json.loads(buf.value.decode())
    if DO_WARMUP:
        rc = _gpu_lib.csp_warmup(0, 50)
        if rc != 0:
            raise RuntimeError(
                "csp_warmup failed: %s"
                % _gpu_lib.csp_last_error().decode(errors="replace")
            )


class _DeferredCuda:
    """A CUDA result buffer (one large tensor, or the arena of packed small
    ones) whose bytes leave the device only while its frame is being sent
    (see _send_buffer)."""

    def __init__(self, lib, ptr, nbytes):
        self.lib = lib
        self.ptr = ptr
        self.nbytes = nbytes


def _send_buffer(fd, view):
    """Write one out-of-band result buffer as a frame on ``fd``."""
    if not isinstance(view, _DeferredCuda):
        _write_frame(fd, view)
        return
    import ctypes

    rc = view.lib.csp_d2h_stream_fd(
        fd, ctypes.c_void_p(view.ptr), view.nbytes, STREAM_CHUNK, None, None
    )
    if rc != 0:
        # R1 has already promised this frame, and a frame that failed
        # part-way cannot be made valid: leave, so the dispatcher sees
        # ChannelClosed after the ack instead of a shifted stream
        sys.stderr.write(
            "csp worker: csp_d2h_stream_fd failed (rc=%d): %s\n"
            % (rc, view.lib.csp_last_error().decode(errors="replace"))
        )
        sys.stderr.flush()
        os._exit(4)


def _retain_large_bytes():
    """With retention on, a CUDA result tensor of at least this many bytes is
    its own out-of-band buffer: where the argument side stops packing."""
    return min(STAGING_THRESHOLD, RETAIN_MIN_BYTES)


def _pack_checksum(lib, src_ptrs, offsets, sizes, arena_ptr, total):
    """One csp_pack_checksum_dev call; returns [s0, s1] of the arena."""
    import ctypes

    count = len(sizes)
    out = (ctypes.c_uint64 * 2)()
    rc = lib.csp_pack_checksum_dev(
        (ctypes.c_void_p * count)(*src_ptrs), (ctypes.c_uint64 * count)(*offsets),
        (ctypes.c_uint64 * count)(*sizes), count, ctypes.c_void_p(arena_ptr), total,
        out, None,
    )
    if rc != 0:
        raise RuntimeError(
            "csp_pack_checksum_dev failed (rc=%d): %s"
            % (rc, lib.csp_last_error().decode(errors="replace"))
        )
    return [int(out[0]), int(out[1])]


def _retain_buffer(lib, retain, index, src_ptrs, offsets, sizes, total, nbytes, stats,
                   keep=True):
    """Result buffer ``index`` gathered, copied and checksummed by one
    csp_pack_checksum_dev call into a buffer of its own of ``total`` bytes,
    which with ``keep`` is a new argument master held under the worker's name
    "r:<op_id>:<index>" as (master, nbytes, sum).  Returns (buffer, sum,
    name or None).  No room in the budget, no HBM, or any refusal or error of
    the call: None, the reason in stats["retain_fallback"], and the buffer
    takes the path it takes without retention.  The caller has synchronised
    the null stream."""
    global _arg_cache_resident
    import torch

    t0 = time.monotonic()
    report = retain["report"]
    name = "r:%s:%d" % (retain["op_id"], index) if keep else None
    evicted = _new_arg_cache_report()
    try:
        if keep:
            _arg_cache_drop(name)  # an op_id used twice: the new result replaces the old
            arena = _arg_cache_new_master(total, evicted)
            if arena is None:
                raise RuntimeError(
                    "no room for %d bytes in the budget of %d or in HBM"
                    % (total, ARG_CACHE_BYTES)
                )
        else:
            arena = torch.empty(total, dtype=torch.uint8, device="cuda")
        sums = _pack_checksum(lib, src_ptrs, offsets, sizes, arena.data_ptr(), total)
    except Exception as e:  # noqa: BLE001 - retention never fails a task
        stats["retain_fallback"] = repr(e)[:500]
        if keep:
            report["not_stored"].append(name)
        return None
    finally:
        report["evicted"].extend(evicted["evicted"])
        stats["retain_ms"] = round(
            stats.get("retain_ms", 0.0) + (time.monotonic() - t0) * 1000, 3
        )
    if keep:
        _arg_cache[name] = (arena, nbytes, sums)
        _arg_cache_resident += total  # as allocated and as checked against the budget
        report["stored"].append(name)
        retain.setdefault("sizes", {})[name] = nbytes
        stats["retained_buffers"] = stats.get("retained_buffers", 0) + 1
        stats["retained_bytes"] = stats.get("retained_bytes", 0) + nbytes
    return arena, sums, name


def _retain_settle(retain, buffer_meta, stats):
    """After staging: a master that a later buffer of the same result pushed
    out of the budget is not held after all."""
    report = retain["report"]
    gone = [name for name in report["stored"] if name not in _arg_cache]
    for name in gone:
        report["stored"].remove(name)
        report["not_stored"].append(name)
        stats["retained_buffers"] -= 1
        stats["retained_bytes"] -= retain["sizes"][name]
        for info in buffer_meta:
            if info.get("retained") == name:
                del info["retained"]
    report["evicted"] = [k for k in report["evicted"] if k not in gone]


def _retain_rollback(retain):
    """The result does not leave after all: nothing of it stays held."""
    report = retain["report"]
    for name in report["stored"]:
        _arg_cache_drop(name)
    report["not_stored"].extend(report["stored"])
    report["stored"] = []


def _small_cuda_tensors(result, limit=None):
    """The CUDA tensors of ``result`` below ``limit`` (STAGING_THRESHOLD when
    None), each object once, in walk order."""
    import torch

    found = {}
    if limit is None:
        limit = STAGING_THRESHOLD

    def walk(obj):
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda and obj.numel() * obj.element_size() < limit:
                found.setdefault(id(obj), obj)
        elif isinstance(obj, dict):
            for v in obj.values():
                walk(v)
        elif isinstance(obj, (tuple, list)):
            for v in obj:
                walk(v)

    walk(result)
    return list(found.values())


def _pack_small_cuda(lib, result, stats, buffers, buffer_meta, retain=None):
    """Gather the small CUDA tensors of ``result`` into one device arena
    with csp_pack_dev and emit it as one streamed buffer.  Returns
    {id(tensor): marker}; empty when there is nothing to pack, the total is
    below PACK_MIN_BYTES, or anything went wrong (the reason then goes to
    stats["pack_fallback"] and the tensors take the per-tensor path).

    The arena is a transient second copy of the packed tensors in HBM until
    its frame is sent; only the out-of-memory fallback bounds its size.

    With ``retain`` (retention on) the small tensors are those below
    _retain_large_bytes(), one csp_pack_checksum_dev call stands in for
    csp_pack_dev and csp_checksum_dev, and an arena of at least
    max(1, RETAIN_MIN_BYTES) bytes stays in HBM as an argument master
    (_retain_buffer); when that fails the two calls run as without it."""
    import ctypes

    import torch

    tensors = _small_cuda_tensors(
        result, None if retain is None else _retain_large_bytes()
    )
    sizes = [t.numel() * t.element_size() for t in tensors]
    if not tensors or sum(sizes) == 0 or sum(sizes) < PACK_MIN_BYTES:
        return {}
    name = None
    try:
        # torch makes non-contiguous tensors contiguous, as on the large path
        srcs = [t.contiguous() for t in tensors]
        offsets = []
        total = 0
        for n in sizes:
            offsets.append(total)
            total += (n + 15) // 16 * 16
        # the library's copy stream does not wait on the null stream
        torch.cuda.synchronize()
        count = len(srcs)
        ptrs = [(t.data_ptr() or None) if n else None for t, n in zip(srcs, sizes)]
        kept = None
        if retain is not None:
            kept = _retain_buffer(
                lib, retain, len(buffers), ptrs, offsets, sizes, total, total, stats,
                keep=total >= max(1, RETAIN_MIN_BYTES),
            )
        if kept is not None:
            arena, sums, name = kept
        else:
            arena = torch.empty(total, dtype=torch.uint8, device="cuda")
            rc = lib.csp_pack_dev(
                (ctypes.c_void_p * count)(*ptrs), (ctypes.c_uint64 * count)(*offsets),
                (ctypes.c_uint64 * count)(*sizes), count,
                ctypes.c_void_p(arena.data_ptr()), total, None,
            )
            if rc != 0:
                raise RuntimeError(
                    "csp_pack_dev failed (rc=%d): %s"
                    % (rc, lib.csp_last_error().decode(errors="replace"))
                )
            sums = (ctypes.c_uint64 * 2)()
            rc = lib.csp_checksum_dev(ctypes.c_void_p(arena.data_ptr()), total, sums)
            if rc != 0:
                raise RuntimeError(
                    "csp_checksum_dev failed (rc=%d): %s"
                    % (rc, lib.csp_last_error().decode(errors="replace"))
                )
    except Exception as e:  # noqa: BLE001 - packing never fails a task
        stats["pack_fallback"] = repr(e)[:500]
        return {}
    del srcs  # their bytes are in the arena
    buffers.append((_DeferredCuda(lib, arena.data_ptr(), total), arena))
    buffer_meta.append({
        "packed": [
            {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
             "offset": off, "nbytes": n}
            for t, off, n in zip(tensors, offsets, sizes)
        ],
        "nbytes": total,
        "sum": [int(sums[0]), int(sums[1])],
    })
    if name is not None:
        buffer_meta[-1]["retained"] = name
    index = len(buffers) - 1
    stats["packed_tensors"] = count
    stats["packed_bytes"] = sum(sizes)
    stats["mode"] = "pinned"
    return {
        id(t): ("__csp_packed_tensor_v1__", index, j) for j, t in enumerate(tensors)
    }


def _stage_result(result, stats, buffers, buffer_meta, retain=None):
    """Replace large tensors in ``result`` with out-of-band buffer
    markers.  A large CUDA tensor is only recorded here (device pointer,
    byte count, the tensor as keep-alive); the send loop streams it
    through hipHostMalloc-pinned memory.  Large contiguous CPU tensors
    are shipped zero-copy from their own storage.  Small tensors stay
    inline in the pickle, unless PACK_RESULTS gathers the small CUDA
    tensors into one more streamed buffer (_pack_small_cuda).

    ``retain`` ({"op_id", "report"}; retention on): a CUDA tensor of at least
    _retain_large_bytes() bytes is copied and checksummed by one
    csp_pack_checksum_dev call into a new argument master, its frame is
    streamed from the master (the user's tensor is let go) and its meta entry
    carries "sum" and "retained"; the packed arena likewise.  A buffer that
    cannot be retained takes the path it takes without retention."""
    if "torch" not in sys.modules:
        return result
    import ctypes

    import torch

    lib = _gpu_lib
    if lib is None and GPU_LIB and os.path.exists(GPU_LIB):
        try:
            lib = _load_gpu_lib()
        except Exception:  # noqa: BLE001
            lib = None

    if lib is None:
        retain = None
    packed = {}
    if PACK_RESULTS and lib is not None:
        packed = _pack_small_cuda(lib, result, stats, buffers, buffer_meta, retain)

    def emit_buffer(view, keepalive, dtype, shape):
        buffers.append((view, keepalive))
        buffer_meta.append(
            {"dtype": str(dtype).replace("torch.", ""), "shape": list(shape)}
        )
        return ("__csp_tensor_buffer_v1__", len(buffers) - 1)

    retained_markers = {}  # id(tensor) -> marker: one object met twice, one master

    def retain_large(t, nbytes):
        """The marker of ``t``'s retained buffer, or None."""
        if id(t) in retained_markers:
            return retained_markers[id(t)]
        src_t = t.contiguous()
        # the library's copy stream does not wait on the null stream
        torch.cuda.synchronize()
        total = (nbytes + 15) // 16 * 16
        kept = _retain_buffer(
            lib, retain, len(buffers), [src_t.data_ptr()], [0], [nbytes], total, nbytes,
            stats,
        )
        if kept is None:
            return None
        master, sums, name = kept
        stats["pinned_tensors"] += 1
        stats["mode"] = "pinned"
        marker = emit_buffer(
            _DeferredCuda(lib, master.data_ptr(), nbytes), master, src_t.dtype, src_t.shape
        )
        buffer_meta[-1]["sum"] = sums
        buffer_meta[-1]["retained"] = name
        retained_markers[id(t)] = marker
        return marker

    def to_host(t):
        stats["tensors"] += 1
        nbytes = t.numel() * t.element_size()
        stats["bytes"] += nbytes
        if id(t) in packed:
            return packed[id(t)]
        if retain is not None and t.is_cuda and 0 < nbytes >= _retain_large_bytes():
            marker = retain_large(t, nbytes)
            if marker is not None:
                return marker
        if nbytes < STAGING_THRESHOLD:
            return t.cpu() if t.is_cuda else t
        if t.is_cuda:
            if lib is None:
                raise RuntimeError(
                    "CUDA tensor result but the CDNA4 staging library is "
                    "not available on this GPU host"
                )
            src_t = t.contiguous()
            # the library's copy stream does not wait on the null stream
            torch.cuda.synchronize()
            view = _DeferredCuda(lib, src_t.data_ptr(), nbytes)
            stats["pinned_tensors"] += 1
            stats["mode"] = "pinned"
            return emit_buffer(view, src_t, src_t.dtype, src_t.shape)
        # large CPU tensor: zero-copy out-of-band (keep tensor alive)
        src_t = t.contiguous()
        view = (ctypes.c_char * nbytes).from_address(src_t.data_ptr())
        if stats["mode"] != "pinned":
            stats["mode"] = "cpu-oob"
        return emit_buffer(view, src_t, src_t.dtype, src_t.shape)

    def walk(obj):
        if isinstance(obj, torch.Tensor):
            return to_host(obj)
        if isinstance(obj, dict):
            return {k: walk(v) for k, v in obj.items()}
        if isinstance(obj, tuple):
            vals = [walk(v) for v in obj]
            return type(obj)(*vals) if hasattr(obj, "_fields") else tuple(vals)
        if isinstance(obj, list):
            return [walk(v) for v in obj]
        return obj

    staged = walk(result)
    if retain is not None:
        _retain_settle(retain, buffer_meta, stats)
    return staged


def _read_frame(fd, idle_timeout=0.0):
    if idle_timeout > 0:
        import select

        ready, _, _ = select.select([fd], [], [], idle_timeout)
        if not ready:
            return None  # idle too long: orderly exit
    header = b""
    while len(header) < 8:
        chunk = os.read(fd, 8 - len(header))
        if not chunk:
            return None
        header += chunk
    (length,) = struct.unpack(">Q", header)
    if length == 0:
        return b""
    parts = []
    remaining = length
    while remaining:
        chunk = os.read(fd, min(remaining, 1 << 20))
        if not chunk:
            return None
        parts.append(chunk)
        remaining -= len(chunk)
    return b"".join(parts)


def _write_frame(fd, payload):
    view = memoryview(payload)
    if view.nbytes <= 64 * 1024:
        # small frames: single write (header + payload) — halves the
        # per-frame syscalls on the no-op hot path
        os.write(fd, struct.pack(">Q", view.nbytes) + bytes(view))
        return
    os.write(fd, struct.pack(">Q", view.nbytes))
    while view:
        written = os.write(fd, view[: 1 << 20])
        view = view[written:]


# --- tensor arguments that land on the device -------------------------------

_NO_DEVICE_ARGS = (
    "device tensor arguments (device_tensor_args) need a GPU worker with "
    "the CDNA4 library: "
)


def _new_arg_stage():
    return {"mode": "none", "tensors": 0, "bytes": 0, "verified": 0,
            "read_ms": 0.0, "h2d_ms": 0.0}


def _device_arg_lib():
    """The CDNA4 library for device arguments, loaded on first use the way
    _stage_result does.  Raises the documented RuntimeError when torch,
    a GPU or the library is missing."""
    global _gpu_lib
    import importlib.util

    if importlib.util.find_spec("torch") is None:
        raise RuntimeError(_NO_DEVICE_ARGS + "torch is not installed on the worker")
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE_ARGS + "the worker sees no GPU")
    if _gpu_lib is None:
        if not (GPU_LIB and os.path.exists(GPU_LIB)):
            raise RuntimeError(_NO_DEVICE_ARGS + "the library was not provisioned")
        try:
            _gpu_lib = _load_gpu_lib()
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(_NO_DEVICE_ARGS + "loading it failed: %r" % (e,))
    return _gpu_lib


def _verify_device_arg(lib, index, tensor, nbytes, info, stage):
    """Compare the dispatcher's checksum with csp_checksum_dev's over the
    bytes in HBM (a zero-byte tensor against (0, 0))."""
    if "sum" not in info:
        return
    import ctypes

    out = (ctypes.c_uint64 * 2)()
    ptr = tensor.data_ptr() if nbytes else 0
    if lib.csp_checksum_dev(ctypes.c_void_p(ptr), nbytes, out) != 0:
        raise RuntimeError(
            "argument buffer %d: csp_checksum_dev failed: %s"
            % (index, lib.csp_last_error().decode(errors="replace"))
        )
    stage["verified"] += 1
    _compare_arg_sum(index, [int(out[0]), int(out[1])], info, nbytes)


def _compare_arg_sum(index, got, info, nbytes):
    want = [int(info["sum"][0]), int(info["sum"][1])]
    if got != want:
        raise RuntimeError(
            "argument buffer %d failed its integrity check: the dispatcher "
            "sent checksum %r, the %d bytes on the device give %r"
            % (index, want, nbytes, got)
        )


# --- repeated tensor arguments kept in HBM (cache_tensor_args) --------------
#
# key -> (master, nbytes, [s0, s1]); least recently used first.  A master is
# a uint8 CUDA tensor that only this file touches: every electron gets a
# private copy made (and verified) by csp_copy_checksum_dev.

_arg_cache = collections.OrderedDict()
_arg_cache_resident = 0  # bytes held by the masters


def _new_arg_cache_report():
    return {"hits": [], "stored": [], "not_stored": [], "miss": [], "evicted": []}


def _arg_cache_drop(key, report=None):
    global _arg_cache_resident
    entry = _arg_cache.pop(key, None)
    if entry is not None:
        # what the master holds: nbytes, or for a retained large result the
        # next multiple of 16
        _arg_cache_resident -= entry[0].numel()
        if report is not None:
            report["evicted"].append(key)


def _arg_cache_evict_all(report, keep=None):
    """Let go of every master but ``keep`` and return their memory to the
    device.  Returns whether anything was let go."""
    import torch

    victims = [k for k in _arg_cache if k != keep]
    for k in victims:
        _arg_cache_drop(k, report)
    if victims:
        torch.cuda.empty_cache()
    return bool(victims)


def _arg_cache_new_master(nbytes, report, keep=None):
    """A master of ``nbytes`` within ARG_CACHE_BYTES, least recently used
    entries evicted to make room; None when it does not fit the budget or
    the device has no room for it.  ``keep``: a key that is never evicted
    (the base of a rebase); None as well when the budget cannot hold it and
    the new master together, and then nothing is evicted."""
    import torch

    if nbytes > ARG_CACHE_BYTES:
        return None
    if keep is not None and keep in _arg_cache:
        if _arg_cache[keep][1] + nbytes > ARG_CACHE_BYTES:
            return None
    while _arg_cache and _arg_cache_resident + nbytes > ARG_CACHE_BYTES:
        victim = next(k for k in _arg_cache if k != keep)
        _arg_cache_drop(victim, report)
    try:
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    except Exception:  # noqa: BLE001 - out of HBM: the argument goes uncached
        return None


def _alloc_device_arg(info, dtype, report, keep=None):
    """The electron's own tensor.  When the device has no room, the masters
    (all but ``keep``) go and the allocation is tried once more."""
    import torch

    try:
        return torch.empty(info["shape"], dtype=dtype, device="cuda")
    except Exception:  # noqa: BLE001 - e.g. out of HBM
        if not _arg_cache_evict_all(report, keep=keep):
            raise
    return torch.empty(info["shape"], dtype=dtype, device="cuda")


def _copy_from_master(lib, index, tensor, master, nbytes):
    """csp_copy_checksum_dev(master -> tensor); returns [s0, s1]."""
    import ctypes

    out = (ctypes.c_uint64 * 2)()
    rc = lib.csp_copy_checksum_dev(
        ctypes.c_void_p(tensor.data_ptr()), ctypes.c_void_p(master.data_ptr()),
        nbytes, out,
    )
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: csp_copy_checksum_dev failed: %s"
            % (index, lib.csp_last_error().decode(errors="replace"))
        )
    return [int(out[0]), int(out[1])]


def _device_arg_from_cache(lib, index, info, dtype, nbytes, key, stage, report):
    """A ``ref`` entry: no frame on the wire, the tensor is a verified copy
    of the cached master.  An absent key, another byte count or another
    checksum is a miss: the entry goes, the index is reported, and the
    argument fails with an error that the dispatcher answers by sending the
    task again with full frames."""
    entry = _arg_cache.get(key)
    reason = None
    if entry is None:
        reason = "is not in the cache"
    elif entry[1] != nbytes or "sum" not in info:
        reason = "holds %d bytes, the argument has %d" % (entry[1], nbytes)
    else:
        tensor = _alloc_device_arg(info, dtype, report, keep=key)
        got = _copy_from_master(lib, index, tensor, entry[0], nbytes)
        want = [int(info["sum"][0]), int(info["sum"][1])]
        if got == want:
            _arg_cache.move_to_end(key)
            report["hits"].append(key)
            stage["tensors"] += 1
            stage["verified"] += 1
            if stage["mode"] == "none":
                stage["mode"] = "cached"
            return tensor
        reason = "has checksum %r, the dispatcher sent %r" % (got, want)
    _arg_cache_drop(key)
    report["miss"].append(index)
    raise RuntimeError(
        "argument buffer %d: cached argument %s %s" % (index, key, reason)
    )


def _receive_device_arg(index, info, stage, report):
    """Persistent mode: take argument frame ``index`` off stdin straight
    into a fresh CUDA tensor.  Whatever goes wrong short of a broken
    stream, the frame is consumed before the error is raised, so the
    caller can go on to the next frame and report the error in R1.

    With ``"cache": {"key", "ref": true}`` there is no frame: the tensor is
    copied from the cached master (_device_arg_from_cache).  With
    ``"cache": {"key", "store": true}`` the frame lands in a new master
    first and the tensor is a verified copy of it; when the key is already
    cached, or the master does not fit, the frame lands in the tensor as
    without a cache."""
    global _arg_cache_resident
    import ctypes

    cache = info.get("cache") or {}
    try:
        lib = _device_arg_lib()
    except RuntimeError:
        if not cache.get("ref") and _read_frame(0) is None:  # drain with the Python reader
            os._exit(4)
        raise
    import torch

    dtype = getattr(torch, info["dtype"])
    nbytes = torch.empty((), dtype=dtype).element_size()
    for dim in info["shape"]:
        nbytes *= int(dim)
    # the library's copy stream does not wait on the null stream
    torch.cuda.synchronize()
    if cache.get("ref"):
        return _device_arg_from_cache(
            lib, index, info, dtype, nbytes, cache["key"], stage, report
        )
    key = None
    master = None
    if cache.get("store") and "sum" in info and nbytes:
        key = cache["key"]
        if key in _arg_cache:
            # the frame is on its way all the same: it lands in the tensor
            _arg_cache.move_to_end(key)
            report["stored"].append(key)
            key = None
        else:
            master = _arg_cache_new_master(nbytes, report)
            if master is None:
                report["not_stored"].append(key)
    alloc_error = None
    tensor = None
    try:
        tensor = _alloc_device_arg(info, dtype, report)
    except Exception as e:  # noqa: BLE001 - e.g. out of HBM
        alloc_error = e  # drain mode below: the frame still has to go
        if master is not None:
            # the new master goes too: the argument travels uncached
            master = None
            report["not_stored"].append(key)
            torch.cuda.empty_cache()
            try:
                tensor = torch.empty(info["shape"], dtype=dtype, device="cuda")
                alloc_error = None
            except Exception as e2:  # noqa: BLE001
                alloc_error = e2
    ptr = tensor.data_ptr() if (tensor is not None and nbytes) else 0
    if master is not None:
        ptr = master.data_ptr()
    read_ms = ctypes.c_double()
    h2d_ms = ctypes.c_double()
    rc = lib.csp_h2d_stream_fd(
        0, ctypes.c_void_p(ptr), nbytes, STREAM_CHUNK, -1,
        ctypes.byref(read_ms), ctypes.byref(h2d_ms),
    )
    stage["read_ms"] += read_ms.value
    stage["h2d_ms"] += h2d_ms.value
    if rc == 2:
        # the request stream is no longer aligned: same policy as a
        # failed send, leave so the dispatcher sees ChannelClosed
        sys.stderr.write(
            "csp worker: csp_h2d_stream_fd lost the stream: %s\n"
            % lib.csp_last_error().decode(errors="replace")
        )
        sys.stderr.flush()
        os._exit(4)
    if alloc_error is not None:
        raise alloc_error
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: H2D copy failed (rc=%d): %s"
            % (index, rc, lib.csp_last_error().decode(errors="replace"))
        )
    stage["mode"] = "pinned-h2d"
    stage["tensors"] += 1
    stage["bytes"] += nbytes
    if master is None:
        _verify_device_arg(lib, index, tensor, nbytes, info, stage)
        return tensor
    # the copy that the electron gets is also the verification pass
    got = _copy_from_master(lib, index, tensor, master, nbytes)
    stage["verified"] += 1
    _compare_arg_sum(index, got, info, nbytes)  # a mismatch drops the master
    _arg_cache[key] = (master, nbytes, got)
    _arg_cache_resident += nbytes
    report["stored"].append(key)
    return tensor


# --- small tensor arguments packed into one frame (pack_tensor_args) --------

# Ring chunk for a packed arena's frame.  Measured on the 295 MB, 200-tensor
# arena (profiles/packed_args.md): 75 ms per dispatch with 1 MiB chunks, 79 ms
# with 4 MiB, 92 ms with STREAM_CHUNK's 16 MiB (82 ms per tensor, unpacked).
PACKED_ARG_CHUNK = 1 << 20


def _alloc_packed_tensors(info, report, keep=None):
    """The electron's private tensors for a packed entry, one allocation
    each (a survivor then pins its own bytes, not an arena)."""
    import torch

    tensors = []
    for seg in info["packed"]:
        dtype = getattr(torch, seg["dtype"])
        t = _alloc_device_arg(seg, dtype, report, keep=keep)
        if t.numel() * t.element_size() != int(seg["nbytes"]):
            raise RuntimeError(
                "packed argument: %s%r is not %d bytes"
                % (seg["dtype"], seg["shape"], int(seg["nbytes"]))
            )
        tensors.append(t)
    return tensors


def _unpack_arena(lib, index, arena, total, info, tensors, stage):
    """One csp_unpack_checksum_dev call: the arena's segments into
    ``tensors``, and [s0, s1] of the whole arena from the same pass."""
    import ctypes

    segs = info["packed"]
    count = len(segs)
    sizes = [int(seg["nbytes"]) for seg in segs]
    dst = (ctypes.c_void_p * count)(
        *[(t.data_ptr() or None) if n else None for t, n in zip(tensors, sizes)]
    )
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    rc = lib.csp_unpack_checksum_dev(
        ctypes.c_void_p(arena.data_ptr() if total else 0), total, dst,
        (ctypes.c_uint64 * count)(*[int(seg["offset"]) for seg in segs]),
        (ctypes.c_uint64 * count)(*sizes), count, out, ctypes.byref(kernel_ms),
    )
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: csp_unpack_checksum_dev failed: %s"
            % (index, lib.csp_last_error().decode(errors="replace"))
        )
    stage["packed_tensors"] = stage.get("packed_tensors", 0) + count
    stage["packed_bytes"] = stage.get("packed_bytes", 0) + sum(sizes)
    stage["unpack_ms"] = round(stage.get("unpack_ms", 0.0) + kernel_ms.value, 3)
    return [int(out[0]), int(out[1])]


def _packed_args_from_cache(lib, index, info, total, key, stage, report):
    """A ``ref`` packed entry: no frame, the tensors are unpacked from the
    cached arena and the arena verified in the same pass.  A miss is what it
    is in _device_arg_from_cache."""
    entry = _arg_cache.get(key)
    reason = None
    if entry is None:
        reason = "is not in the cache"
    elif entry[1] != total or "sum" not in info:
        reason = "holds %d bytes, the argument has %d" % (entry[1], total)
    else:
        tensors = _alloc_packed_tensors(info, report, keep=key)
        got = _unpack_arena(lib, index, entry[0], total, info, tensors, stage)
        want = [int(info["sum"][0]), int(info["sum"][1])]
        if got == want:
            _arg_cache.move_to_end(key)
            report["hits"].append(key)
            stage["tensors"] += 1
            stage["verified"] += 1
            if stage["mode"] == "none":
                stage["mode"] = "cached"
            return tensors
        reason = "has checksum %r, the dispatcher sent %r" % (got, want)
    _arg_cache_drop(key)
    report["miss"].append(index)
    raise RuntimeError(
        "argument buffer %d: cached argument %s %s" % (index, key, reason)
    )


def _packed_chunk():
    return min(STREAM_CHUNK, PACKED_ARG_CHUNK) if STREAM_CHUNK > 0 else PACKED_ARG_CHUNK


def _patch_packed_args(lib, index, info, total, cache, stage, report):
    """A ``patch`` packed entry: the frame is a delta arena, the changed
    segments of the held arena ``base`` in the pack layout.  ONE
    csp_patch_unpack_checksum_dev call writes them over the master in place,
    scatters the whole new arena into private tensors and yields its
    checksum; the master is then held under the new key.  The frame is
    consumed whatever happens.  An absent base, another byte count, no
    ``sum`` or another checksum is a miss as in _packed_args_from_cache, and
    the master goes: after a failed patch in place its bytes are unknown.
    When the new key is already held the frame is only drained, the base
    stays, and the tensors come from the arena held under the new key."""
    import ctypes

    import torch

    new_key = cache["key"]
    base_key = cache["patch"]["base"]
    delta_total = int(info["patch_nbytes"])
    converged = new_key in _arg_cache
    entry = _arg_cache.get(base_key)
    reason = None
    if converged:
        pass
    elif entry is None:
        reason = "is not in the cache"
    elif entry[1] != total or "sum" not in info:
        reason = "holds %d bytes, the argument has %d" % (entry[1], total)
    delta = None
    tensors = None
    alloc_error = None
    if reason is None and not converged:
        try:
            if delta_total:
                delta = _alloc_device_arg(
                    {"shape": [delta_total]}, torch.uint8, report, keep=base_key
                )
            tensors = _alloc_packed_tensors(info, report, keep=base_key)
        except Exception as e:  # noqa: BLE001 - e.g. out of HBM
            alloc_error = e  # drain mode below: the frame still has to go
            delta = None
    read_ms = ctypes.c_double()
    h2d_ms = ctypes.c_double()
    rc = lib.csp_h2d_stream_fd(
        0, ctypes.c_void_p(delta.data_ptr() if delta is not None else 0),
        delta_total, _packed_chunk(), -1,
        ctypes.byref(read_ms), ctypes.byref(h2d_ms),
    )
    stage["read_ms"] += read_ms.value
    stage["h2d_ms"] += h2d_ms.value
    if rc == 2:
        # the request stream is no longer aligned: leave, as _receive_device_arg does
        sys.stderr.write(
            "csp worker: csp_h2d_stream_fd lost the stream: %s\n"
            % lib.csp_last_error().decode(errors="replace")
        )
        sys.stderr.flush()
        os._exit(4)
    if rc == 0:
        stage["bytes"] += delta_total
    if converged:
        return _packed_args_from_cache(lib, index, info, total, new_key, stage, report)
    if reason is not None:
        _arg_cache_drop(base_key)
        report["miss"].append(index)
        raise RuntimeError(
            "argument buffer %d: cached argument %s %s" % (index, base_key, reason)
        )
    if alloc_error is not None:
        raise alloc_error
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: H2D copy failed (rc=%d): %s"
            % (index, rc, lib.csp_last_error().decode(errors="replace"))
        )
    segs = info["packed"]
    count = len(segs)
    sizes = [int(seg["nbytes"]) for seg in segs]
    changed = set(int(j) for j in cache["patch"]["segments"])
    unchanged = (1 << 64) - 1
    delta_offs = []
    patched_bytes = 0
    for j, n in enumerate(sizes):
        if j in changed:
            delta_offs.append(patched_bytes)
            patched_bytes += (n + 15) // 16 * 16
        else:
            delta_offs.append(unchanged)
    master = entry[0]
    dst = (ctypes.c_void_p * count)(
        *[(t.data_ptr() or None) if n else None for t, n in zip(tensors, sizes)]
    )
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    rc = lib.csp_patch_unpack_checksum_dev(
        ctypes.c_void_p(master.data_ptr() if total else 0), total,
        ctypes.c_void_p(delta.data_ptr() if delta is not None else 0), delta_total,
        dst, (ctypes.c_uint64 * count)(*[int(seg["offset"]) for seg in segs]),
        (ctypes.c_uint64 * count)(*sizes), (ctypes.c_uint64 * count)(*delta_offs),
        count, out, ctypes.byref(kernel_ms),
    )
    if rc != 0:
        _arg_cache_drop(base_key)
        raise RuntimeError(
            "argument buffer %d: csp_patch_unpack_checksum_dev failed: %s"
            % (index, lib.csp_last_error().decode(errors="replace"))
        )
    got = [int(out[0]), int(out[1])]
    want = [int(info["sum"][0]), int(info["sum"][1])]
    if got != want:
        _arg_cache_drop(base_key)
        report["miss"].append(index)
        raise RuntimeError(
            "argument buffer %d: cached argument %s patched to %s has checksum %r, "
            "the dispatcher sent %r" % (index, base_key, new_key, got, want)
        )
    # the same master under the new key, most recently used; the resident
    # bytes do not change
    del _arg_cache[base_key]
    _arg_cache[new_key] = (master, total, got)
    report["stored"].append(new_key)
    report.setdefault("patched", []).append([base_key, new_key])
    stage["mode"] = "pinned-h2d"
    stage["tensors"] += 1
    stage["verified"] += 1
    stage["packed_tensors"] = stage.get("packed_tensors", 0) + count
    stage["packed_bytes"] = stage.get("packed_bytes", 0) + sum(sizes)
    stage["patched_segments"] = stage.get("patched_segments", 0) + len(changed)
    stage["patched_bytes"] = stage.get("patched_bytes", 0) + delta_total
    stage["patch_ms"] = round(stage.get("patch_ms", 0.0) + kernel_ms.value, 3)
    return tensors


def _rebase_sources(info, cache, base_total):
    """Check a ``rebase`` entry's ``sources`` against its segments and the
    held base before anything is handed to the library: one source per
    segment, each -1 (from the delta) or a multiple of 16 whose rounded
    segment lies inside the base, and a delta whose layout totals
    ``rebase_nbytes``.  Returns (base offsets, delta offsets, segments from
    the delta) or raises ValueError."""
    sizes = [int(seg["nbytes"]) for seg in info["packed"]]
    sources = cache["rebase"].get("sources")
    if not isinstance(sources, (list, tuple)) or len(sources) != len(sizes):
        raise ValueError("sources do not match the %d segments" % len(sizes))
    none = (1 << 64) - 1
    base_offs, delta_offs = [], []
    delta_bytes = 0
    from_delta = 0
    for j, (src, n) in enumerate(zip(sources, sizes)):
        rounded = (n + 15) // 16 * 16
        if not isinstance(src, int) or isinstance(src, bool):
            raise ValueError("source %d is %r" % (j, src))
        if src == -1:
            base_offs.append(none)
            delta_offs.append(delta_bytes)
            delta_bytes += rounded
            from_delta += 1
        elif src >= 0 and src % 16 == 0 and src + rounded <= base_total:
            base_offs.append(src)
            delta_offs.append(none)
        else:
            raise ValueError(
                "source %d is %r for %d bytes of a base of %d" % (j, src, n, base_total)
            )
    if delta_bytes != int(info["rebase_nbytes"]):
        raise ValueError(
            "the delta has %d bytes, its segments need %d"
            % (int(info["rebase_nbytes"]), delta_bytes)
        )
    return base_offs, delta_offs, from_delta


def _rebase_packed_args(lib, index, info, total, cache, stage, report):
    """A ``rebase`` packed entry: the frame is a delta arena, the segments
    that the held arena ``base`` lacks, in the pack layout.  ONE
    csp_rebase_unpack_checksum_dev call takes every segment from the base (at
    the offset ``sources`` names) or from the delta, writes the new arena
    into a NEW master, scatters it into private tensors and yields its
    checksum.  The base is only read and stays in the cache under its own
    key, most recently used but for the new master.  When ARG_CACHE_BYTES
    cannot hold base and new together there is no new master (a transient
    rebase): the new key goes to ``not_stored`` and the electron still runs.
    The frame is consumed whatever happens.  An absent base, another byte
    count or no ``sum`` is a miss as in _packed_args_from_cache; after a
    checksum mismatch nobody can tell whether the base or the delta was
    wrong, so the base goes with the new master and it is a miss.  When the
    new key is already held the frame is only drained and the tensors come
    from the arena held under the new key."""
    global _arg_cache_resident
    import ctypes

    import torch

    new_key = cache["key"]
    base_key = cache["rebase"]["base"]
    delta_total = int(info["rebase_nbytes"])
    converged = new_key in _arg_cache
    entry = _arg_cache.get(base_key)
    reason = None
    plan = None
    if converged:
        pass
    elif entry is None:
        reason = "is not in the cache"
    elif entry[1] != int(cache["rebase"].get("base_nbytes", -1)) or "sum" not in info:
        reason = "holds %d bytes, the rebase names %r" % (
            entry[1], cache["rebase"].get("base_nbytes"))
    else:
        try:
            plan = _rebase_sources(info, cache, entry[1])
        except (ValueError, KeyError, TypeError) as e:
            reason = "cannot be the base: %s" % e
    delta = None
    tensors = None
    master = None
    alloc_error = None
    if reason is None and not converged:
        try:
            if delta_total:
                delta = _alloc_device_arg(
                    {"shape": [delta_total]}, torch.uint8, report, keep=base_key
                )
            tensors = _alloc_packed_tensors(info, report, keep=base_key)
        except Exception as e:  # noqa: BLE001 - e.g. out of HBM
            alloc_error = e  # drain mode below: the frame still has to go
            delta = None
        if alloc_error is None and base_key in _arg_cache:
            _arg_cache.move_to_end(base_key)
            if total:
                master = _arg_cache_new_master(total, report, keep=base_key)
    read_ms = ctypes.c_double()
    h2d_ms = ctypes.c_double()
    rc = lib.csp_h2d_stream_fd(
        0, ctypes.c_void_p(delta.data_ptr() if delta is not None else 0),
        delta_total, _packed_chunk(), -1,
        ctypes.byref(read_ms), ctypes.byref(h2d_ms),
    )
    stage["read_ms"] += read_ms.value
    stage["h2d_ms"] += h2d_ms.value
    if rc == 2:
        # the request stream is no longer aligned: leave, as _receive_device_arg does
        sys.stderr.write(
            "csp worker: csp_h2d_stream_fd lost the stream: %s\n"
            % lib.csp_last_error().decode(errors="replace")
        )
        sys.stderr.flush()
        os._exit(4)
    if rc == 0:
        stage["bytes"] += delta_total
    if converged:
        return _packed_args_from_cache(lib, index, info, total, new_key, stage, report)
    if reason is not None:
        _arg_cache_drop(base_key)
        report["miss"].append(index)
        raise RuntimeError(
            "argument buffer %d: cached argument %s %s" % (index, base_key, reason)
        )
    if alloc_error is not None:
        raise alloc_error
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: H2D copy failed (rc=%d): %s"
            % (index, rc, lib.csp_last_error().decode(errors="replace"))
        )
    entry = _arg_cache.get(base_key)
    if entry is None:
        # the private tensors needed the base's memory (out of HBM)
        report["miss"].append(index)
        raise RuntimeError(
            "argument buffer %d: cached argument %s had to go for the electron's tensors"
            % (index, base_key)
        )
    base_offs, delta_offs, from_delta = plan
    segs = info["packed"]
    count = len(segs)
    sizes = [int(seg["nbytes"]) for seg in segs]
    dst = (ctypes.c_void_p * count)(
        *[(t.data_ptr() or None) if n else None for t, n in zip(tensors, sizes)]
    )
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    rc = lib.csp_rebase_unpack_checksum_dev(
        ctypes.c_void_p(entry[0].data_ptr() if entry[1] else 0), entry[1],
        ctypes.c_void_p(delta.data_ptr() if delta is not None else 0), delta_total,
        ctypes.c_void_p(master.data_ptr() if master is not None else 0), total,
        dst, (ctypes.c_uint64 * count)(*[int(seg["offset"]) for seg in segs]),
        (ctypes.c_uint64 * count)(*sizes), (ctypes.c_uint64 * count)(*base_offs),
        (ctypes.c_uint64 * count)(*delta_offs), count, out, ctypes.byref(kernel_ms),
    )
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: csp_rebase_unpack_checksum_dev failed: %s"
            % (index, lib.csp_last_error().decode(errors="replace"))
        )
    got = [int(out[0]), int(out[1])]
    want = [int(info["sum"][0]), int(info["sum"][1])]
    if got != want:
        master = None
        _arg_cache_drop(base_key)
        report["miss"].append(index)
        raise RuntimeError(
            "argument buffer %d: cached argument %s rebased to %s has checksum %r, "
            "the dispatcher sent %r" % (index, base_key, new_key, got, want)
        )
    if master is not None:
        _arg_cache[new_key] = (master, total, got)  # most recently used
        _arg_cache_resident += total
        report["stored"].append(new_key)
    else:
        report["not_stored"].append(new_key)
    report.setdefault("rebased", []).append([base_key, new_key])
    stage["mode"] = "pinned-h2d"
    stage["tensors"] += 1
    stage["verified"] += 1
    stage["packed_tensors"] = stage.get("packed_tensors", 0) + count
    stage["packed_bytes"] = stage.get("packed_bytes", 0) + sum(sizes)
    stage["rebased_segments"] = stage.get("rebased_segments", 0) + from_delta
    stage["rebased_bytes"] = stage.get("rebased_bytes", 0) + delta_total
    stage["rebase_ms"] = round(stage.get("rebase_ms", 0.0) + kernel_ms.value, 3)
    return tensors


def _receive_packed_device_args(index, info, stage, report):
    """Persistent mode: a ``packed`` device entry.  Its one frame lands in
    HBM as one arena through csp_h2d_stream_fd, and ONE
    csp_unpack_checksum_dev call scatters the arena into a private tensor per
    segment and yields the arena's checksum.  Returns the list of tensors.

    With ``"cache": {"key", "store": true}`` the arena is a new master that
    stays in HBM under the key; with ``{"key", "ref": true}`` there is no
    frame and the tensors are unpacked from the master already held
    (_packed_args_from_cache); with ``{"key", "patch": {"base", "segments"}}``
    the frame is a delta that is applied to the master held under ``base``
    (_patch_packed_args); with ``{"key", "rebase": {"base", "base_nbytes",
    "sources"}}`` the frame is a delta from which, with the master held under
    ``base``, a new master is built (_rebase_packed_args).  A transient arena is let go before user code
    runs.  Whatever goes wrong short of a broken stream, the frame is
    consumed before the error is raised, as in _receive_device_arg."""
    global _arg_cache_resident
    import ctypes

    cache = info.get("cache") or {}
    total = int(info["nbytes"])
    try:
        lib = _device_arg_lib()
    except RuntimeError:
        if not cache.get("ref") and _read_frame(0) is None:  # drain with the Python reader
            os._exit(4)
        raise
    import torch

    # the library's copy stream does not wait on the null stream
    torch.cuda.synchronize()
    if cache.get("ref"):
        return _packed_args_from_cache(
            lib, index, info, total, cache["key"], stage, report
        )
    if cache.get("patch"):
        return _patch_packed_args(lib, index, info, total, cache, stage, report)
    if cache.get("rebase"):
        return _rebase_packed_args(lib, index, info, total, cache, stage, report)
    key = None
    master = None
    if cache.get("store") and "sum" in info and total:
        key = cache["key"]
        if key in _arg_cache:
            # the frame is on its way all the same: it lands in a transient arena
            _arg_cache.move_to_end(key)
            report["stored"].append(key)
            key = None
        else:
            master = _arg_cache_new_master(total, report)
            if master is None:
                report["not_stored"].append(key)
    alloc_error = None
    arena = master
    tensors = None
    try:
        if arena is None:
            arena = _alloc_device_arg({"shape": [total]}, torch.uint8, report)
        tensors = _alloc_packed_tensors(info, report)
    except Exception as e:  # noqa: BLE001 - e.g. out of HBM
        alloc_error = e  # drain mode below: the frame still has to go
        if master is not None:
            report["not_stored"].append(key)
        arena = master = None
    read_ms = ctypes.c_double()
    h2d_ms = ctypes.c_double()
    rc = lib.csp_h2d_stream_fd(
        0, ctypes.c_void_p(arena.data_ptr() if (arena is not None and total) else 0),
        total, min(STREAM_CHUNK, PACKED_ARG_CHUNK) if STREAM_CHUNK > 0 else PACKED_ARG_CHUNK, -1,
        ctypes.byref(read_ms), ctypes.byref(h2d_ms),
    )
    stage["read_ms"] += read_ms.value
    stage["h2d_ms"] += h2d_ms.value
    if rc == 2:
        # the request stream is no longer aligned: leave, as _receive_device_arg does
        sys.stderr.write(
            "csp worker: csp_h2d_stream_fd lost the stream: %s\n"
            % lib.csp_last_error().decode(errors="replace")
        )
        sys.stderr.flush()
        os._exit(4)
    if alloc_error is not None:
        raise alloc_error
    if rc != 0:
        raise RuntimeError(
            "argument buffer %d: H2D copy failed (rc=%d): %s"
            % (index, rc, lib.csp_last_error().decode(errors="replace"))
        )
    got = _unpack_arena(lib, index, arena, total, info, tensors, stage)
    stage["mode"] = "pinned-h2d"
    stage["tensors"] += 1
    stage["bytes"] += total
    if "sum" in info:
        stage["verified"] += 1
        _compare_arg_sum(index, got, info, total)  # a mismatch drops the master
    if master is not None:
        _arg_cache[key] = (master, total, got)
        _arg_cache_resident += total
        report["stored"].append(key)
    return tensors


def _receive_arg_frames(arg_meta):
    """Read the request's out-of-band argument frames.  Returns
    (frames, stage, error, cache_report); frames is None when stdin ended,
    cache_report is None unless an entry carries ``"cache"``.  A frame is a
    bytearray (host) or, for a device entry in persistent mode, the CUDA
    tensor itself (for a ``packed`` entry the list of its CUDA tensors).
    The first per-argument error is kept and EVERY frame
    is still consumed, so the stream stays aligned.

    In isolate mode this process is the zygote and must not touch HIP:
    device entries are read to host memory like the others and the forked
    child moves them (_device_args_in_child)."""
    frames = []
    stage = _new_arg_stage()
    error = None
    report = None
    if any(info.get("cache") for info in arg_meta):
        report = _new_arg_cache_report()
    for index, info in enumerate(arg_meta):
        if info.get("device") and not ISOLATE:
            receive = (
                _receive_packed_device_args if "packed" in info else _receive_device_arg
            )
            try:
                frames.append(
                    receive(index, info, stage, report or _new_arg_cache_report())
                )
            except Exception as e:  # noqa: BLE001
                frames.append(None)
                if error is None:
                    error = e
            continue
        f = _read_frame(0)
        if f is None:
            return None, stage, error, report
        frames.append(bytearray(f))
    if report is not None:
        report["entries"] = len(_arg_cache)
        report["resident_bytes"] = _arg_cache_resident
    return frames, stage, error, report


def _device_args_in_child(frames, meta_list, stage):
    """Isolate mode, in the forked child after its prologue: move every
    device-flagged argument buffer (in host memory, read by the zygote) to
    the GPU and verify it there.  A pinned ring here would only repeat what
    torch's own pageable copy does (stage through pinned memory, chunk by
    chunk), and the receive it could overlap with is already over, so this
    is a plain ``.cuda()``."""
    flagged = [i for i, info in enumerate(meta_list) if info.get("device")]
    if not flagged:
        return
    lib = _device_arg_lib()
    import torch

    for i in flagged:
        info = meta_list[i]
        if "packed" in info:
            # one .cuda() for the arena, then the same single unpack call
            total = int(info["nbytes"])
            t0 = time.monotonic()
            if len(frames[i]) != total:
                raise RuntimeError(
                    "argument buffer %d: the packed frame has %d bytes, its "
                    "entry announces %d" % (i, len(frames[i]), total)
                )
            arena = torch.frombuffer(frames[i], dtype=torch.uint8).cuda()
            tensors = _alloc_packed_tensors(info, _new_arg_cache_report())
            # the library's copy stream does not wait on the null stream
            torch.cuda.synchronize()
            stage["h2d_ms"] += (time.monotonic() - t0) * 1000
            got = _unpack_arena(lib, i, arena, total, info, tensors, stage)
            stage["mode"] = "isolated-copy"
            stage["tensors"] += 1
            stage["bytes"] += total
            if "sum" in info:
                stage["verified"] += 1
                _compare_arg_sum(i, got, info, total)
            del arena
            frames[i] = tensors
            continue
        dtype = getattr(torch, info["dtype"])
        t0 = time.monotonic()
        if len(frames[i]) == 0:
            tensor = torch.empty(info["shape"], dtype=dtype, device="cuda")
        else:
            tensor = (
                torch.frombuffer(frames[i], dtype=dtype).reshape(info["shape"]).cuda()
            )
        # the library's copy stream does not wait on the null stream
        torch.cuda.synchronize()
        stage["h2d_ms"] += (time.monotonic() - t0) * 1000
        nbytes = tensor.numel() * tensor.element_size()
        stage["mode"] = "isolated-copy"
        stage["tensors"] += 1
        stage["bytes"] += nbytes
        _verify_device_arg(lib, i, tensor, nbytes, info, stage)
        frames[i] = tensor


def _rebuild_arg_tensors(obj, buffers, meta_list):
    """Mirror of the dispatcher-side marker walk for request buffers."""
    import torch

    def build(i):
        if isinstance(buffers[i], torch.Tensor):
            return buffers[i]  # a device argument, already in HBM
        info = meta_list[i]
        dtype = getattr(torch, info["dtype"])
        if len(buffers[i]) == 0:
            return torch.empty(info["shape"], dtype=dtype)
        return torch.frombuffer(buffers[i], dtype=dtype).reshape(info["shape"])

    def walk(o):
        if isinstance(o, tuple) and len(o) == 2 and o[0] == "__csp_tensor_buffer_v1__":
            return build(o[1])
        if (
            isinstance(o, tuple)
            and len(o) == 3
            and isinstance(o[0], str)
            and o[0] == "__csp_packed_tensor_v1__"
        ):
            # tensor j of packed entry i: a marker met twice gives the same
            # object, as the dispatcher had it
            return buffers[o[1]][o[2]]
        if isinstance(o, dict):
            return {k: walk(v) for k, v in o.items()}
        if isinstance(o, tuple):
            vals = [walk(v) for v in o]
            return type(o)(*vals) if hasattr(o, "_fields") else tuple(vals)
        if isinstance(o, list):
            return [walk(v) for v in o]
        return o

    return walk(obj)


def _serve_one(request):
    global _served
    _served += 1
    if TELEMETRY_EVERY > 0 and _served % TELEMETRY_EVERY == 1 % TELEMETRY_EVERY:
        _sample_hbm()
    t0 = time.monotonic()
    meta = {"phases_ms": {}, "gpu": _gpu_info, "staging": None,
            "hbm": _last_mem,
            "gpu_slot": GPU_SLOT, "buffers": [],
            "hip_visible_devices": os.environ.get("HIP_VISIBLE_DEVICES"),
            "pid": os.getpid(), "worker": True, "served": _served}
    arg_stage = request.get("_arg_staging") or _new_arg_stage()
    meta["arg_staging"] = arg_stage
    if request.get("_arg_cache") is not None:
        meta["arg_cache"] = request["_arg_cache"]
    result = None
    exception = None
    buffers = []
    retain = None  # retention on and a result to stage: {"op_id", "report"}
    try:
        if request.get("_arg_error") is not None:
            # an argument frame was consumed but could not be delivered:
            # the electron fails with that error, user code does not run
            raise request["_arg_error"]
        fn, args, kwargs = pickle.loads(request["function_blob"])
        arg_bufs = request.get("_arg_buffer_frames") or []
        if arg_bufs:
            if ISOLATE:
                _device_args_in_child(arg_bufs, request["arg_buffers"], arg_stage)
            args = _rebuild_arg_tensors(args, arg_bufs, request["arg_buffers"])
            kwargs = _rebuild_arg_tensors(kwargs, arg_bufs, request["arg_buffers"])
    except Exception as e:  # noqa: BLE001
        exception = e
        fn = None
    for key in ("read_ms", "h2d_ms"):
        arg_stage[key] = round(arg_stage[key], 3)

    home = os.getcwd()
    if exception is None:
        workdir = request.get("workdir") or "."
        try:
            os.makedirs(workdir, exist_ok=True)
            os.chdir(workdir)
        except OSError as e:
            exception = e

    if exception is None:
        t_fn = time.monotonic()
        # capture the task's python-level stdout/stderr into the meta
        # (fd-level output still flows to the worker's stderr stream)
        import contextlib
        import io as _io

        out_buf, err_buf = _io.StringIO(), _io.StringIO()
        try:
            with contextlib.redirect_stdout(out_buf), contextlib.redirect_stderr(err_buf):
                result = fn(*args, **kwargs)
        except Exception as e:  # noqa: BLE001
            exception = e
        meta["phases_ms"]["user_fn"] = round((time.monotonic() - t_fn) * 1000, 3)
        meta["stdout"] = out_buf.getvalue()[-65536:]
        meta["stderr"] = err_buf.getvalue()[-65536:]
        if meta["stdout"]:
            sys.stderr.write(meta["stdout"])
        if meta["stderr"]:
            sys.stderr.write(meta["stderr"])
    os.chdir(home)

    if exception is None and result is not None:
        t_stage = time.monotonic()
        stats = {"tensors": 0, "pinned_tensors": 0, "bytes": 0, "mode": "none"}
        if PACK_RESULTS:
            stats["packed_tensors"] = 0
            stats["packed_bytes"] = 0
        if RETAIN_MIN_BYTES >= 0 and ARG_CACHE_BYTES > 0 and not ISOLATE:
            retain = {"op_id": request.get("op_id"),
                      "report": {"stored": [], "not_stored": [], "evicted": []}}
            stats.update(retained_buffers=0, retained_bytes=0, retain_ms=0.0)
            meta["retained"] = retain["report"]
        try:
            result = _stage_result(result, stats, buffers, meta["buffers"], retain)
            meta["staging"] = stats
        except Exception as e:  # noqa: BLE001
            result, exception, buffers = None, e, []
            meta["buffers"] = []
            if retain is not None:
                _retain_rollback(retain)
        meta["phases_ms"]["staging"] = round((time.monotonic() - t_stage) * 1000, 3)

    try:
        result_blob = pickle.dumps((result, exception))
    except Exception as e:  # noqa: BLE001
        result_blob = pickle.dumps((None, e))
        buffers = []
        meta["buffers"] = []
        if retain is not None:
            _retain_rollback(retain)
    meta["phases_ms"]["total"] = round((time.monotonic() - t0) * 1000, 3)
    return result_blob, meta, buffers


def _serve_isolated(request):
    """Run one electron in a freshly forked child (fresh-process
    semantics: no state, no HIP context, no module cache survives into
    the next electron).  The child writes its response frames to a pipe;
    the parent relays them frame-by-frame so a child crash can never
    leave a half-written frame on the protocol stream."""
    global _served
    _served += 1
    serial = _served
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        # ---- child: the per-task process ----
        os.close(r)
        try:
            import ctypes

            libc = ctypes.CDLL(None, use_errno=True)
            libc.prctl(1, 9, 0, 0, 0)  # PR_SET_PDEATHSIG=SIGKILL: die with parent
        except Exception:  # noqa: BLE001
            pass
        wrote_reply = False
        try:
            if GPU_LIB and GPU_SLOT is not None and DO_WARMUP:
                _prologue()  # fresh HIP init belongs to THIS child
            result_blob, meta, buffers = _serve_one(request)
            meta["isolated"] = True
            meta["served"] = serial
            _write_frame(w, pickle.dumps(("R1", result_blob, meta, len(buffers))))
            wrote_reply = True
            for view, _keep in buffers:
                _send_buffer(w, view)
        except BaseException as e:  # noqa: BLE001 - report anything reportable
            # Fallback error reply ONLY if the real R1 never went out: a
            # failure mid-buffer-stream must NOT append a second R1 that
            # the parent would miscount as a raw buffer frame (the parent
            # detects the short stream and drops the channel instead).
            if not wrote_reply:
                try:
                    blob = pickle.dumps(
                        (None, RuntimeError(f"isolated task failed: {e!r}"))
                    )
                    _write_frame(
                        w,
                        pickle.dumps(
                            ("R1", blob, {"phases_ms": {}, "isolated": True}, 0)
                        ),
                    )
                except BaseException:  # noqa: BLE001
                    pass
        os._exit(0)

    # ---- parent: frame-by-frame relay ----
    os.close(w)
    relayed = 0
    expected = None
    while True:
        frame = _read_frame(r)
        if frame is None or frame == b"":
            break
        if relayed == 0:
            _tag, _blob, _meta, nbuf = pickle.loads(frame)
            expected = 1 + nbuf
        _write_frame(_proto_fd, frame)
        relayed += 1
        if expected is not None and relayed >= expected:
            break
    os.close(r)
    _, status = os.waitpid(pid, 0)
    if relayed == 0:
        # child died before completing even the main response frame:
        # synthesize the error so the electron fails cleanly and the
        # zygote keeps serving (no worker respawn needed)
        blob = pickle.dumps(
            (None, RuntimeError(
                f"isolated task process died (wait status {status}) "
                "before reporting a result"
            ))
        )
        _write_frame(
            _proto_fd,
            pickle.dumps(("R1", blob, {"phases_ms": {}, "isolated": True,
                                       "served": serial}, 0)),
        )
    elif expected is not None and relayed < expected:
        # partial multi-frame response already relayed: the stream is
        # unrecoverable — exit so the dispatcher sees ChannelClosed
        os._exit(4)


def main():
    startup_meta = {"pid": os.getpid(), "gpu": None, "error": None,
                    "gpu_slot": GPU_SLOT, "isolate": ISOLATE,
                    "hip_visible_devices": os.environ.get("HIP_VISIBLE_DEVICES")}
    if ISOLATE:
        # zygote warm-up: bind the configured imports pre-fork, but
        # touch NO GPU state (HIP contexts do not survive fork)
        if ISOLATE_PRELOAD == "torch":
            try:
                import importlib.util

                if importlib.util.find_spec("torch") is not None:
                    import torch  # noqa: F401
            except Exception as e:  # noqa: BLE001
                startup_meta["error"] = repr(e)
    elif GPU_LIB and GPU_SLOT is not None:
        try:
            _prologue()
            startup_meta["gpu"] = _gpu_info
        except Exception as e:  # noqa: BLE001
            startup_meta["error"] = repr(e)
    _write_frame(_proto_fd, pickle.dumps(("READY", startup_meta)))
    if startup_meta["error"]:
        sys.exit(3)

    while True:
        frame = _read_frame(0, idle_timeout=IDLE_TIMEOUT)
        if frame is None or frame == b"":
            break
        request = pickle.loads(frame)
        arg_meta = request.get("arg_buffers") or []
        if arg_meta:
            frames, arg_stage, arg_error, cache_report = _receive_arg_frames(arg_meta)
            if frames is None:
                return
            request["_arg_buffer_frames"] = frames
            request["_arg_staging"] = arg_stage
            request["_arg_cache"] = cache_report
            request["_arg_error"] = arg_error
        # ack AFTER the full request is in hand, BEFORE user code runs:
        # the dispatcher's retry-on-death policy keys off this frame
        _write_frame(_proto_fd, pickle.dumps(("A1", request.get("op_id"))))
        if ISOLATE:
            _serve_isolated(request)
            continue
        result_blob, meta, buffers = _serve_one(request)
        _write_frame(_proto_fd, pickle.dumps(("R1", result_blob, meta, len(buffers))))
        for view, _keep in buffers:
            _send_buffer(_proto_fd, view)
        del buffers
        request = None  # lets go of device arguments before the next wait
        if _gpu_lib is not None:
            _gpu_lib.csp_staging_release_all()


if __name__ == "__main__":
    main()
