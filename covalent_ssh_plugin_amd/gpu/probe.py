"""ctypes bindings to the in-tree CDNA4 GPU library (libcsp_gpu.so).

The library (covalent_ssh_plugin_amd/ops/hip/csp_gpu.hip, built for
gfx950 only) provides:

* ``csp_probe_json`` — device probe: properties + measured HBM bandwidth
  and bf16 MFMA throughput from the hand-written warm-up kernels,
* ``csp_warmup`` — clock/cache warm-up spin (MFMA + HBM sweep),
* ``csp_staging_get`` / ``csp_host_alloc`` / ``csp_host_free`` /
  ``csp_memcpy_d2h`` / ``csp_memcpy_h2d`` — hipHostMalloc-pinned staging,
* ``csp_d2h_stream_fd`` / ``csp_h2d_stream_fd`` — one framed tensor buffer
  between device memory and a channel fd, the copy overlapped with the I/O,
* ``csp_checksum_dev`` — the argument checksum over bytes in HBM,
* ``csp_pack_dev`` — many small device buffers gathered into one contiguous
  zero-padded arena by one kernel launch (``pack_tensor_results``),
* ``csp_pack_checksum_dev`` — the same gather with the arena's checksum from
  the same launch (``retain_tensor_results``),
* ``csp_unpack_checksum_dev`` — such an arena scattered into private
  per-tensor buffers and checksummed by one kernel launch
  (``pack_tensor_args``),
* ``csp_patch_unpack_checksum_dev`` — the same launch on a held arena, with
  the changed segments written over it in place from a small delta arena
  (``patch_tensor_args``),
* ``csp_rebase_unpack_checksum_dev`` — the same launch for a new arena of any
  layout, each segment from a held arena or from a small delta arena, written
  out as a new master while the held one is only read
  (``rebase_tensor_args``),
* ``csp_hbm_sweep_dev`` — one launch of the probe's HBM sweep kernel on the
  caller's buffers, and ``csp_checksum_grid_cap`` /
  ``csp_copy_checksum_grid_cap`` / ``csp_unpack_checksum_grid_cap`` (tools
  and tests only).

On a GPU box these bindings FAIL LOUDLY if the extension is missing or
broken — there is no eager/CPU fallback for the device path.
"""

from __future__ import annotations

import ctypes
import json
import os
from pathlib import Path
from typing import Optional

_LIB_NAME = "libcsp_gpu.so"
_lib: Optional[ctypes.CDLL] = None


class GpuLibError(RuntimeError):
    """The CDNA4 GPU extension is missing or a call into it failed."""


def local_gpu_lib_path() -> str:
    """Path of the built in-tree library, or '' if not built."""
    candidate = Path(__file__).resolve().parent.parent / "ops" / _LIB_NAME
    return str(candidate) if candidate.exists() else ""


def load(path: str = "") -> ctypes.CDLL:
    """Load (once) and return the GPU library with typed signatures."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = path or local_gpu_lib_path()
    if not lib_path:
        raise GpuLibError(
            f"{_LIB_NAME} not built — run __graft_entry__.build() / "
            "python -m covalent_ssh_plugin_amd.ops.build"
        )
    # One HSA runtime per process: bind torch's bundled ROCm runtime
    # first when torch is installed, so this library shares it instead of
    # initializing the system runtime (which would break a later
    # torch.cuda init with "No HIP GPUs are available").
    import importlib.util

    if importlib.util.find_spec("torch") is not None:
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
    lib = ctypes.CDLL(lib_path)

    lib.csp_device_count.restype = ctypes.c_int
    lib.csp_probe_json.restype = ctypes.c_int
    lib.csp_probe_json.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.csp_probe_props_json.restype = ctypes.c_int
    lib.csp_probe_props_json.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.csp_warmup.restype = ctypes.c_int
    lib.csp_warmup.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.csp_host_alloc.restype = ctypes.c_void_p
    lib.csp_host_alloc.argtypes = [ctypes.c_size_t]
    lib.csp_host_free.restype = ctypes.c_int
    lib.csp_host_free.argtypes = [ctypes.c_void_p]
    lib.csp_staging_get.restype = ctypes.c_void_p
    lib.csp_staging_get.argtypes = [ctypes.c_size_t]
    lib.csp_staging_alloc.restype = ctypes.c_void_p
    lib.csp_staging_alloc.argtypes = [ctypes.c_size_t]
    lib.csp_staging_release_all.restype = ctypes.c_int
    lib.csp_staging_reset.restype = ctypes.c_int
    lib.csp_memcpy_d2h.restype = ctypes.c_int
    lib.csp_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.csp_memcpy_h2d.restype = ctypes.c_int
    lib.csp_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
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
        ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64),
    ]
    lib.csp_copy_checksum_dev.restype = ctypes.c_int
    lib.csp_copy_checksum_dev.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
    ]
    lib.csp_copy_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_copy_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_set_sweep_variant.restype = None
    lib.csp_set_sweep_variant.argtypes = [ctypes.c_int]
    lib.csp_hbm_sweep_dev.restype = ctypes.c_int
    lib.csp_hbm_sweep_dev.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
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
    lib.csp_pack_tile_bytes.restype = ctypes.c_size_t
    lib.csp_pack_tile_bytes.argtypes = []
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
    lib.csp_pack_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_pack_checksum_grid_cap.argtypes = [ctypes.c_size_t]
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
    lib.csp_unpack_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_unpack_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_mem_info.restype = ctypes.c_int
    lib.csp_mem_info.argtypes = [
        ctypes.c_int,
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_last_error.restype = ctypes.c_char_p

    _lib = lib
    return lib


def _check(lib: ctypes.CDLL, rc: int, what: str) -> None:
    if rc != 0:
        err = lib.csp_last_error().decode(errors="replace")
        raise GpuLibError(f"{what} failed (rc={rc}): {err}")


def device_count() -> int:
    lib = load()
    n = lib.csp_device_count()
    if n < 0:
        _check(lib, n, "csp_device_count")
    return n


def probe(device: int = 0) -> dict:
    """Probe + measure one GPU.  Returns the JSON dict produced by the
    HIP library (name, gfx arch, CUs, HBM size/bandwidth, bf16 MFMA
    TFLOP/s from the warm-up kernels)."""
    lib = load()
    buf = ctypes.create_string_buffer(8192)
    _check(lib, lib.csp_probe_json(device, buf, len(buf)), "csp_probe_json")
    return json.loads(buf.value.decode())


def probe_props(device: int = 0) -> dict:
    """Device properties only (no measurement kernels, no big allocs)."""
    lib = load()
    buf = ctypes.create_string_buffer(8192)
    _check(lib, lib.csp_probe_props_json(device, buf, len(buf)), "csp_probe_props_json")
    return json.loads(buf.value.decode())


def mem_info(device: int = 0) -> dict:
    """HBM occupancy via csp_mem_info (the per-task telemetry call)."""
    lib = load()
    free_gb = ctypes.c_double()
    total_gb = ctypes.c_double()
    _check(lib, lib.csp_mem_info(device, ctypes.byref(free_gb), ctypes.byref(total_gb)),
           "csp_mem_info")
    return {"hbm_free_gb": free_gb.value, "hbm_total_gb": total_gb.value}


def warmup(device: int = 0, budget_ms: int = 50) -> None:
    lib = load()
    _check(lib, lib.csp_warmup(device, budget_ms), "csp_warmup")


# csp_d2h_stream_fd return codes
STREAM_OK = 0
STREAM_FAILED_BEFORE_HEADER = 1
STREAM_FAILED_MID_FRAME = 2


def stream_d2h_to_fd(fd: int, data_ptr: int, nbytes: int, chunk_bytes: int = 0) -> dict:
    """Frame ``nbytes`` at device pointer ``data_ptr`` onto ``fd`` (8-byte
    big-endian length, then the bytes), the D2H copy overlapped with the
    writes through the two-chunk pinned ring.  ``chunk_bytes`` 0 takes the
    library default.  Returns ``{"rc", "d2h_ms", "write_ms"}``; a non-zero
    ``rc`` is one of the STREAM_FAILED_* codes, not an exception — the
    caller decides what a cut-short frame means for its stream."""
    lib = load()
    d2h_ms = ctypes.c_double()
    write_ms = ctypes.c_double()
    rc = lib.csp_d2h_stream_fd(
        fd, ctypes.c_void_p(data_ptr), nbytes, chunk_bytes,
        ctypes.byref(d2h_ms), ctypes.byref(write_ms),
    )
    return {"rc": rc, "d2h_ms": d2h_ms.value, "write_ms": write_ms.value}


# csp_h2d_stream_fd return codes
H2D_OK = 0
H2D_FAILED_DRAINED = 1  # a HIP call failed; the frame was still consumed
H2D_FAILED_STREAM = 2  # EOF, I/O error, timeout, header mismatch


def stream_fd_to_device(
    fd: int, data_ptr: int, nbytes: int, chunk_bytes: int = 0, timeout_ms: int = -1
) -> dict:
    """Read one frame (8-byte big-endian length, which must equal
    ``nbytes``, then the bytes) from ``fd`` into device memory at
    ``data_ptr``, the H2D copy overlapped with the reads through the
    two-chunk pinned ring.  ``data_ptr`` 0 consumes and discards the frame.
    ``timeout_ms`` bounds each wait for the next byte; negative means no
    limit.  Returns ``{"rc", "read_ms", "h2d_ms"}``; ``rc`` is one of the
    H2D_* codes, not an exception: only the caller knows what an unaligned
    stream means for it."""
    lib = load()
    read_ms = ctypes.c_double()
    h2d_ms = ctypes.c_double()
    rc = lib.csp_h2d_stream_fd(
        fd, ctypes.c_void_p(data_ptr), nbytes, chunk_bytes, timeout_ms,
        ctypes.byref(read_ms), ctypes.byref(h2d_ms),
    )
    return {"rc": rc, "read_ms": read_ms.value, "h2d_ms": h2d_ms.value}


def checksum_device(data_ptr: int, nbytes: int) -> tuple:
    """``(s0, s1)`` of ``nbytes`` at the 16-byte aligned device pointer
    ``data_ptr``: the same two numbers as ``native_io.checksum`` over the
    same bytes.  Runs on the library's copy stream; data written on another
    stream must be complete (``torch.cuda.synchronize()``) first."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    _check(lib, lib.csp_checksum_dev(ctypes.c_void_p(data_ptr), nbytes, out),
           "csp_checksum_dev")
    return int(out[0]), int(out[1])


def copy_checksum_device(dst_ptr: int, src_ptr: int, nbytes: int) -> tuple:
    """Copy ``nbytes`` from device pointer ``src_ptr`` to device pointer
    ``dst_ptr`` and return ``(s0, s1)`` of those bytes, the same two numbers
    as :func:`checksum_device`, from one pass over HBM (``cache_tensor_args``:
    a cached master's private copy for one electron).  Both pointers must be
    16-byte aligned and the ranges disjoint; a violation raises
    ``GpuLibError`` and launches nothing.  Runs on the library's copy stream;
    work on the two buffers on another stream must be complete
    (``torch.cuda.synchronize()``) first."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    _check(
        lib,
        lib.csp_copy_checksum_dev(
            ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), nbytes, out
        ),
        "csp_copy_checksum_dev",
    )
    return int(out[0]), int(out[1])


def copy_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`copy_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_copy_checksum_grid_cap(int(cap)))


def checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`checksum_device` (0 restores
    the shipped default of 1024 blocks).  Returns the cap in effect."""
    return int(load().csp_checksum_grid_cap(int(cap)))


SWEEP_VARIANT_DEFAULT = 2
# float4 vectors in flight per lane for each sweep variant; any other
# variant number runs variant 0
SWEEP_UNROLL = {0: 1, 1: 4, 2: 1, 3: 4, 4: 8}


def set_sweep_variant(variant: int = SWEEP_VARIANT_DEFAULT) -> None:
    """Tools only: the HBM sweep variant that the probe, the warm-up and
    ``hbm_sweep_device(-1, ...)`` run from now on."""
    load().csp_set_sweep_variant(int(variant))


def hbm_sweep_device(variant: int, src_ptr: int, dst_ptr: int, n4: int, blocks: int = 1024) -> None:
    """One launch of the probe's HBM sweep kernel: ``n4`` 16-byte vectors
    from device pointer ``src_ptr`` to device pointer ``dst_ptr`` (both
    16-byte aligned) with ``blocks`` blocks of 256 lanes, complete on return.
    ``variant`` -1 is the one the probe measures with; a number outside
    ``SWEEP_UNROLL`` runs variant 0.  Runs on the null stream.  A misaligned
    pointer or ``blocks < 1`` raises ``GpuLibError`` and launches nothing."""
    lib = load()
    _check(
        lib,
        lib.csp_hbm_sweep_dev(
            int(variant), ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), n4, int(blocks)
        ),
        "csp_hbm_sweep_dev",
    )


PACK_ALIGN = 16  # every packed segment starts on a multiple of this


def pack_layout(sizes) -> tuple:
    """``(offsets, arena_bytes)`` for segments of ``sizes`` bytes under the
    layout rule of ``csp_pack_dev``: the first at 0, each next one after the
    previous size rounded up to 16."""
    offsets = []
    total = 0
    for n in sizes:
        offsets.append(total)
        total += (int(n) + PACK_ALIGN - 1) // PACK_ALIGN * PACK_ALIGN
    return offsets, total


def pack_tile_bytes() -> int:
    """Bytes of one segment that one block moves per trip of the pack kernel."""
    return int(load().csp_pack_tile_bytes())


def pack_device(segments, arena_ptr: int, arena_bytes: int) -> dict:
    """Gather ``segments``, a sequence of ``(src_ptr, dst_off, nbytes)`` with
    device pointers, into the 16-byte aligned device arena at ``arena_ptr``
    with one kernel launch.  The offsets must follow :func:`pack_layout` and
    ``arena_bytes`` must be its total; a violation raises ``GpuLibError`` and
    launches nothing.  Afterwards every arena byte outside a segment is zero.
    Runs on the library's copy stream; sources written on another stream must
    be complete (``torch.cuda.synchronize()``) first.  Returns
    ``{"kernel_ms": ...}``, the kernel alone."""
    lib = load()
    n = len(segments)
    src = (ctypes.c_void_p * n)(*[int(s[0]) or None for s in segments])
    off = (ctypes.c_uint64 * n)(*[int(s[1]) for s in segments])
    size = (ctypes.c_uint64 * n)(*[int(s[2]) for s in segments])
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_pack_dev(src, off, size, n, ctypes.c_void_p(arena_ptr), arena_bytes,
                         ctypes.byref(kernel_ms)),
        "csp_pack_dev",
    )
    return {"kernel_ms": kernel_ms.value}


def pack_checksum_device(segments, arena_ptr: int, arena_bytes: int) -> dict:
    """:func:`pack_device` and :func:`checksum_device` of the arena in ONE
    kernel launch (``retain_tensor_results``): every 16-byte vector is
    assembled once, stored once and summed as stored.  One segment is a
    checksummed copy from a source of any alignment.  Refuses what
    :func:`pack_device` refuses and also an ``arena_bytes`` above 16 GiB and a
    source range that overlaps the arena (``GpuLibError``, nothing launched).
    Returns ``{"sum": (s0, s1), "kernel_ms": ...}``, the kernel alone.  Runs
    on the library's copy stream; sources written on another stream must be
    complete (``torch.cuda.synchronize()``) first."""
    lib = load()
    n = len(segments)
    src = (ctypes.c_void_p * n)(*[int(s[0]) or None for s in segments])
    off = (ctypes.c_uint64 * n)(*[int(s[1]) for s in segments])
    size = (ctypes.c_uint64 * n)(*[int(s[2]) for s in segments])
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_pack_checksum_dev(
            src, off, size, n, ctypes.c_void_p(arena_ptr or None), arena_bytes, out,
            ctypes.byref(kernel_ms),
        ),
        "csp_pack_checksum_dev",
    )
    return {"sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def pack_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`pack_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_pack_checksum_grid_cap(int(cap)))


def unpack_checksum_device(arena_ptr: int, arena_bytes: int, segments) -> dict:
    """Scatter the 16-byte aligned device arena at ``arena_ptr`` into
    ``segments``, a sequence of ``(dst_ptr, src_off, nbytes)`` with 16-byte
    aligned device pointers, and checksum the whole arena in the same kernel
    launch (``pack_tensor_args``).  The offsets must follow
    :func:`pack_layout` and ``arena_bytes`` must be its total; a violation, a
    misaligned pointer or a destination that overlaps the arena raises
    ``GpuLibError`` and launches nothing.  Overlap between destinations is
    the caller's responsibility.  Exactly ``nbytes`` bytes are written at
    each ``dst_ptr`` (0 is allowed for a zero-byte segment) and the arena is
    only read.  Returns ``{"sum": (s0, s1), "kernel_ms": ...}``: the sum is
    :func:`checksum_device` of the arena, padding included, and the time is
    the kernel alone.  Runs on the library's copy stream; work on the buffers
    on another stream must be complete (``torch.cuda.synchronize()``) first."""
    lib = load()
    n = len(segments)
    dst = (ctypes.c_void_p * n)(*[int(s[0]) or None for s in segments])
    off = (ctypes.c_uint64 * n)(*[int(s[1]) for s in segments])
    size = (ctypes.c_uint64 * n)(*[int(s[2]) for s in segments])
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_unpack_checksum_dev(
            ctypes.c_void_p(arena_ptr), arena_bytes, dst, off, size, n, out,
            ctypes.byref(kernel_ms),
        ),
        "csp_unpack_checksum_dev",
    )
    return {"sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


PATCH_UNCHANGED = (1 << 64) - 1  # a segment's delta_off when it is not patched


def patch_unpack_checksum_device(
    master_ptr: int, arena_bytes: int, delta_ptr: int, delta_bytes: int, segments
) -> dict:
    """:func:`unpack_checksum_device` on a held arena of which some segments
    changed (``patch_tensor_args``).  ``segments`` is a sequence of
    ``(dst_ptr, src_off, nbytes, delta_off_or_None)``: a segment with a
    ``delta_off`` takes its new bytes from the device arena at ``delta_ptr``,
    where the patched segments, in order, follow :func:`pack_layout` and
    total ``delta_bytes``.  In one kernel launch the patched segments'
    16-byte vectors are written over the master in place (their padding as
    the delta has it), every segment of the patched master is scattered to
    its ``dst_ptr``, and the master as it is afterwards is checksummed.  The
    delta is only read, and no master byte outside a patched segment is
    written.  A layout violation, a misaligned pointer, or an overlap of the
    delta with the master or a destination raises ``GpuLibError`` and
    launches nothing.  Returns ``{"sum": (s0, s1), "kernel_ms": ...}``.
    Shares the grid cap of :func:`unpack_checksum_grid_cap`.  Runs on the
    library's copy stream; work on the buffers on another stream must be
    complete (``torch.cuda.synchronize()``) first."""
    lib = load()
    n = len(segments)
    dst = (ctypes.c_void_p * n)(*[int(s[0]) or None for s in segments])
    off = (ctypes.c_uint64 * n)(*[int(s[1]) for s in segments])
    size = (ctypes.c_uint64 * n)(*[int(s[2]) for s in segments])
    delta_off = (ctypes.c_uint64 * n)(
        *[PATCH_UNCHANGED if s[3] is None else int(s[3]) for s in segments]
    )
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_patch_unpack_checksum_dev(
            ctypes.c_void_p(master_ptr), arena_bytes, ctypes.c_void_p(delta_ptr),
            delta_bytes, dst, off, size, delta_off, n, out, ctypes.byref(kernel_ms),
        ),
        "csp_patch_unpack_checksum_dev",
    )
    return {"sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def rebase_unpack_checksum_device(
    base_ptr: int, base_bytes: int, delta_ptr: int, delta_bytes: int,
    out_arena_ptr: int, arena_bytes: int, segments,
) -> dict:
    """Build a NEW arena from a held one plus a delta, scatter it and checksum
    it in one kernel launch (``rebase_tensor_args``).  ``segments`` is a
    sequence of ``(dst_ptr, out_off, nbytes, base_off_or_None,
    delta_off_or_None)`` with exactly one source each: ``out_off`` follows
    :func:`pack_layout` for the new arena of ``arena_bytes``; a ``base_off``
    is any 16-byte multiple inside the base arena (any order, shared between
    segments); the delta-sourced segments, in order, follow
    :func:`pack_layout` inside the delta and total ``delta_bytes``.  Every
    16-byte vector a segment owns is loaded once, written to the new master
    at ``out_arena_ptr`` (padding as the source has it), scattered to
    ``dst_ptr`` and summed with its word index in the new arena.
    ``out_arena_ptr == 0`` is a transient rebase: the same scatter and sum,
    no new master.  Base and delta are only read.  A layout violation, a
    misaligned pointer, or an overlap of the new master or a destination with
    anything it must not touch raises ``GpuLibError`` and launches nothing.
    Returns ``{"sum": (s0, s1), "kernel_ms": ...}``: the sum is
    :func:`checksum_device` of the new arena.  Shares the grid cap of
    :func:`unpack_checksum_grid_cap`.  Runs on the library's copy stream;
    work on the buffers on another stream must be complete
    (``torch.cuda.synchronize()``) first."""
    lib = load()
    n = len(segments)
    dst = (ctypes.c_void_p * n)(*[int(s[0]) or None for s in segments])
    off = (ctypes.c_uint64 * n)(*[int(s[1]) for s in segments])
    size = (ctypes.c_uint64 * n)(*[int(s[2]) for s in segments])
    base_off = (ctypes.c_uint64 * n)(
        *[PATCH_UNCHANGED if s[3] is None else int(s[3]) for s in segments]
    )
    delta_off = (ctypes.c_uint64 * n)(
        *[PATCH_UNCHANGED if s[4] is None else int(s[4]) for s in segments]
    )
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_rebase_unpack_checksum_dev(
            ctypes.c_void_p(base_ptr or None), base_bytes,
            ctypes.c_void_p(delta_ptr or None), delta_bytes,
            ctypes.c_void_p(out_arena_ptr or None), arena_bytes,
            dst, off, size, base_off, delta_off, n, out, ctypes.byref(kernel_ms),
        ),
        "csp_rebase_unpack_checksum_dev",
    )
    return {"sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def unpack_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`unpack_checksum_device`,
    :func:`patch_unpack_checksum_device` and
    :func:`rebase_unpack_checksum_device` (0 restores the shipped default).
    Returns the cap in effect."""
    return int(load().csp_unpack_checksum_grid_cap(int(cap)))


def staged_d2h_bytes(data_ptr: int, nbytes: int) -> bytes:
    """Copy ``nbytes`` from device pointer ``data_ptr`` to host through
    the pooled pinned staging buffer and return them as bytes."""
    lib = load()
    dst = lib.csp_staging_alloc(nbytes)
    if not dst:
        _check(lib, -1, "csp_staging_alloc")
    try:
        _check(
            lib,
            lib.csp_memcpy_d2h(ctypes.c_void_p(dst), ctypes.c_void_p(data_ptr), nbytes),
            "csp_memcpy_d2h",
        )
        return ctypes.string_at(dst, nbytes)
    finally:
        lib.csp_staging_release_all()
