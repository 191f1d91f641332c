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
* ``csp_gather_checksum_dev`` — one strided device tensor written in
  row-major order to a contiguous buffer, with that buffer's checksum from the
  same launch (``gather_tensor_results``),
* ``csp_pack_gather_checksum_dev`` — the packed arena filled from contiguous
  and strided tensors together by one launch, with its checksum
  (``pack_tensor_results`` with ``gather_tensor_results``), and
  ``csp_gather_supported``, the host-side question whether a layout is served,
* ``csp_narrow_checksum_dev`` — a contiguous float32, float64, int32 or int64
  device tensor tested for a lossless narrower form, written in that form and
  checksummed by one launch (``narrow_tensor_results``),
* ``csp_pack_narrow_probe_dev`` and ``csp_pack_narrow_checksum_dev`` — the
  same inside the packed arena: one launch tests all candidate tensors, one
  fills and sums an arena of narrowed segments and plain copies
  (``pack_tensor_results`` with ``narrow_tensor_results``),
* ``csp_widen_checksum_dev`` — the inverse for arguments: narrow bytes in HBM
  widened into one or two destinations and checksummed by one launch
  (``narrow_tensor_args``),
* ``csp_bool_pack_checksum_dev`` / ``csp_bool_unpack_checksum_dev`` — a bool
  tensor packed to one bit per element, tested and checksummed by one launch,
  and the inverse into one or two destinations (both options),
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


class PackGatherSeg(ctypes.Structure):
    """``CspPackGatherSeg``: one segment of ``csp_pack_gather_checksum_dev``.
    ``ndim == 0`` is ``nbytes`` contiguous bytes; otherwise a strided tensor
    with ``shape`` and ``stride`` in elements, as torch reports them."""

    _fields_ = [
        ("src", ctypes.c_void_p),
        ("dst_off", ctypes.c_uint64),
        ("nbytes", ctypes.c_uint64),
        ("elem_size", ctypes.c_uint32),
        ("ndim", ctypes.c_uint32),
        ("shape", ctypes.c_uint64 * 8),
        ("stride", ctypes.c_uint64 * 8),
    ]


class PackNarrowSeg(ctypes.Structure):
    """``CspPackNarrowSeg``: one segment of ``csp_pack_narrow_probe_dev`` and
    ``csp_pack_narrow_checksum_dev``.  ``dst_kind == -1`` is a copy of
    ``numel`` bytes; otherwise ``numel`` elements of ``src_kind``."""

    _fields_ = [
        ("src", ctypes.c_void_p),
        ("numel", ctypes.c_uint64),
        ("src_kind", ctypes.c_int32),
        ("dst_kind", ctypes.c_int32),
        ("dst_off", ctypes.c_uint64),
    ]


class UnpackWidenSeg(ctypes.Structure):
    """``CspUnpackWidenSeg``: one segment of ``csp_unpack_widen_checksum_dev``.
    ``narrow_kind == -1`` is a copy of ``count`` bytes; otherwise ``count``
    elements widened from ``narrow_kind`` to ``wide_kind``."""

    _fields_ = [
        ("dst", ctypes.c_void_p),
        ("src_off", ctypes.c_uint64),
        ("dst_off", ctypes.c_uint64),
        ("count", ctypes.c_uint64),
        ("narrow_kind", ctypes.c_int32),
        ("wide_kind", ctypes.c_int32),
    ]


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
    lib.csp_diff_checksum_dev.restype = ctypes.c_int
    lib.csp_diff_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_float),
    ]
    lib.csp_diff_block_bytes.restype = ctypes.c_size_t
    lib.csp_diff_block_bytes.argtypes = []
    lib.csp_diff_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_diff_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_narrow_checksum_dev.restype = ctypes.c_int
    lib.csp_narrow_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_int,
        ctypes.c_int,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_float),
    ]
    lib.csp_narrow_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_narrow_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_pack_narrow_probe_dev.restype = ctypes.c_int
    lib.csp_pack_narrow_probe_dev.argtypes = [
        ctypes.POINTER(PackNarrowSeg),
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_pack_narrow_checksum_dev.restype = ctypes.c_int
    lib.csp_pack_narrow_checksum_dev.argtypes = [
        ctypes.POINTER(PackNarrowSeg),
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_pack_narrow_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_pack_narrow_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_pack_narrow_probe_nt.restype = ctypes.c_int
    lib.csp_pack_narrow_probe_nt.argtypes = [ctypes.c_int]
    lib.csp_narrow_fits.restype = ctypes.c_uint32
    lib.csp_narrow_fits.argtypes = [ctypes.c_int, ctypes.c_uint64]
    lib.csp_widen_checksum_dev.restype = ctypes.c_int
    lib.csp_widen_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_int,
        ctypes.c_int,
        ctypes.c_void_p,
        ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_float),
    ]
    lib.csp_widen_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_widen_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_bool_pack_checksum_dev.restype = ctypes.c_int
    lib.csp_bool_pack_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_float),
    ]
    lib.csp_bool_unpack_checksum_dev.restype = ctypes.c_int
    lib.csp_bool_unpack_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_float),
    ]
    for name in ("csp_bool_pack_checksum_grid_cap", "csp_bool_unpack_checksum_grid_cap"):
        getattr(lib, name).restype = ctypes.c_size_t
        getattr(lib, name).argtypes = [ctypes.c_size_t]
    lib.csp_unpack_widen_checksum_dev.restype = ctypes.c_int
    lib.csp_unpack_widen_checksum_dev.argtypes = [
        ctypes.POINTER(UnpackWidenSeg),
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
    ]
    lib.csp_unpack_widen_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_unpack_widen_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_gather_checksum_dev.restype = ctypes.c_int
    lib.csp_gather_checksum_dev.argtypes = [
        ctypes.c_void_p,
        ctypes.c_uint,
        ctypes.c_uint,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_int),
    ]
    lib.csp_gather_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_gather_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_gather_checksum_path.restype = ctypes.c_int
    lib.csp_gather_checksum_path.argtypes = [ctypes.c_int]
    lib.csp_pack_gather_checksum_dev.restype = ctypes.c_int
    lib.csp_pack_gather_checksum_dev.argtypes = [
        ctypes.POINTER(PackGatherSeg),
        ctypes.c_size_t,
        ctypes.c_void_p,
        ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_int),
    ]
    lib.csp_gather_supported.restype = ctypes.c_int
    lib.csp_gather_supported.argtypes = [
        ctypes.c_uint,
        ctypes.c_uint,
        ctypes.POINTER(ctypes.c_uint64),
        ctypes.POINTER(ctypes.c_uint64),
    ]
    lib.csp_pack_gather_checksum_grid_cap.restype = ctypes.c_size_t
    lib.csp_pack_gather_checksum_grid_cap.argtypes = [ctypes.c_size_t]
    lib.csp_pack_gather_checksum_path.restype = ctypes.c_int
    lib.csp_pack_gather_checksum_path.argtypes = [ctypes.c_int]
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


def diff_block_bytes() -> int:
    """Bytes of one block of :func:`diff_checksum_device`."""
    return int(load().csp_diff_block_bytes())


def diff_checksum_device(
    cur_ptr: int, base_ptr: int, nbytes: int, delta_ptr: int, cap_blocks: int
) -> dict:
    """Compare ``nbytes`` at device pointer ``cur_ptr`` with ``nbytes`` at
    ``base_ptr`` bitwise in blocks of :func:`diff_block_bytes`, compact the
    blocks that differ into the device buffer at ``delta_ptr`` (room for
    ``cap_blocks * (block + 4)`` bytes) and checksum ``cur`` in the same
    kernel launch (``delta_tensor_results``).  Returns ``{"rc", "changed",
    "sum", "kernel_ms"}``.  ``rc`` 0: ``delta[0 : changed * (block + 4))`` is
    the frame, the changed blocks in slot order (the last block of the
    buffer zero padded) and then their block numbers as little-endian u32.
    ``rc`` 1: more than ``cap_blocks`` blocks differ; ``changed`` and ``sum``
    are valid, ``delta`` is not.  ``sum`` equals ``checksum_device(cur_ptr,
    nbytes)``.  A null or misaligned pointer, a ``delta`` range that overlaps
    ``cur`` or ``base`` or a block count beyond u32 raises ``GpuLibError`` and
    launches nothing.  Runs on the library's copy stream; the two buffers
    written on another stream must be complete first."""
    lib = load()
    changed = ctypes.c_uint64()
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_float()
    rc = lib.csp_diff_checksum_dev(
        ctypes.c_void_p(cur_ptr or None), ctypes.c_void_p(base_ptr or None), nbytes,
        ctypes.c_void_p(delta_ptr or None), cap_blocks, ctypes.byref(changed), out,
        ctypes.byref(kernel_ms),
    )
    if rc not in (0, 1):
        _check(lib, rc, "csp_diff_checksum_dev")
    return {
        "rc": rc,
        "changed": int(changed.value),
        "sum": (int(out[0]), int(out[1])),
        "kernel_ms": kernel_ms.value,
    }


def diff_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`diff_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_diff_checksum_grid_cap(int(cap)))


# element kinds of :func:`narrow_checksum_device`, by torch dtype name, their
# sizes, and every source's targets from the narrowest to the widest
NARROW_KINDS = {
    "float32": 0, "float64": 1, "int32": 2, "int64": 3, "bfloat16": 4, "int16": 5, "uint8": 6,
}
NARROW_ELEM_SIZE = {
    "float32": 4, "float64": 8, "int32": 4, "int64": 8, "bfloat16": 2, "int16": 2, "uint8": 1,
}
NARROW_TARGETS = {
    "float32": ("bfloat16",),
    "float64": ("float32",),
    "int64": ("uint8", "int16", "int32"),
    "int32": ("uint8", "int16"),
}


def narrow_bytes(numel: int, dst: str) -> int:
    """Bytes of ``numel`` elements narrowed to ``dst``, zero padded to 16."""
    return (numel * NARROW_ELEM_SIZE[dst] + 15) // 16 * 16


def narrow_checksum_device(
    src_ptr: int, numel: int, src: str, dst: str = "", dst_ptr: int = 0, dst_bytes: int = 0
) -> dict:
    """Test the ``numel`` contiguous ``src`` elements (a dtype name of
    ``NARROW_TARGETS``) at device pointer ``src_ptr`` for lossless narrowing
    (``narrow_tensor_results``).  Returns ``{"rc", "fits", "sum",
    "kernel_ms"}``; ``fits`` is the tuple of ``src``'s targets, narrowest
    first, that give every element back bit for bit when widened.  With
    ``dst_ptr`` 0 the call is a probe and stores nothing.  With ``dst_ptr``
    set, the elements narrowed to ``dst`` are written there in the same kernel
    launch, zero padded to ``dst_bytes == narrow_bytes(numel, dst)``, and
    ``sum`` equals ``checksum_device(dst_ptr, dst_bytes)`` if ``dst`` is in
    ``fits``; if it is not, the buffer and ``sum`` mean nothing.  An unserved
    pair, a null or misaligned pointer, a wrong ``dst_bytes``, a source above
    16 GiB or overlapping buffers raise ``GpuLibError`` and launch nothing.
    Runs on the library's copy stream; a source written on another stream
    must be complete first."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    fits = ctypes.c_uint32()
    kernel_ms = ctypes.c_float()
    rc = lib.csp_narrow_checksum_dev(
        ctypes.c_void_p(src_ptr or None), numel, NARROW_KINDS.get(src, -1),
        NARROW_KINDS.get(dst, -1), ctypes.c_void_p(dst_ptr or None), dst_bytes, out,
        ctypes.byref(fits), ctypes.byref(kernel_ms),
    )
    _check(lib, rc, "csp_narrow_checksum_dev")
    return {
        "rc": rc,
        "fits": tuple(
            d for d in NARROW_TARGETS.get(src, ()) if fits.value >> NARROW_KINDS[d] & 1
        ),
        "sum": (int(out[0]), int(out[1])),
        "kernel_ms": kernel_ms.value,
    }


def narrow_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`narrow_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_narrow_checksum_grid_cap(int(cap)))


def _pack_narrow_table(segments):
    """``(src_ptr, numel, src, dst, dst_off)`` rows as ``PackNarrowSeg``;
    ``dst`` ``""`` is a copy of ``numel`` bytes."""
    table = (PackNarrowSeg * max(1, len(segments)))()
    for row, (ptr, numel, src, dst, off) in zip(table, segments):
        row.src = int(ptr) or None
        row.numel = int(numel)
        row.src_kind = NARROW_KINDS.get(src, -2) if src else 0
        row.dst_kind = NARROW_KINDS.get(dst, -2) if dst else -1
        row.dst_off = int(off)
    return table


def _fits_of(lib, src: str, bad: int) -> tuple:
    mask = lib.csp_narrow_fits(NARROW_KINDS.get(src, -1), bad)
    return tuple(d for d in NARROW_TARGETS.get(src, ()) if mask >> NARROW_KINDS[d] & 1)


def pack_narrow_probe_device(segments) -> dict:
    """Test every ``(src_ptr, numel, src)`` of ``segments``, contiguous
    16-byte aligned device tensors of a dtype name in ``NARROW_TARGETS``, for
    lossless narrowing in ONE kernel launch that stores one word per segment
    (``pack_tensor_results`` with ``narrow_tensor_results``).  Returns
    ``{"bad", "fits", "kernel_ms"}``: per segment the raw word, and the tuple of
    its targets, narrowest first, that give every element back bit for bit.
    A null or misaligned pointer, a dtype without targets or a segment above
    16 GiB raises ``GpuLibError`` naming the segment and launches nothing.
    Runs on the library's copy stream; sources written on another stream must
    be complete first."""
    lib = load()
    n = len(segments)
    table = _pack_narrow_table([(s[0], s[1], s[2], "", 0) for s in segments])
    bad = (ctypes.c_uint64 * max(1, n))()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_pack_narrow_probe_dev(table, n, bad, ctypes.byref(kernel_ms)),
        "csp_pack_narrow_probe_dev",
    )
    words = [int(bad[k]) for k in range(n)]
    return {
        "bad": words,
        "fits": [_fits_of(lib, s[2], w) for s, w in zip(segments, words)],
        "kernel_ms": kernel_ms.value,
    }


def pack_narrow_layout(segments):
    """``(offsets, total)`` of an arena of ``(src_ptr, numel, src, dst)``
    segments: :func:`pack_layout` over the bytes each occupies in the arena,
    ``numel`` bytes for a copy (``dst == ""``), ``numel`` elements of ``dst``
    otherwise."""
    return pack_layout(
        [s[1] * NARROW_ELEM_SIZE[s[3]] if s[3] else s[1] for s in segments]
    )


def pack_narrow_checksum_device(segments, arena_ptr: int, arena_bytes: int) -> dict:
    """Fill the 16-byte aligned device arena at ``arena_ptr`` from
    ``segments``, ``(src_ptr, numel, src, dst, dst_off)`` each, and checksum it
    in ONE kernel launch.  ``dst == ""`` copies ``numel`` bytes from any
    alignment; otherwise the ``numel`` contiguous ``src`` elements at the
    16-byte aligned ``src_ptr`` are narrowed to ``dst`` (a pair of
    :func:`narrow_checksum_device`).  Offsets and ``arena_bytes`` follow
    :func:`pack_narrow_layout`; the padding is stored as zero.  Returns
    ``{"sum", "bad", "fits", "kernel_ms"}``: ``sum`` is :func:`checksum_device`
    of the arena; ``fits[k]`` is what the pass that wrote segment ``k`` found
    exact (``None`` for a copy) — when ``dst`` is not in it the segment's
    bytes mean nothing.  A layout violation, an unserved pair, a null or
    misaligned pointer or a source that overlaps the arena raises
    ``GpuLibError`` naming the segment and launches nothing.  Runs on the
    library's copy stream; sources written on another stream must be complete
    first."""
    lib = load()
    n = len(segments)
    table = _pack_narrow_table(segments)
    out = (ctypes.c_uint64 * 2)()
    bad = (ctypes.c_uint64 * max(1, n))()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_pack_narrow_checksum_dev(
            table, n, ctypes.c_void_p(arena_ptr or None), arena_bytes, out, bad,
            ctypes.byref(kernel_ms),
        ),
        "csp_pack_narrow_checksum_dev",
    )
    words = [int(bad[k]) for k in range(n)]
    return {
        "sum": (int(out[0]), int(out[1])),
        "bad": words,
        "fits": [_fits_of(lib, s[2], w) if s[3] else None for s, w in zip(segments, words)],
        "kernel_ms": kernel_ms.value,
    }


def pack_narrow_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`pack_narrow_probe_device` and
    :func:`pack_narrow_checksum_device` (0 restores the shipped default).
    Returns the cap in effect."""
    return int(load().csp_pack_narrow_checksum_grid_cap(int(cap)))


def pack_narrow_probe_nt(on: int = -1) -> int:
    """Tools only: 1 makes :func:`pack_narrow_probe_device` load
    nontemporally, 0 plainly, -1 restores the shipped default.  Returns the
    value in effect."""
    return int(load().csp_pack_narrow_probe_nt(int(on)))


def widen_checksum_device(
    src_ptr: int, numel: int, narrow: str, wide: str, dst_ptr: int, dst2_ptr: int = 0
) -> dict:
    """Widen the ``numel`` contiguous ``narrow`` elements at device pointer
    ``src_ptr`` to ``wide`` (a pair of ``NARROW_TARGETS`` read backwards;
    ``narrow_tensor_args``) into ``dst_ptr`` and, when set, ``dst2_ptr`` as
    well, in one kernel launch.  Returns ``{"rc", "sum", "kernel_ms"}``;
    ``sum`` equals ``checksum_device(dst_ptr, numel * NARROW_ELEM_SIZE[wide])``.
    The source must be readable up to ``narrow_bytes(numel, narrow)``, its pad
    bytes may hold anything; the destinations are exactly the wide bytes.  An
    unserved pair, a null or misaligned pointer, wide bytes above 16 GiB or
    overlapping buffers raise ``GpuLibError`` and launch nothing.  Runs on the
    library's copy stream; a source written on another stream must be complete
    first."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_float()
    rc = lib.csp_widen_checksum_dev(
        ctypes.c_void_p(src_ptr or None), numel, NARROW_KINDS.get(narrow, -1),
        NARROW_KINDS.get(wide, -1), ctypes.c_void_p(dst_ptr or None),
        ctypes.c_void_p(dst2_ptr or None), out, ctypes.byref(kernel_ms),
    )
    _check(lib, rc, "csp_widen_checksum_dev")
    return {"rc": rc, "sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def widen_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`widen_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_widen_checksum_grid_cap(int(cap)))


def unpack_widen_layout(segments):
    """``(narrow offsets, narrow total, wide offsets, wide total)`` of an
    argument arena of ``(count, narrow, wide)`` segments: :func:`pack_layout`
    over the bytes each has on the wire and over its full-width bytes.
    ``narrow == ""`` is a copy of ``count`` bytes; otherwise ``count`` elements
    travel as ``narrow`` and are ``wide`` on the device."""
    src_off, narrow_total = pack_layout(
        [n * NARROW_ELEM_SIZE[narrow] if narrow else n for n, narrow, _wide in segments]
    )
    dst_off, wide_total = pack_layout(
        [n * NARROW_ELEM_SIZE[wide] if narrow else n for n, narrow, wide in segments]
    )
    return src_off, narrow_total, dst_off, wide_total


def unpack_widen_checksum_device(
    segments, narrow_ptr: int, narrow_bytes: int, master_ptr: int, wide_bytes: int
) -> dict:
    """Unpack the narrow device arena at ``narrow_ptr`` into ``segments``,
    ``(dst_ptr, src_off, dst_off, count, narrow, wide)`` each, at full width
    and checksum the WIDE arena in ONE kernel launch (``pack_tensor_args``
    with ``narrow_tensor_args``).  ``narrow == ""`` copies ``count`` bytes;
    otherwise ``count`` ``narrow`` elements are widened to ``wide`` (a pair of
    :func:`widen_checksum_device`).  Offsets and totals follow
    :func:`unpack_widen_layout`.  With ``master_ptr`` set every segment is also
    written there at ``dst_off``, the padding after a widened segment zero:
    afterwards it is the wide arena.  Returns ``{"sum", "kernel_ms"}``;
    ``sum`` is :func:`checksum_device` of the wide arena.  A layout violation,
    an unserved pair, a null or misaligned pointer, ``wide_bytes`` above 4 GiB
    or an overlap among the narrow arena, the master and a destination raises
    ``GpuLibError`` naming the segment and launches nothing.  Runs on the
    library's copy stream; work on the buffers on another stream must be
    complete first."""
    lib = load()
    n = len(segments)
    table = (UnpackWidenSeg * max(1, n))()
    for row, (dst, src_off, dst_off, count, narrow, wide) in zip(table, segments):
        row.dst = int(dst) or None
        row.src_off = int(src_off)
        row.dst_off = int(dst_off)
        row.count = int(count)
        row.narrow_kind = NARROW_KINDS.get(narrow, -2) if narrow else -1
        row.wide_kind = NARROW_KINDS.get(wide, -2) if narrow else 0
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    _check(
        lib,
        lib.csp_unpack_widen_checksum_dev(
            table, n, ctypes.c_void_p(narrow_ptr or None), narrow_bytes,
            ctypes.c_void_p(master_ptr or None), wide_bytes, out, ctypes.byref(kernel_ms),
        ),
        "csp_unpack_widen_checksum_dev",
    )
    return {"sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def unpack_widen_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`unpack_widen_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_unpack_widen_checksum_grid_cap(int(cap)))


def bool_bits_bytes(numel: int) -> int:
    """Bytes of ``numel`` bool elements as ``"bits"`` in a device buffer: one
    bit each, zero padded to 16 bytes."""
    return ((numel + 7) // 8 + 15) // 16 * 16


def bool_pack_checksum_device(src_ptr: int, numel: int, dst_ptr: int = 0, dst_bytes: int = 0) -> dict:
    """Test the ``numel`` bool bytes at device pointer ``src_ptr`` for the
    ``"bits"`` form (``narrow_tensor_results``).  Returns ``{"rc", "bad", "sum",
    "kernel_ms"}``; ``bad`` is the OR of ``byte & 0xFE`` over all bytes, 0 iff
    every byte is 0 or 1.  With ``dst_ptr`` 0 the call is a probe and stores
    nothing.  With ``dst_ptr`` set, element ``i`` is written as bit ``i % 8`` of
    byte ``i // 8`` (``numpy.packbits(bitorder="little")``) in the same kernel
    launch, zero padded to ``dst_bytes == bool_bits_bytes(numel)``, and ``sum``
    equals ``checksum_device(dst_ptr, dst_bytes)`` when ``bad`` is 0.  A null or
    misaligned pointer, a wrong ``dst_bytes``, more than 16 GiB or overlapping
    buffers raise ``GpuLibError`` and launch nothing.  Runs on the library's
    copy stream; a source written on another stream must be complete first."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    bad = ctypes.c_uint32()
    kernel_ms = ctypes.c_float()
    rc = lib.csp_bool_pack_checksum_dev(
        ctypes.c_void_p(src_ptr or None), numel, ctypes.c_void_p(dst_ptr or None), dst_bytes,
        out, ctypes.byref(bad), ctypes.byref(kernel_ms),
    )
    _check(lib, rc, "csp_bool_pack_checksum_dev")
    return {"rc": rc, "bad": bad.value, "sum": (int(out[0]), int(out[1])),
            "kernel_ms": kernel_ms.value}


def bool_unpack_checksum_device(src_ptr: int, numel: int, dst_ptr: int, dst2_ptr: int = 0) -> dict:
    """Unpack the ``numel`` elements held as ``"bits"`` at device pointer
    ``src_ptr`` into bool bytes at ``dst_ptr`` and, when set, ``dst2_ptr`` as
    well, in one kernel launch (``narrow_tensor_args``).  Returns ``{"rc",
    "sum", "kernel_ms"}``; ``sum`` equals ``checksum_device(dst_ptr, numel)``.
    The source must be readable up to ``bool_bits_bytes(numel)``, its pad bits
    and pad bytes may hold anything; the destinations are exactly ``numel``
    bytes.  A null or misaligned pointer, more than 16 GiB or overlapping
    buffers raise ``GpuLibError`` and launch nothing."""
    lib = load()
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_float()
    rc = lib.csp_bool_unpack_checksum_dev(
        ctypes.c_void_p(src_ptr or None), numel, ctypes.c_void_p(dst_ptr or None),
        ctypes.c_void_p(dst2_ptr or None), out, ctypes.byref(kernel_ms),
    )
    _check(lib, rc, "csp_bool_unpack_checksum_dev")
    return {"rc": rc, "sum": (int(out[0]), int(out[1])), "kernel_ms": kernel_ms.value}


def bool_pack_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`bool_pack_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_bool_pack_checksum_grid_cap(int(cap)))


def bool_unpack_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`bool_unpack_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_bool_unpack_checksum_grid_cap(int(cap)))


GATHER_PATHS = {0: "none", 1: "direct", 2: "direct16", 3: "transpose", 5: "slab"}


def gather_checksum_device(
    src_ptr: int, elem_size: int, sizes, strides, dst_ptr: int, dst_bytes: int
) -> dict:
    """Write the strided device tensor at ``src_ptr`` (``sizes`` and
    ``strides`` in elements of ``elem_size`` bytes, as torch gives them) in
    row-major order to the 16-byte aligned device buffer at ``dst_ptr`` and
    checksum that buffer in the same kernel launch
    (``gather_tensor_results``).  ``dst_bytes`` is the data rounded up to 16;
    the padding is stored as zero.  Returns ``{"sums": (s0, s1), "kernel_ms",
    "path"}``: ``sums`` equals ``checksum_device(dst_ptr, dst_bytes)``,
    ``path`` is ``"direct"`` (per-element loads), ``"direct16"`` (16-byte
    loads), ``"transpose"`` (through an LDS tile), ``"slab"`` (a short inner
    dimension under the unit-stride one, such as a ``channels_last`` 3 x 3
    weight, through an LDS slab in output order; only under
    ``gather_checksum_path(2)``) or ``"none"`` (no element).
    An element size outside 1, 2, 4, 8, 16, more than 4 dimensions after
    collapsing, a null or misaligned pointer, a wrong ``dst_bytes`` or a source
    extent that overlaps the destination raises ``GpuLibError`` and launches
    nothing.  Runs on the library's copy stream; a source written on another
    stream must be complete (``torch.cuda.synchronize()``) first."""
    lib = load()
    n = len(sizes)
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    path = ctypes.c_int()
    _check(
        lib,
        lib.csp_gather_checksum_dev(
            ctypes.c_void_p(src_ptr or None), elem_size, n,
            (ctypes.c_uint64 * n)(*[int(v) for v in sizes]),
            (ctypes.c_uint64 * n)(*[int(v) for v in strides]),
            ctypes.c_void_p(dst_ptr or None), dst_bytes, out,
            ctypes.byref(kernel_ms), ctypes.byref(path),
        ),
        "csp_gather_checksum_dev",
    )
    return {
        "sums": (int(out[0]), int(out[1])),
        "kernel_ms": kernel_ms.value,
        "path": GATHER_PATHS[path.value],
    }


def gather_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`gather_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_gather_checksum_grid_cap(int(cap)))


def gather_checksum_path(force: int = 0) -> int:
    """Tools only: 1 forces the direct path of :func:`gather_checksum_device`,
    2 takes the slab path wherever its rule holds (the host does not choose it
    by itself: it measured slower than the direct path), 0 restores the host's
    choice.  Returns the value in effect."""
    return int(load().csp_gather_checksum_path(int(force)))


PACK_GATHER_PATHS = dict(GATHER_PATHS)
PACK_GATHER_PATHS[4] = "copy"


def pack_gather_segments(segments):
    """A ``PackGatherSeg`` array from ``(src_ptr, dst_off, nbytes)`` tuples
    (contiguous bytes) and ``(src_ptr, dst_off, nbytes, elem_size, shape,
    stride)`` tuples (strided tensors)."""
    array = (PackGatherSeg * len(segments))()
    for seg, entry in zip(array, segments):
        seg.src = int(entry[0]) or None
        seg.dst_off, seg.nbytes = int(entry[1]), int(entry[2])
        if len(entry) > 3:
            seg.elem_size, shape, stride = int(entry[3]), entry[4], entry[5]
            seg.ndim = len(shape)
            if len(shape) > 8 or len(stride) != len(shape):
                raise GpuLibError("a packed strided segment has at most 8 dimensions")
            seg.shape[: len(shape)] = [int(v) for v in shape]
            seg.stride[: len(stride)] = [int(v) for v in stride]
    return array


def pack_gather_checksum_device(segments, arena_ptr: int, arena_bytes: int) -> dict:
    """:func:`pack_checksum_device` for a mix of contiguous and strided
    sources in ONE kernel launch (``pack_tensor_results`` with
    ``gather_tensor_results``).  ``segments`` is a sequence of ``(src_ptr,
    dst_off, nbytes)`` for contiguous bytes and ``(src_ptr, dst_off, nbytes,
    elem_size, shape, stride)`` for a strided tensor, which lands in row-major
    order; offsets follow :func:`pack_layout`.  Returns ``{"sums": (s0, s1),
    "kernel_ms", "paths"}``: ``sums`` equals ``checksum_device(arena_ptr,
    arena_bytes)``, ``paths`` has one of ``"copy"``, ``"direct"``,
    ``"direct16"``, ``"transpose"``, ``"slab"`` or ``"none"`` (no byte) per
    segment.
    Refuses what :func:`pack_checksum_device` refuses, a strided segment that
    :func:`gather_supported` does not serve, an ``nbytes`` that disagrees with
    the shape, and a source extent that overlaps the arena (``GpuLibError``
    naming the segment, nothing launched).  Runs on the library's copy stream;
    sources written on another stream must be complete first."""
    lib = load()
    n = len(segments)
    out = (ctypes.c_uint64 * 2)()
    kernel_ms = ctypes.c_double()
    paths = (ctypes.c_int * max(n, 1))()
    _check(
        lib,
        lib.csp_pack_gather_checksum_dev(
            pack_gather_segments(segments), n, ctypes.c_void_p(arena_ptr or None), arena_bytes,
            out, ctypes.byref(kernel_ms), paths,
        ),
        "csp_pack_gather_checksum_dev",
    )
    return {
        "sums": (int(out[0]), int(out[1])),
        "kernel_ms": kernel_ms.value,
        "paths": [PACK_GATHER_PATHS[paths[k]] for k in range(n)],
    }


def gather_supported(elem_size: int, sizes, strides) -> bool:
    """Whether :func:`pack_gather_checksum_device` serves a strided segment of
    this layout: element size 1, 2, 4, 8 or 16, at most 4 dimensions after
    collapsing, fewer than 2^32 elements.  Host only, nothing is launched."""
    n = len(sizes)
    if n > 8 or len(strides) != n:
        return False
    return bool(load().csp_gather_supported(
        elem_size, n,
        (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in sizes]),
        (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in strides]),
    ))


def pack_gather_checksum_grid_cap(cap: int = 0) -> int:
    """Tools only: set the grid cap of :func:`pack_gather_checksum_device` (0
    restores the shipped default).  Returns the cap in effect."""
    return int(load().csp_pack_gather_checksum_grid_cap(int(cap)))


def pack_gather_checksum_path(force: int = 0) -> int:
    """Tools only: 1 makes :func:`pack_gather_checksum_device` take the direct
    path where the host would choose the transpose, 2 makes it take the slab
    path wherever its rule holds (the host does not choose it by itself), 0
    restores the host's choice.  Returns the value in effect."""
    return int(load().csp_pack_gather_checksum_path(int(force)))


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
