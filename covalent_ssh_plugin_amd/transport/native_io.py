"""ctypes bindings to the host-only native I/O library (libcsp_io.so).

The library (covalent_ssh_plugin_amd/ops/csrc/csp_io.cpp) reads or
writes an exact byte count on a raw fd straight from or into the
caller's buffer.  The channel uses it to receive a large tensor frame
with one kernel-to-destination copy on an executor thread (ctypes drops
the GIL for the call) instead of several passes on the event loop.

It has no HIP or ROCm in it.  A dispatcher host may have no compiler, so
unlike the GPU library a missing build is no error here: :func:`load`
returns ``None`` and the channel keeps its pure-Python receive path.
"""

from __future__ import annotations

import ctypes
import os
import weakref
from pathlib import Path
from typing import Optional

_LIB_NAME = "libcsp_io.so"

OK = 0
EOF = 1
TIMEOUT = 2
# every other code is -errno

_lib: Optional[ctypes.CDLL] = None
_tried = False
# test hook: pretend the library is not built
force_absent = False


def local_io_lib_path() -> str:
    """Path of the built in-tree library, or '' if not built."""
    candidate = Path(__file__).resolve().parent.parent / "ops" / _LIB_NAME
    return str(candidate) if candidate.exists() else ""


def load(path: str = "") -> Optional[ctypes.CDLL]:
    """Load (once) and return the library with typed signatures, or
    ``None`` when it is not built or cannot be loaded."""
    global _lib, _tried
    if force_absent:
        return None
    if _lib is not None or (_tried and not path):
        return _lib
    _tried = True
    lib_path = path or local_io_lib_path()
    if not lib_path:
        return None
    try:
        lib = ctypes.CDLL(lib_path, use_errno=True)
    except OSError:
        return None
    lib.csp_io_read_full.restype = ctypes.c_int
    lib.csp_io_read_full.argtypes = [
        ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
    ]
    lib.csp_io_write_full.restype = ctypes.c_int
    lib.csp_io_write_full.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    lib.csp_io_alloc.restype = ctypes.c_void_p
    lib.csp_io_alloc.argtypes = [ctypes.c_size_t]
    lib.csp_io_free.restype = ctypes.c_int
    lib.csp_io_free.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.csp_io_checksum.restype = None
    lib.csp_io_checksum.argtypes = [
        ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64),
    ]
    _lib = lib
    return lib


def _address(buf, offset: int, nbytes: int) -> tuple:
    """(address, keep-alive) of ``nbytes`` at ``offset`` in a writable
    buffer-protocol object."""
    view = memoryview(buf).cast("B")
    if offset < 0 or nbytes < 0 or offset + nbytes > view.nbytes:
        raise ValueError("range outside the buffer")
    if nbytes == 0:
        return 0, view
    window = view[offset : offset + nbytes]
    carrier = (ctypes.c_char * nbytes).from_buffer(window)  # TypeError if read-only
    return ctypes.addressof(carrier), (carrier, window)


def read_full(fd: int, buf, nbytes: int, timeout_ms: int, offset: int = 0) -> int:
    """Read exactly ``nbytes`` from ``fd`` into ``buf[offset:]``.  Returns
    OK, EOF, TIMEOUT or -errno.  ``timeout_ms`` bounds each wait for the
    next byte; negative means no limit."""
    lib = load()
    if lib is None:
        raise RuntimeError(f"{_LIB_NAME} is not built")
    addr, keep = _address(buf, offset, nbytes)
    rc = lib.csp_io_read_full(fd, addr, nbytes, timeout_ms)
    del keep
    return rc


def write_full(fd: int, buf, nbytes: Optional[int] = None, offset: int = 0) -> int:
    """Write exactly ``nbytes`` of ``buf[offset:]`` to ``fd``.  Returns OK
    or -errno (-EPIPE for a closed reader)."""
    lib = load()
    if lib is None:
        raise RuntimeError(f"{_LIB_NAME} is not built")
    if nbytes is None:
        nbytes = memoryview(buf).nbytes - offset
    view = memoryview(buf).cast("B")
    if nbytes == 0:
        return lib.csp_io_write_full(fd, None, 0)
    window = view[offset : offset + nbytes]
    if window.readonly:
        # ctypes cannot borrow a read-only buffer; bytes pass by pointer
        return lib.csp_io_write_full(fd, bytes(window), nbytes)
    carrier = (ctypes.c_char * nbytes).from_buffer(window)
    return lib.csp_io_write_full(fd, ctypes.addressof(carrier), nbytes)


def checksum(buf, nbytes: Optional[int] = None, offset: int = 0):
    """The two-word checksum ``(s0, s1)`` of ``nbytes`` of ``buf[offset:]``
    (definition in ops/csrc/csp_io.h; the worker's GPU kernel computes the
    same two numbers over the bytes once they are in HBM).  ``None`` when
    the library is not loaded: the caller then sends no checksum and the
    worker verifies nothing.  There is no pure-Python fallback on purpose,
    it would cost more than the transfer."""
    lib = load()
    if lib is None:
        return None
    view = memoryview(buf).cast("B")
    if nbytes is None:
        nbytes = view.nbytes - offset
    if offset < 0 or nbytes < 0 or offset + nbytes > view.nbytes:
        raise ValueError("range outside the buffer")
    out = (ctypes.c_uint64 * 2)()
    if nbytes == 0:
        lib.csp_io_checksum(None, 0, out)
        return int(out[0]), int(out[1])
    window = view[offset : offset + nbytes]
    if window.readonly:
        # ctypes cannot borrow a read-only buffer; bytes pass by pointer
        lib.csp_io_checksum(bytes(window), nbytes, out)
    else:
        carrier = (ctypes.c_char * nbytes).from_buffer(window)
        lib.csp_io_checksum(ctypes.addressof(carrier), nbytes, out)
    return int(out[0]), int(out[1])


def alloc_buffer(nbytes: int):
    """A writable ``nbytes`` buffer (ctypes ``c_ubyte`` array) on an
    anonymous mapping that asks for transparent huge pages: first touch of
    a fresh 1 GiB destination then costs a few hundred faults instead of
    262,144.  The mapping is unmapped when the array is collected;
    ``torch.frombuffer`` on it keeps it alive.  ``None`` when the library
    is absent or the mapping fails (callers fall back to ``bytearray``)."""
    lib = load()
    if lib is None or nbytes <= 0:
        return None
    addr = lib.csp_io_alloc(nbytes)
    if not addr:
        return None
    arr = (ctypes.c_ubyte * nbytes).from_address(addr)
    weakref.finalize(arr, lib.csp_io_free, addr, nbytes)
    return arr


def strerror(rc: int) -> str:
    if rc == OK:
        return "ok"
    if rc == EOF:
        return "end of file"
    if rc == TIMEOUT:
        return "timed out"
    return os.strerror(-rc)
