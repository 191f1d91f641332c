"""Host-only native I/O library (ops/csrc/csp_io.cpp) through its ctypes
binding: exact-length reads and writes on pipes, blocking and
O_NONBLOCK, delivered in awkward pieces."""

import errno
import os
import threading
import time

import pytest

from covalent_ssh_plugin_amd.ops import build as ops_build
from covalent_ssh_plugin_amd.transport import native_io

PAYLOAD_SIZES = [0, 1, 65535, 65537, (1 << 20) + 3]
PIECES = [1, 4095, 65537]


@pytest.fixture(scope="module", autouse=True)
def _built_library():
    ops_build.build_io(verbose=False)
    assert native_io.load() is not None, "libcsp_io.so did not load"


def _pattern(n: int) -> bytes:
    # period 251 (prime): a shifted, dropped or repeated piece shows up
    return bytes((i * 7 + 3) % 251 for i in range(min(n, 251))) * (n // 251 + 1)


def _payload(n: int) -> bytes:
    return _pattern(n)[:n]


def _write_in_pieces(fd: int, data: bytes, piece: int, close: bool = True) -> None:
    try:
        view = memoryview(data)
        while view:
            os.write(fd, view[:piece])
            view = view[piece:]
    finally:
        if close:
            os.close(fd)


@pytest.mark.parametrize("nonblock", [False, True], ids=["blocking", "nonblock"])
@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("size", PAYLOAD_SIZES)
def test_read_full_exact(size, piece, nonblock):
    data = _payload(size)
    r, w = os.pipe()
    os.set_blocking(r, not nonblock)

    def writer():
        _write_in_pieces(w, data, piece, close=False)
        _write_in_pieces(w, b"TRAILER", 1 << 16)

    t = threading.Thread(target=writer)
    t.start()
    try:
        buf = bytearray(size + 16)
        buf[size:] = b"\xee" * 16
        rc = native_io.read_full(r, buf, size, 10_000)
        assert rc == native_io.OK
        assert bytes(buf[:size]) == data
        assert bytes(buf[size:]) == b"\xee" * 16, "wrote past n"
        # nothing past the n-th byte was consumed from the pipe
        os.set_blocking(r, True)
        t.join()
        assert os.read(r, 64) == b"TRAILER"
    finally:
        t.join()
        os.close(r)


def test_read_full_at_offset():
    r, w = os.pipe()
    os.write(w, b"abcdef")
    os.close(w)
    buf = bytearray(b"..........")
    assert native_io.read_full(r, buf, 6, 1000, offset=2) == native_io.OK
    os.close(r)
    assert bytes(buf) == b"..abcdef.."


@pytest.mark.parametrize("nonblock", [False, True], ids=["blocking", "nonblock"])
def test_read_full_eof_mid_read(nonblock):
    r, w = os.pipe()
    os.set_blocking(r, not nonblock)
    t = threading.Thread(target=_write_in_pieces, args=(w, _payload(1000), 333))
    t.start()
    buf = bytearray(4096)
    rc = native_io.read_full(r, buf, 4096, 10_000)
    t.join()
    os.close(r)
    assert rc == native_io.EOF
    assert bytes(buf[:1000]) == _payload(1000)


@pytest.mark.parametrize("nonblock", [False, True], ids=["blocking", "nonblock"])
def test_read_full_timeout(nonblock):
    r, w = os.pipe()
    os.set_blocking(r, not nonblock)
    os.write(w, b"xy")  # some bytes, then silence with the writer still open
    buf = bytearray(8)
    t0 = time.monotonic()
    rc = native_io.read_full(r, buf, 8, 50)
    waited = time.monotonic() - t0
    os.close(r)
    os.close(w)
    assert rc == native_io.TIMEOUT
    assert bytes(buf[:2]) == b"xy"
    assert waited < 5.0


def test_read_full_bad_fd_is_errno():
    r, w = os.pipe()
    os.close(r)
    os.close(w)
    assert native_io.read_full(r, bytearray(4), 4, 100) == -errno.EBADF


@pytest.mark.parametrize("nonblock", [False, True], ids=["blocking", "nonblock"])
@pytest.mark.parametrize("size", PAYLOAD_SIZES)
def test_write_full_slow_reader(size, nonblock):
    """The reader drains in small odd pieces with pauses, so the pipe
    fills and the writer has to wait (EAGAIN + poll when non-blocking)."""
    data = _payload(size)
    r, w = os.pipe()
    os.set_blocking(w, not nonblock)
    got = bytearray()

    def reader():
        n = 0
        while True:
            chunk = os.read(r, 65537)
            if not chunk:
                return
            got.extend(chunk)
            n += 1
            if n <= 3:
                time.sleep(0.01)  # let the 64 KiB pipe fill up first

    t = threading.Thread(target=reader)
    t.start()
    rc = native_io.write_full(w, data)
    os.close(w)
    t.join()
    os.close(r)
    assert rc == native_io.OK
    assert bytes(got) == data


def test_write_full_from_bytearray_window():
    r, w = os.pipe()
    assert native_io.write_full(w, bytearray(b"0123456789"), 4, offset=3) == native_io.OK
    os.close(w)
    assert os.read(r, 64) == b"3456"
    os.close(r)


def test_write_full_closed_reader_gives_epipe():
    """A closed reader is a return code, never a fatal SIGPIPE."""
    r, w = os.pipe()
    os.close(r)
    rc = native_io.write_full(w, _payload(1 << 17))
    os.close(w)
    assert rc == -errno.EPIPE
    assert native_io.strerror(rc) == os.strerror(errno.EPIPE)


def test_force_absent_returns_none(monkeypatch):
    monkeypatch.setattr(native_io, "force_absent", True)
    assert native_io.load() is None
    with pytest.raises(RuntimeError):
        native_io.read_full(0, bytearray(1), 1, 0)
