"""Large frames through Channel.recv_frame: the native single-copy receive
and the pure-Python fallback must hand back every frame exact and in
order, consume nothing past a frame's end, and drop the channel when the
peer dies mid-frame."""

import asyncio
import sys
import time

import pytest

from covalent_ssh_plugin_amd.ops import build as ops_build
from covalent_ssh_plugin_amd.transport import native_io
from covalent_ssh_plugin_amd.transport.channel import (
    Channel,
    ChannelClosed,
    open_subprocess_channel,
)

LARGE = (1 << 20) + 3
THRESHOLD = 64 * 1024

# The fake worker: widens its stdout pipe so that ONE write can carry all
# three frames, then emits small + large patterned + small in that write.
FAKE_WORKER = r'''
import fcntl, os, struct, sys, time
LARGE = %(large)d
try:
    fcntl.fcntl(1, 1031, 4 << 20)  # F_SETPIPE_SZ
except OSError:
    pass
def frame(b):
    return struct.pack(">Q", len(b)) + b
def pattern(n):
    unit = bytes((i * 7 + 3) %% 251 for i in range(251))
    return (unit * (n // 251 + 1))[:n]
mode = sys.argv[1]
if mode == "three":
    blob = frame(b"first-small") + frame(pattern(LARGE)) + frame(b"last-small")
    view = memoryview(blob)
    n = os.write(1, view)          # the one write
    view = view[n:]
    while view:                    # only if the pipe could not be widened
        view = view[os.write(1, view):]
    sys.stdin.buffer.read()        # stay until the test closes us
elif mode == "die-mid-frame":
    os.write(1, frame(b"hello") + struct.pack(">Q", LARGE) + pattern(LARGE // 2))
    sys.stdin.buffer.readline()    # the test says when
    os._exit(9)
''' % {"large": LARGE}


def _pattern(n: int) -> bytes:
    unit = bytes((i * 7 + 3) % 251 for i in range(251))
    return (unit * (n // 251 + 1))[:n]


@pytest.fixture(params=["native", "native-bytearray", "fallback"])
def io_mode(request, monkeypatch):
    if request.param.startswith("native"):
        monkeypatch.setattr(
            Channel, "large_frame_huge_pages", request.param == "native"
        )
        ops_build.build_io(verbose=False)
        assert native_io.load() is not None, "libcsp_io.so did not load"
    else:
        monkeypatch.setattr(native_io, "force_absent", True)
        assert native_io.load() is None
    return request.param


@pytest.fixture
def worker_script(tmp_path):
    path = tmp_path / "fake_worker.py"
    path.write_text(FAKE_WORKER)
    return str(path)


async def _open(script: str, mode: str) -> Channel:
    ch = await open_subprocess_channel([sys.executable, script, mode], "fake")
    ch.large_frame_threshold = THRESHOLD
    return ch


@pytest.mark.parametrize("sleep_first", [False, True], ids=["prompt", "prebuffered"])
def test_three_frames_exact_and_in_order(worker_script, io_mode, sleep_first):
    async def run():
        ch = await _open(worker_script, "three")
        try:
            if sleep_first:
                # let the loop's pipe transport pull PART of the large
                # frame into the reader before anyone asks for it: a low
                # flow limit stops it there, the rest waits in the pipe
                ch._reader.FLOW_LIMIT = 128 * 1024
                await asyncio.sleep(0.3)
                buffered = len(ch._reader._buf)
                assert 128 * 1024 < buffered < LARGE
            first = await ch.recv_frame(timeout=10)
            large = await ch.recv_frame(timeout=10)
            last = await ch.recv_frame(timeout=10)
        finally:
            await ch.close()
        return first, large, last

    first, large, last = asyncio.run(run())
    assert first == b"first-small"
    assert not isinstance(large, bytes) and len(large) == LARGE  # writable
    assert bytes(large) == _pattern(LARGE)
    assert last == b"last-small"


def test_threshold_is_an_attribute_and_defaults_to_4mib():
    assert Channel.large_frame_threshold == 4 << 20


def test_peer_killed_mid_frame_raises_channel_closed(worker_script, io_mode):
    async def run():
        ch = await _open(worker_script, "die-mid-frame")
        try:
            assert await ch.recv_frame(timeout=10) == b"hello"
            task = asyncio.ensure_future(ch.recv_frame())
            await asyncio.sleep(0.2)  # the receive is inside the frame now
            assert not task.done()
            ch._proc.stdin.write(b"die\n")
            t0 = time.monotonic()
            with pytest.raises(ChannelClosed):
                await asyncio.wait_for(task, timeout=10)
            took = time.monotonic() - t0
            # a channel that lost a frame is never used again
            with pytest.raises(ChannelClosed):
                await ch.recv_frame(timeout=1)
        finally:
            ch.kill()
            await ch._proc.wait()
        return took

    assert asyncio.run(run()) < 10.0


def test_cancel_mid_frame_kills_the_channel(worker_script, io_mode):
    async def run():
        ch = await _open(worker_script, "die-mid-frame")
        try:
            assert await ch.recv_frame(timeout=10) == b"hello"
            with pytest.raises(asyncio.TimeoutError):
                await ch.recv_frame(timeout=0.2)  # peer stalls mid-frame
            assert not ch.alive
            with pytest.raises(ChannelClosed):
                await ch.recv_frame(timeout=1)
            with pytest.raises(ChannelClosed):
                await ch.send_frame(b"x")
        finally:
            ch.kill()
            await ch._proc.wait()

    asyncio.run(run())
