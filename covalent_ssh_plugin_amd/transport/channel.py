"""Long-lived framed channels over a transport.

A :class:`Channel` wraps one persistent remote process (a worker,
remote/worker_template.py) whose stdin/stdout carry 4-byte
length-prefixed frames (8-byte big-endian lengths: single tensor
buffers can exceed 4 GiB on a 288 GB HBM3E node).  Channels are how persistent workers are fed:
over SSH the process rides the pooled ControlMaster (no per-task
handshake), locally it is a plain subprocess — either way the remote
python + HIP runtime stay warm across electrons.
"""

from __future__ import annotations

import asyncio
import os
import struct
from typing import List, Optional

from . import native_io


class ChannelClosed(ConnectionError):
    """The remote worker process went away (EOF on its stdout)."""


class FrameParts:
    """The payload of ONE frame given as an ordered list of buffer-protocol
    parts (``pack_tensor_args``: the tensors of a packed argument arena and
    the zero padding between them, never copied into a second host buffer).
    ``nbytes`` is the total.  :meth:`Channel.send_frame` writes the 8-byte
    length of the total and then the parts in order."""

    # parts below SMALL are gathered into one write of up to about GATHER
    SMALL = 64 * 1024
    GATHER = 1 << 20

    def __init__(self, parts):
        self.parts = [memoryview(p).cast("B") for p in parts]
        self.nbytes = sum(p.nbytes for p in self.parts)

    def writes(self):
        """The payload as a sequence of buffers to write: runs of parts below
        ``SMALL`` coalesced into one ``bytes`` of at most about ``GATHER``,
        larger parts as they are (no copy)."""
        run = []
        size = 0
        for part in self.parts:
            if part.nbytes == 0:
                continue
            if part.nbytes >= self.SMALL:
                if run:
                    yield b"".join(run)
                    run, size = [], 0
                yield part
                continue
            run.append(part)
            size += part.nbytes
            if size >= self.GATHER:
                yield b"".join(run)
                run, size = [], 0
        if run:
            yield b"".join(run)

    def tobytes(self) -> bytes:
        return b"".join(self.parts)


class _PipeFrameReader(asyncio.Protocol):
    """Read side of a channel: the project's own protocol on the worker's
    stdout pipe (``loop.connect_read_pipe``) in place of a StreamReader.

    It buffers what the pipe transport delivers and hands out exact byte
    counts, like ``StreamReader.readexactly``.  Owning the buffer is what
    lets a large frame bypass it: the channel pauses the transport, takes
    what is already buffered for the frame (:meth:`take_into`) and reads
    the rest natively from the raw fd; nothing the transport read is ever
    out of reach, and bytes past the frame stay here for the next read.
    Without the native library :meth:`read_into` has ``data_received``
    copy each chunk straight into the destination."""

    # stop reading the pipe while this much is buffered and unclaimed
    FLOW_LIMIT = 8 << 20

    def __init__(self, loop: asyncio.AbstractEventLoop):
        self._loop = loop
        self._buf = bytearray()
        self._waiter: Optional[asyncio.Future] = None
        self._eof = False
        self._transport = None
        self._flow_paused = False
        self._held = False  # paused by the channel for a native read
        self._sink: Optional[memoryview] = None
        self._sink_pos = 0

    # -- asyncio.Protocol ----------------------------------------------
    def connection_made(self, transport) -> None:
        self._transport = transport

    def data_received(self, data: bytes) -> None:
        sink = self._sink
        if sink is not None:
            pos = self._sink_pos
            room = len(sink) - pos
            if len(data) <= room:
                sink[pos : pos + len(data)] = data
                self._sink_pos = pos + len(data)
            else:
                chunk = memoryview(data)
                sink[pos:] = chunk[:room]
                self._sink_pos = len(sink)
                self._buf += chunk[room:]
        else:
            self._buf += data
            if len(self._buf) > self.FLOW_LIMIT and not self._flow_paused:
                self._flow_paused = True
                self._apply_pause()
        self._wake()

    def eof_received(self) -> None:
        self._eof = True
        self._wake()

    def connection_lost(self, exc) -> None:
        self._eof = True
        self._wake()

    # -- flow control ----------------------------------------------------
    def _apply_pause(self) -> None:
        t = self._transport
        if t is None or t.is_closing():
            return
        if self._flow_paused or self._held:
            t.pause_reading()
        else:
            t.resume_reading()

    def _flow_resume(self) -> None:
        if self._flow_paused:
            self._flow_paused = False
            self._apply_pause()

    def hold(self) -> None:
        """Stop the transport from reading the fd (a native read owns it)."""
        self._held = True
        self._apply_pause()

    def release(self) -> None:
        self._held = False
        self._apply_pause()

    # -- reading -----------------------------------------------------------
    def _wake(self) -> None:
        w = self._waiter
        if w is not None and not w.done():
            w.set_result(None)

    async def _wait(self) -> None:
        if self._waiter is not None:
            raise RuntimeError("channel read side has two concurrent readers")
        self._waiter = self._loop.create_future()
        try:
            await self._waiter
        finally:
            self._waiter = None

    def at_eof(self) -> bool:
        return self._eof

    def fileno(self) -> Optional[int]:
        """The pipe's fd while the transport holds it open, else None."""
        t = self._transport
        if t is None or t.is_closing():
            return None
        pipe = t.get_extra_info("pipe")
        return None if pipe is None else pipe.fileno()

    async def readexactly(self, n: int) -> bytes:
        buf = self._buf
        while len(buf) < n:
            if self._eof:
                partial = bytes(buf)
                buf.clear()
                raise asyncio.IncompleteReadError(partial, n)
            self._flow_resume()  # the wanted bytes are still in the pipe
            await self._wait()
        if len(buf) == n:
            data = bytes(buf)
            buf.clear()
        else:
            data = bytes(memoryview(buf)[:n])
            del buf[:n]
        if self._flow_paused and len(buf) <= self.FLOW_LIMIT:
            self._flow_resume()
        return data

    def take_into(self, view: memoryview) -> int:
        """Move buffered bytes (at most ``len(view)``) to the front of
        ``view``; returns how many."""
        k = min(len(self._buf), len(view))
        if k:
            with memoryview(self._buf) as m:
                view[:k] = m[:k]
            del self._buf[:k]
            if self._flow_paused and len(self._buf) <= self.FLOW_LIMIT:
                self._flow_resume()
        return k

    async def read_into(self, view: memoryview) -> None:
        """Fill ``view`` completely: buffered bytes first, then each chunk
        the transport delivers is copied straight in."""
        n = len(view)
        pos = self.take_into(view)
        if pos == n:
            return
        self._sink, self._sink_pos = view, pos
        try:
            while self._sink_pos < n:
                if self._eof:
                    raise asyncio.IncompleteReadError(b"", n)
                self._flow_resume()
                await self._wait()
        finally:
            self._sink = None

    def close(self) -> None:
        t = self._transport
        if t is not None:
            try:
                t.close()
            except RuntimeError:
                pass  # transport's loop already closed


def _native_fill(fd: int, buf: bytearray, pos: int, nbytes: int, timeout_ms: int) -> int:
    """Executor-thread half of a large-frame receive: read ``nbytes`` from
    ``fd`` (a dup this call owns and closes) into ``buf[pos:]``."""
    try:
        return native_io.read_full(fd, buf, nbytes, timeout_ms, offset=pos)
    finally:
        os.close(fd)


class Channel:
    # Frames above this many bytes (tensor buffers) are received into one
    # preallocated destination, natively where libcsp_io.so is built.
    large_frame_threshold = 4 << 20
    # Longest wait for the next byte INSIDE a large frame before the
    # native read gives up (seconds): a dead peer cannot strand its thread.
    large_frame_idle_timeout = 300.0
    # Destination of a large frame: a huge-page-advised mapping from the
    # native library (first touch of fresh 4 KiB pages was a measured
    # share of the receive, profiles/staging_return_path.md) or a bytearray.
    large_frame_huge_pages = True

    def __init__(
        self,
        proc: asyncio.subprocess.Process,
        label: str = "worker",
        reader: Optional[_PipeFrameReader] = None,
    ):
        """``reader``: the read-side protocol on the process's stdout pipe
        (see :func:`spawn_channel_process`).  Without it the channel reads
        ``proc.stdout``, a StreamReader asyncio owns, the slower way."""
        self._proc = proc
        self._reader = reader
        self._broken = False  # a large frame was abandoned mid-read
        self._label = label
        self._lock = asyncio.Lock()  # guards the write side
        self._inflight = 0  # requests sent, replies not yet resolved
        self.loop = asyncio.get_event_loop()

    @property
    def alive(self) -> bool:
        return self._proc.returncode is None and not self._broken

    @property
    def inflight(self) -> int:
        return self._inflight

    async def send_frame(self, payload) -> None:
        """``payload`` is bytes or any buffer-protocol object (ctypes
        views of pinned/tensor memory go out without copies)."""
        if not self.alive:
            raise ChannelClosed(f"{self._label}: process exited")
        try:
            view = memoryview(payload).cast("B")
        except TypeError:
            # not a buffer: a FrameParts (off the hot path of plain frames)
            if not isinstance(payload, FrameParts):
                raise
            await self._send_parts(payload)
            return
        if view.nbytes <= 64 * 1024:
            # hot path (small control/request frames): one buffered write
            # instead of two halves the syscall/transport work per frame
            self._proc.stdin.write(struct.pack(">Q", view.nbytes) + view.tobytes())
        else:
            # large frames (tensor buffers): never copy
            self._proc.stdin.write(struct.pack(">Q", view.nbytes))
            self._proc.stdin.write(view)
        await self._proc.stdin.drain()

    async def _send_parts(self, payload: FrameParts) -> None:
        """One frame from many buffers: the length of the total, then the
        parts in order, small ones gathered, large ones never copied."""
        self._proc.stdin.write(struct.pack(">Q", payload.nbytes))
        for piece in payload.writes():
            self._proc.stdin.write(piece)
            if len(piece) >= FrameParts.SMALL:
                # keep the transport's buffer from holding the whole frame
                await self._proc.stdin.drain()
        await self._proc.stdin.drain()

    async def _recv_large(self, length: int):
        """One frame body above the threshold into ONE preallocated
        writable buffer (tensors reconstruct zero-copy on it).  With the native
        library: pause the pipe transport, move what the reader already
        buffered for this frame, read exactly the remainder from the raw
        fd on an executor thread, resume.  Exactly ``length`` bytes are
        consumed, so the next frame arrives through the normal path."""
        reader = self._reader
        buf = native_io.alloc_buffer(length) if self.large_frame_huge_pages else None
        if buf is None:
            buf = bytearray(length)
        view = memoryview(buf).cast("B")
        native = native_io.load() is not None and reader.fileno() is not None
        loop = asyncio.get_running_loop()
        complete = False
        if native:
            reader.hold()
        try:
            if not native:
                # no library on this host: the reader copies each chunk
                # the transport delivers straight into the destination
                await reader.read_into(view)
                complete = True
                return buf
            pos = reader.take_into(view)
            if pos < length:
                if reader.at_eof():
                    raise asyncio.IncompleteReadError(b"", length)
                # the thread gets its own dup: it stays valid (and reaches
                # EOF) even if this task is cancelled and the transport
                # closes the original under it
                fd = os.dup(reader.fileno())
                rc = await loop.run_in_executor(
                    None, _native_fill, fd, buf, pos, length - pos,
                    int(self.large_frame_idle_timeout * 1000),
                )
                if rc == native_io.EOF:
                    raise asyncio.IncompleteReadError(b"", length)
                if rc != native_io.OK:
                    raise ChannelClosed(
                        f"{self._label}: large-frame read failed: "
                        f"{native_io.strerror(rc)}"
                    )
            complete = True
            return buf
        finally:
            if complete:
                if native:
                    reader.release()
            else:
                # cancelled, timed out or failed mid-frame: the stream
                # position is lost for good — never reuse this channel
                self._broken = True
                self.kill()

    async def recv_frame(self, timeout: Optional[float] = None) -> bytes:
        async def _read() -> bytes:
            reader = self._reader
            if reader is None:
                return await self._read_stream_reader()
            header = await reader.readexactly(8)
            (length,) = struct.unpack(">Q", header)
            if length == 0:
                return b""
            if length <= self.large_frame_threshold:
                return await reader.readexactly(length)
            return await self._recv_large(length)

        if self._broken:
            raise ChannelClosed(f"{self._label}: channel abandoned mid-frame")
        try:
            if timeout is None:
                return await _read()
            return await asyncio.wait_for(_read(), timeout=timeout)
        except (asyncio.IncompleteReadError, ConnectionResetError) as e:
            raise ChannelClosed(f"{self._label}: EOF mid-frame") from e

    async def _read_stream_reader(self) -> bytes:
        """Receive path for a channel built on ``proc.stdout``."""
        header = await self._proc.stdout.readexactly(8)
        (length,) = struct.unpack(">Q", header)
        if length == 0:
            return b""
        if length <= self.large_frame_threshold:
            return await self._proc.stdout.readexactly(length)
        # large frame (tensor buffer): assemble into ONE preallocated
        # bytearray instead of readexactly's chunk-list + join + a
        # later bytearray copy — tensors reconstruct zero-copy on it
        buf = bytearray(length)
        view = memoryview(buf)
        pos = 0
        while pos < length:
            # read(remaining): takes the reader's ENTIRE internal
            # buffer in one pop.  Small fixed-size reads here are
            # quadratic — StreamReader deletes consumed bytes from
            # the front of its (up to 2*limit = 128 MiB) buffer, an
            # O(buffer) memmove per call.
            chunk = await self._proc.stdout.read(length - pos)
            if not chunk:
                raise asyncio.IncompleteReadError(bytes(view[:pos]), length)
            view[pos : pos + len(chunk)] = chunk
            pos += len(chunk)
        return buf

    async def request(self, payload: bytes, timeout: Optional[float] = None) -> bytes:
        """Serialized request/response round trip (single response frame)."""
        async with self._lock:
            await self.send_frame(payload)
            return await self.recv_frame(timeout=timeout)

    def transaction(self):
        """Async context manager holding the channel's request lock for a
        multi-frame exchange (e.g. a response followed by raw
        tensor-buffer frames)."""
        return _Transaction(self)

    # -- pipelined exchange --------------------------------------------
    #
    # The worker protocol is strictly ordered: responses come back in
    # request order.  ``exchange`` therefore only needs the write lock
    # while SENDING its request frames; replies are consumed by a single
    # reader pump that resolves waiter futures FIFO.  Over a real SSH
    # link this removes the one-RTT-per-electron serialization the
    # plain transaction() exchange pays.

    def _ensure_pump(self) -> None:
        if getattr(self, "_pump_task", None) is None or self._pump_task.done():
            self._waiters: "asyncio.Queue" = asyncio.Queue()
            self._pump_task = asyncio.get_running_loop().create_task(self._pump())

    def _fail_waiters(self, first=None) -> None:
        if first is not None and not first.done():
            first.set_exception(ChannelClosed(f"{self._label}: channel down"))
        waiters = getattr(self, "_waiters", None)
        while waiters is not None and not waiters.empty():
            w, _ = waiters.get_nowait()
            if not w.done():
                try:
                    w.set_exception(ChannelClosed(f"{self._label}: channel down"))
                except RuntimeError:
                    pass  # waiter's loop already gone

    async def _pump(self) -> None:
        fut = None
        try:
            while True:
                fut, reply_frames = await self._waiters.get()
                main = await self.recv_frame()
                extra_count = reply_frames(main)
                while extra_count is None:
                    # control frame (e.g. the worker's A1 execution ack)
                    # consumed by the callback: the real reply follows
                    main = await self.recv_frame()
                    extra_count = reply_frames(main)
                extras = [await self.recv_frame() for _ in range(extra_count)]
                if not fut.done():
                    fut.set_result((main, extras))
                fut = None
        except asyncio.CancelledError:
            # channel killed/closed: fail whatever is still waiting
            self._fail_waiters(fut)
            raise
        except Exception as e:  # noqa: BLE001 - fail this + later waiters
            if fut is not None and not fut.done():
                fut.set_exception(
                    e
                    if isinstance(e, ChannelClosed)
                    else ChannelClosed(f"{self._label}: reader failed: {e!r}")
                )
            self._fail_waiters()

    async def exchange(
        self,
        request_frames,
        reply_frames,
        timeout: Optional[float] = None,
    ):
        """Pipelined request/response.

        ``request_frames``: iterable of payloads sent back-to-back under
        the write lock.  ``reply_frames``: callable(main_frame) -> number
        of extra raw frames to read for this reply, or ``None`` to mean
        "that was a control frame; keep reading".  Returns
        ``(main_frame, [extra_frames])``.  Multiple callers may have
        requests in flight concurrently; replies resolve in order.
        """
        self._ensure_pump()
        fut = asyncio.get_running_loop().create_future()
        self._inflight += 1
        try:
            async with self._lock:
                self._waiters.put_nowait((fut, reply_frames))
                for frame in request_frames:
                    await self.send_frame(frame)
            if timeout is None:
                return await fut
            return await asyncio.wait_for(fut, timeout=timeout)
        finally:
            self._inflight -= 1

    def kill(self) -> None:
        """Synchronous hard-kill (for reaping workers whose event loop is
        already gone)."""
        task = getattr(self, "_pump_task", None)
        if task is not None and not task.done():
            try:
                task.cancel()
            except RuntimeError:
                pass  # task's loop already closed
        if self._proc.returncode is None:
            try:
                self._proc.kill()
            except ProcessLookupError:
                pass
        if self._reader is not None:
            self._reader.close()

    async def close(self) -> None:
        task = getattr(self, "_pump_task", None)
        if task is not None and not task.done():
            task.cancel()
        if self.loop is not asyncio.get_event_loop() or self.loop.is_closed():
            # channel belongs to another (likely closed) loop: its pipe
            # transports cannot be driven from here — hard-kill instead
            self.kill()
            return
        if self.alive:
            try:
                # zero-length frame = orderly shutdown
                self._proc.stdin.write(struct.pack(">Q", 0))
                await self._proc.stdin.drain()
                self._proc.stdin.close()
            except (ConnectionResetError, BrokenPipeError, RuntimeError):
                pass
            try:
                await asyncio.wait_for(self._proc.wait(), timeout=5)
            except asyncio.TimeoutError:
                self._proc.kill()
                await self._proc.wait()
        if self._reader is not None:
            self._reader.close()


class _Transaction:
    def __init__(self, channel: "Channel"):
        self._channel = channel

    async def __aenter__(self) -> "Channel":
        await self._channel._lock.acquire()
        return self._channel

    async def __aexit__(self, *exc) -> None:
        self._channel._lock.release()


async def spawn_channel_process(argv: List[str], label: str, **kwargs) -> Channel:
    """Start ``argv`` as a channel process: stdin through asyncio's
    subprocess pipe, stdout on a pipe of our own whose read end carries a
    :class:`_PipeFrameReader` (large frames can then be read natively
    from its fd).  stderr passes through to our logs."""
    loop = asyncio.get_running_loop()
    r_fd, w_fd = os.pipe()
    try:
        proc = await asyncio.create_subprocess_exec(
            *argv,
            stdin=asyncio.subprocess.PIPE,
            stdout=w_fd,
            stderr=None,
            limit=64 * 1024 * 1024,
            **kwargs,
        )
    except BaseException:
        os.close(r_fd)
        raise
    finally:
        os.close(w_fd)
    reader = _PipeFrameReader(loop)
    try:
        await loop.connect_read_pipe(lambda: reader, os.fdopen(r_fd, "rb", 0))
    except BaseException:
        proc.kill()
        raise
    return Channel(proc, label=label, reader=reader)


async def open_subprocess_channel(argv: List[str], label: str) -> Channel:
    return await spawn_channel_process(argv, label)
