#!/usr/bin/env python3
"""Per-stage timing of the large-result return path (bench config
``staging``): where do the milliseconds of a 1 GiB CUDA tensor result go?

Each stage runs in isolation on one MI355X, warm-up first, then ``--reps``
timed repetitions (median, min, max):

  (a)  pinned D2H of the payload (csp_memcpy_d2h into a pooled block)
  (b)  the worker-style pipe write (1 MiB os.write pieces from a reused
       buffer) into a C sink (``cat > /dev/null``)
  (c)  Channel.recv_frame on a StreamReader-backed channel — the receive
       path before the native one — fed by a C source (``head -c`` from
       /dev/zero behind a frame header)
  (c') the same frames through the channel's own pipe reader, with the
       native library and with it forced absent (only where the tree has
       them)
  (d)  allocating and first-touching the destination (bytearray, and the
       huge-page-advised csp_io_alloc where the tree has it)
  (s)  csp_d2h_stream_fd of the payload into the C sink, per chunk size
       (only where the tree has it)

The C source and sink are coreutils, so the same script measures a tree
from before the native library existed.  Prints a markdown table; with
``--out FILE`` also writes it there.

Usage: python tools/staging_stages.py [--mib 1024] [--reps 5] [--out FILE]
"""

from __future__ import annotations

import argparse
import asyncio
import ctypes
import fcntl
import os
import statistics
import subprocess
import sys
import time

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

F_SETPIPE_SZ = 1031
ROWS = []


def report(stage: str, what: str, times_s, nbytes: int) -> None:
    ms = sorted(t * 1000.0 for t in times_s)
    med = statistics.median(ms)
    gbps = nbytes / (med / 1000.0) / 1e9 if med > 0 else float("inf")
    row = (stage, what, f"{med:.1f}", f"{ms[0]:.1f}", f"{ms[-1]:.1f}", f"{gbps:.2f}")
    ROWS.append(row)
    print("| " + " | ".join(row) + " |", flush=True)


def widen(fd: int) -> None:
    try:
        fcntl.fcntl(fd, F_SETPIPE_SZ, 1 << 20)  # what the worker does
    except OSError:
        pass


def c_sink():
    """A child that drains its stdin as fast as C can; returns (proc, fd)."""
    proc = subprocess.Popen(["cat"], stdin=subprocess.PIPE, stdout=subprocess.DEVNULL)
    fd = proc.stdin.fileno()
    widen(fd)
    return proc, fd


def frame_source_script(nbytes: int, frames: int) -> str:
    """bash: ``frames`` times an 8-byte big-endian header + nbytes zeros."""
    header = "".join("\\%03o" % b for b in nbytes.to_bytes(8, "big"))
    return (
        f"for i in $(seq {frames}); do printf '{header}'; "
        f"head -c {nbytes} /dev/zero; done"
    )


def stage_d2h(lib, torch, nbytes, warm, reps):
    t = torch.ones(nbytes // 2, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    dst = lib.csp_staging_alloc(nbytes)
    assert dst, "csp_staging_alloc failed"
    times = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        rc = lib.csp_memcpy_d2h(ctypes.c_void_p(dst), ctypes.c_void_p(t.data_ptr()), nbytes)
        dt = time.perf_counter() - t0
        assert rc == 0
        if i >= warm:
            times.append(dt)
    lib.csp_staging_release_all()
    report("a", "pinned D2H (csp_memcpy_d2h)", times, nbytes)
    return t


def stage_pipe_write(nbytes, warm, reps):
    buf = bytearray(nbytes)
    buf[::4096] = b"\x01" * len(buf[::4096])  # resident before timing
    proc, fd = c_sink()
    times = []
    for i in range(warm + reps):
        view = memoryview(buf)
        t0 = time.perf_counter()
        while view:
            view = view[os.write(fd, view[: 1 << 20]):]
        dt = time.perf_counter() - t0
        if i >= warm:
            times.append(dt)
    proc.stdin.close()
    proc.wait()
    report("b", "worker-style pipe write, 1 MiB pieces, C sink", times, nbytes)


async def _recv_frames(make_channel, nbytes, warm, reps):
    ch = await make_channel(["bash", "-c", frame_source_script(nbytes, warm + reps)])
    times = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        frame = await ch.recv_frame()
        dt = time.perf_counter() - t0
        assert len(frame) == nbytes
        del frame
        if i >= warm:
            times.append(dt)
    ch.kill()
    await ch._proc.wait()
    return times


def stage_recv(nbytes, warm, reps):
    from covalent_ssh_plugin_amd.transport import channel as channel_mod

    async def stream_reader_channel(argv):
        proc = await asyncio.create_subprocess_exec(
            *argv, stdin=asyncio.subprocess.PIPE, stdout=asyncio.subprocess.PIPE,
            limit=64 * 1024 * 1024,
        )
        return channel_mod.Channel(proc, label="stages")

    times = asyncio.run(_recv_frames(stream_reader_channel, nbytes, warm, reps))
    report("c", "Channel.recv_frame, StreamReader path, C source", times, nbytes)

    if not hasattr(channel_mod, "spawn_channel_process"):
        return
    from covalent_ssh_plugin_amd.transport import native_io

    async def own_reader_channel(argv):
        return await channel_mod.spawn_channel_process(argv, label="stages")

    if native_io.load() is not None:
        default = channel_mod.Channel.large_frame_huge_pages
        for huge, dest in ((False, "a bytearray"), (True, "a huge-page mapping")):
            channel_mod.Channel.large_frame_huge_pages = huge
            try:
                times = asyncio.run(_recv_frames(own_reader_channel, nbytes, warm, reps))
            finally:
                channel_mod.Channel.large_frame_huge_pages = default
            report("c'", f"Channel.recv_frame, native read into {dest}", times, nbytes)
    native_io.force_absent = True
    try:
        times = asyncio.run(_recv_frames(own_reader_channel, nbytes, warm, reps))
    finally:
        native_io.force_absent = False
    report("c'", "Channel.recv_frame, own reader, library absent", times, nbytes)


def stage_alloc(nbytes, warm, reps):
    times, free_times = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        buf = bytearray(nbytes)
        view = memoryview(buf)
        touched = 0
        for off in range(0, nbytes, 1 << 26):  # touch every page, 64 MiB at a time
            part = view[off : off + (1 << 26) : 4096]
            part[:] = b"\x01" * len(part)
            touched += len(part)
        dt = time.perf_counter() - t0
        del part, view
        t1 = time.perf_counter()
        del buf
        dfree = time.perf_counter() - t1
        if i >= warm:
            times.append(dt)
            free_times.append(dfree)
    report("d", "bytearray(n) + first touch of every 4 KiB page", times, nbytes)
    report("d", "freeing that bytearray", free_times, nbytes)

    try:
        from covalent_ssh_plugin_amd.transport import native_io
    except ImportError:
        return
    lib = native_io.load()
    if lib is None:
        return
    times, free_times = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        p = lib.csp_io_alloc(nbytes)
        assert p
        arr = (ctypes.c_char * nbytes).from_address(p)
        view = memoryview(arr).cast("B")
        for off in range(0, nbytes, 1 << 26):
            part = view[off : off + (1 << 26) : 4096]
            part[:] = b"\x01" * len(part)
        dt = time.perf_counter() - t0
        del part, view, arr
        t1 = time.perf_counter()
        lib.csp_io_free(p, nbytes)
        dfree = time.perf_counter() - t1
        if i >= warm:
            times.append(dt)
            free_times.append(dfree)
    report("d", "csp_io_alloc (mmap + MADV_HUGEPAGE) + first touch", times, nbytes)
    report("d", "csp_io_free", free_times, nbytes)


def stage_stream(lib, src_tensor, nbytes, warm, reps):
    if not hasattr(lib, "csp_d2h_stream_fd"):
        return
    from covalent_ssh_plugin_amd.gpu import probe

    for chunk_mib in (1, 4, 16, 64):
        proc, fd = c_sink()
        times, d2h, wr = [], [], []
        for i in range(warm + reps):
            t0 = time.perf_counter()
            rep = probe.stream_d2h_to_fd(fd, src_tensor.data_ptr(), nbytes, chunk_mib << 20)
            dt = time.perf_counter() - t0
            assert rep["rc"] == 0, rep
            if i >= warm:
                times.append(dt)
                d2h.append(rep["d2h_ms"])
                wr.append(rep["write_ms"])
        proc.stdin.close()
        proc.wait()
        report(
            "s",
            f"csp_d2h_stream_fd, {chunk_mib} MiB chunks, C sink "
            f"(copy engine {statistics.median(d2h):.1f} ms, in write() "
            f"{statistics.median(wr):.1f} ms)",
            times, nbytes,
        )


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--stages", default="abcds")
    args = ap.parse_args()
    nbytes = args.mib << 20
    warm, reps = args.warmup, max(5, args.reps)

    try:
        with open("/sys/kernel/mm/transparent_hugepage/enabled") as f:
            print("transparent_hugepage:", f.read().strip())
    except OSError:
        pass
    print(f"payload {args.mib} MiB, warm-up {warm}, repetitions {reps}")
    print("| stage | what | median ms | min ms | max ms | GB/s at median |")
    print("|---|---|---|---|---|---|", flush=True)

    src = None
    lib = None
    if "a" in args.stages or "s" in args.stages:
        import torch

        from covalent_ssh_plugin_amd.gpu import probe

        lib = probe.load()
        src = stage_d2h(lib, torch, nbytes, warm, reps)
    if "b" in args.stages:
        stage_pipe_write(nbytes, warm, reps)
    if "c" in args.stages:
        stage_recv(nbytes, warm, reps)
    if "d" in args.stages:
        stage_alloc(nbytes, warm, reps)
    if "s" in args.stages and lib is not None:
        stage_stream(lib, src, nbytes, warm, reps)

    if args.out:
        with open(args.out, "w") as f:
            f.write("| stage | what | median ms | min ms | max ms | GB/s at median |\n")
            f.write("|---|---|---|---|---|---|\n")
            for row in ROWS:
                f.write("| " + " | ".join(row) + " |\n")


if __name__ == "__main__":
    main()
