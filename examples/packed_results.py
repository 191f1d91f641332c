#!/usr/bin/env python3
"""Many small CUDA tensors back as one frame (``pack_tensor_results=True``).

The electron below returns a ``state_dict``-like dict of CUDA tensors, every
one below ``pinned_staging_threshold_bytes``.  With the option the worker
gathers them on the GPU into one arena (one kernel launch), checksums it
there and streams it as a single frame; the dispatcher verifies the checksum
and hands back views into the received buffer.  The script prints the
worker's ``staging`` record and the phase timings of the dispatch.

``--measure`` turns it into the measurement behind
profiles/packed_results.md: it alternates the feature with the behaviour
without it (every tensor through its own ``.cpu()`` and the pickle) on warm
workers and reports medians of the time from before ``execute()`` until the
result is in the caller's hands, the worker's ``staging`` phase, the pack
kernel's own time beside the HBM copy ceiling, and the dispatcher's checksum
time.  Needs a GPU on this host (local transport).
"""

import argparse
import asyncio
import ctypes
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402  (loaded on the dispatcher: tensors are the result)

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402

KIB = 1024
STATE_SIZES = [4 * KIB, 256 * KIB, 4096 * KIB]  # cycled
STATE_TENSORS = 200
SMALL_SIZES = [16 * KIB]
SMALL_TENSORS = 16


def make_state(count, sizes):
    """``count`` fp32 CUDA tensors whose byte sizes cycle through ``sizes``."""
    import torch

    state = {}
    for i in range(count):
        n = sizes[i % len(sizes)] // 4
        state["param%03d" % i] = torch.full((n,), float(i), device="cuda")
    torch.cuda.synchronize()
    return state


def total_bytes(count, sizes):
    return sum(sizes[i % len(sizes)] for i in range(count))


def make_executor(home, cache, pack, min_bytes=None):
    kwargs = {}
    if min_bytes is not None:
        kwargs["pack_results_min_bytes"] = min_bytes
    return SSHExecutor(
        transport="local",
        local_home=home,
        cache_dir=cache,
        python_path=sys.executable,
        persistent_workers=True,
        pack_tensor_results=pack,
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        **kwargs,
    )


def check(state, count, sizes):
    assert len(state) == count
    for i in (0, 1, 2, count - 1):
        t = state["param%03d" % i]
        assert t.numel() == sizes[i % len(sizes)] // 4
        assert float(t[0]) == float(i) and float(t[-1]) == float(i)


async def dispatch(ex, count, sizes, node_id):
    t0 = time.perf_counter()
    state = await ex.execute(make_state, [count, sizes], {}, dispatch_id="packed", node_id=node_id)
    in_hand_ms = (time.perf_counter() - t0) * 1000
    check(state, count, sizes)
    record = ex.last_task_record
    meta = record.remote_meta
    return {
        "in_hand_ms": in_hand_ms,
        "phases_ms": {k: round(v * 1000, 3) for k, v in record.phases.items()},
        "worker_staging_ms": meta["phases_ms"].get("staging"),
        "staging": meta.get("staging"),
        "result_integrity": meta.get("result_integrity"),
        "buffers": len(meta.get("buffers", [])),
    }


async def demo():
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        ex = make_executor(home, cache, pack=True)
        for node_id in range(2):  # the second one meets a warm worker
            report = await dispatch(ex, 48, STATE_SIZES, node_id)
        await SSHExecutor.close_pool()
    print("tensors back:", 48, "in", report["buffers"], "out-of-band buffer(s)")
    print("staging:", json.dumps(report["staging"]))
    print("result_integrity:", json.dumps(report["result_integrity"]))
    print("dispatcher phases (ms):", json.dumps(report["phases_ms"]))
    print("execute() to result in hand: %.1f ms" % report["in_hand_ms"])


def median(rows, key):
    return round(statistics.median(r[key] for r in rows), 3)


async def compare(feature, baseline, count, sizes, reps, node_id):
    rows = {"baseline": [], "feature": []}
    for rep in range(reps + 1):  # the first pair warms workers and pools
        for name, ex in (("baseline", baseline), ("feature", feature)):
            report = await dispatch(ex, count, sizes, node_id)
            node_id += 1
            if rep:
                rows[name].append(report)
    entry = {"tensors": count, "bytes": total_bytes(count, sizes)}
    for name in rows:
        entry[name] = {
            "in_hand_ms": median(rows[name], "in_hand_ms"),
            "in_hand_ms_all": [round(r["in_hand_ms"], 1) for r in rows[name]],
            "worker_staging_ms": median(rows[name], "worker_staging_ms"),
            "dispatch_phase_ms": round(
                statistics.median(r["phases_ms"].get("dispatch", 0.0) for r in rows[name]), 3
            ),
            "staging": rows[name][-1]["staging"],
            "buffers": rows[name][-1]["buffers"],
        }
    entry["feature"]["result_integrity"] = rows["feature"][-1]["result_integrity"]
    return entry, node_id


def pack_kernel(probe, count, sizes, reps):
    """The pack kernel alone on sources already in HBM: median kernel_ms and
    the rate it implies, bytes read plus bytes written."""
    srcs = [
        torch.full((sizes[i % len(sizes)] // 4,), float(i), device="cuda")
        for i in range(count)
    ]
    nbytes = [t.numel() * 4 for t in srcs]
    offsets, total = probe.pack_layout(nbytes)
    arena = torch.empty(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    segments = [(t.data_ptr(), off, n) for t, off, n in zip(srcs, offsets, nbytes)]
    probe.pack_device(segments, arena.data_ptr(), total)  # warm
    times = [
        probe.pack_device(segments, arena.data_ptr(), total)["kernel_ms"]
        for _ in range(max(reps, 5))
    ]
    assert float(arena[offsets[-1] : offsets[-1] + 4].view(torch.float32)[0]) == float(count - 1)
    ms = statistics.median(times)
    return {
        "segments": count,
        "bytes": sum(nbytes),
        "kernel_ms": round(ms, 4),
        "kernel_ms_all": [round(t, 4) for t in times],
        "gbps_read_plus_write": round(2 * sum(nbytes) / (ms / 1000) / 1e9, 1),
    }


def hbm_copy_ceiling(probe):
    """csp_hbm_bench at the library's default sweep variant: GB/s, bytes read
    plus bytes written, of a plain 1 GiB device copy."""
    lib = probe.load()
    lib.csp_hbm_bench.restype = ctypes.c_int
    lib.csp_hbm_bench.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
        ctypes.POINTER(ctypes.c_double),
    ]
    gbps = ctypes.c_double()
    rc = lib.csp_hbm_bench(0, -1, 1 << 30, 6, ctypes.byref(gbps))
    if rc != 0:
        raise RuntimeError(lib.csp_last_error().decode(errors="replace"))
    return round(gbps.value, 1)


async def measure(reps):
    from covalent_ssh_plugin_amd.gpu import probe
    from covalent_ssh_plugin_amd.transport import native_io

    results = {"reps": reps}
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        baseline = make_executor(home, cache, pack=False)
        feature = make_executor(home, cache, pack=True)
        results["state_dict"], node_id = await compare(
            feature, baseline, STATE_TENSORS, STATE_SIZES, reps, 0
        )
        # is the pack_results_min_bytes default on the right side?  packing
        # forced on a result a few times its size
        forced = make_executor(home, cache, pack=True, min_bytes=0)
        results["small"], node_id = await compare(
            forced, baseline, SMALL_TENSORS, SMALL_SIZES, reps, node_id
        )
        await SSHExecutor.close_pool()

    # the dispatcher's share: host checksum of an arena-sized buffer
    arena_bytes = results["state_dict"]["bytes"]
    view = torch.zeros(arena_bytes, dtype=torch.uint8).numpy()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        native_io.checksum(view)
        times.append(time.perf_counter() - t0)
    host_s = statistics.median(times)
    results["host_checksum_ms"] = round(host_s * 1000, 3)
    results["host_checksum_gbps"] = round(arena_bytes / host_s / 1e9, 2)
    results["host_checksum_share_of_dispatch"] = round(
        host_s * 1000 / results["state_dict"]["feature"]["in_hand_ms"], 4
    )

    probe.load()
    results["pack_kernel"] = {
        "state_dict": pack_kernel(probe, STATE_TENSORS, STATE_SIZES, reps),
        "4MiB_only": pack_kernel(probe, 66, [4096 * KIB], reps),
        "200x4KiB": pack_kernel(probe, 200, [4 * KIB], reps),
    }
    results["hbm_copy_gbps"] = hbm_copy_ceiling(probe)
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default="", help="also write the JSON here")
    args = parser.parse_args()
    if not args.measure:
        asyncio.run(demo())
        return
    results = asyncio.run(measure(args.reps))
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
