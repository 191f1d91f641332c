#!/usr/bin/env python3
"""Many small tensor arguments as one frame (``pack_tensor_args=True``).

The electron below takes a ``state_dict``-like dict of CPU tensors, every one
below ``pinned_staging_threshold_bytes``.  With ``device_tensor_args`` alone
each tensor travels as its own frame and pays its own H2D stream and checksum
launch.  With ``pack_tensor_args`` they travel as ONE frame that lands in HBM
as one arena; one kernel launch scatters it into private per-tensor
allocations and verifies its checksum in the same pass.  With
``cache_tensor_args`` on top, the arena stays in HBM under one key and a
repeated dispatch sends no tensor bytes at all.  The script prints the
worker's ``arg_staging`` record and the phase timings of the dispatch.

``--measure`` turns it into the dispatch measurement behind
profiles/packed_args.md: baseline (``device_tensor_args`` alone), feature and
feature with the cache alternate on warm workers of their own, and the
medians of the ``execute()`` wall time are reported with all values.
``--kernel`` measures ``csp_unpack_checksum_dev`` alone at both candidate
grid caps beside ``csp_pack_dev``, ``csp_checksum_dev`` and the HBM copy
ceiling.  Both need a GPU on this host (local transport).
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

import torch  # noqa: E402  (loaded on the dispatcher: tensors are the arguments)

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402

KIB = 1024
STATE_SIZES = [4 * KIB, 256 * KIB, 4096 * KIB]  # cycled
# (name, tensors, sizes): the state_dict mix of profiles/packed_results.md,
# the small row, and totals between them that place pack_args_min_bytes
ROWS = [
    ("200_mix", 200, STATE_SIZES),
    ("16x4KiB", 16, [4 * KIB]),
    ("16x16KiB", 16, [16 * KIB]),
    ("64x16KiB", 64, [16 * KIB]),
    ("64x256KiB", 64, [256 * KIB]),
]
VARIANTS = ("baseline", "feature", "feature_cached")


def make_state(count, sizes):
    """``count`` fp32 CPU tensors whose byte sizes cycle through ``sizes``."""
    return {
        "param%03d" % i: torch.full((sizes[i % len(sizes)] // 4,), float(i))
        for i in range(count)
    }


def total_bytes(count, sizes):
    return sum(sizes[i % len(sizes)] for i in range(count))


def read_one_of_each(state):
    """The electron: one element of every tensor, and where they live."""
    first = torch.stack([t[0] for t in state.values()]).cpu()
    return {"first": first.tolist(), "cuda": all(t.is_cuda for t in state.values())}


def make_executor(root, variant, min_bytes=None):
    home = Path(root) / variant / "home"
    home.mkdir(parents=True)
    kwargs = {}
    if variant != "baseline":
        kwargs["pack_tensor_args"] = True
        if min_bytes is not None:
            kwargs["pack_args_min_bytes"] = min_bytes
    if variant == "feature_cached":
        # arg_cache_min_bytes stays at its default: arenas below it (the
        # small rows) are not cached and travel as in "feature"
        kwargs["cache_tensor_args"] = True
    return SSHExecutor(
        transport="local",
        local_home=str(home),
        cache_dir=str(Path(root) / variant / "cache"),
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        **kwargs,
    )


async def dispatch(ex, state, node_id):
    t0 = time.perf_counter()
    out = await ex.execute(read_one_of_each, [state], {}, dispatch_id="pargs", node_id=node_id)
    wall_ms = (time.perf_counter() - t0) * 1000
    assert out["cuda"] is True
    assert out["first"] == [float(i) for i in range(len(state))]
    record = ex.last_task_record
    meta = record.remote_meta
    return {
        "execute_ms": wall_ms,
        "phases_ms": {k: round(v * 1000, 3) for k, v in record.phases.items()},
        "arg_staging": meta.get("arg_staging"),
        "arg_cache": {
            k: len(v) if isinstance(v, list) else v
            for k, v in (meta.get("arg_cache") or {}).items()
        },
    }


async def demo():
    state = make_state(48, STATE_SIZES)
    with tempfile.TemporaryDirectory() as root:
        ex = make_executor(root, "feature_cached")
        for node_id in range(2):  # the second one is a cache hit
            report = await dispatch(ex, state, node_id)
        counters = dict(ex.counters)
        await SSHExecutor.close_pool()
    print("tensors in:", len(state), "of", total_bytes(48, STATE_SIZES), "bytes")
    print("arg_staging:", json.dumps(report["arg_staging"]))
    print("arg_cache:", json.dumps(report["arg_cache"]))
    print("counters:", json.dumps({k: v for k, v in counters.items() if "arg_cache" in k}))
    print("dispatcher phases (ms):", json.dumps(report["phases_ms"]))
    print("execute(): %.1f ms" % report["execute_ms"])


async def compare(executors, count, sizes, reps, node_id):
    state = make_state(count, sizes)  # the same objects every time
    rows = {name: [] for name in executors}
    for rep in range(reps + 1):  # the first round warms workers, pools and the cache
        for name, ex in executors.items():
            report = await dispatch(ex, state, node_id)
            node_id += 1
            if rep:
                rows[name].append(report)
    entry = {"tensors": count, "bytes": total_bytes(count, sizes)}
    for name, reports in rows.items():
        entry[name] = {
            "execute_ms": round(statistics.median(r["execute_ms"] for r in reports), 3),
            "execute_ms_all": [round(r["execute_ms"], 2) for r in reports],
            "stage_phase_ms": round(
                statistics.median(r["phases_ms"].get("stage", 0.0) for r in reports), 3
            ),
            "dispatch_phase_ms": round(
                statistics.median(r["phases_ms"].get("dispatch", 0.0) for r in reports), 3
            ),
            "arg_staging": reports[-1]["arg_staging"],
            "arg_cache": reports[-1]["arg_cache"],
        }
    return entry, node_id


async def measure(reps):
    results = {"reps": reps}
    with tempfile.TemporaryDirectory() as root:
        # packing forced on at every size: the rows place pack_args_min_bytes
        executors = {name: make_executor(root, name, min_bytes=0) for name in VARIANTS}
        node_id = 0
        for name, count, sizes in ROWS:
            results[name], node_id = await compare(executors, count, sizes, reps, node_id)
        results["counters_feature_cached"] = {
            k: v for k, v in executors["feature_cached"].counters.items() if "arg_cache" in k
        }
        await SSHExecutor.close_pool()
    return results


# -- the kernel alone ---------------------------------------------------------


def _median_call(fn, reps):
    fn()  # warm
    kernel, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1000)
        if isinstance(out, dict):
            kernel.append(out["kernel_ms"])
    row = {"call_ms": round(statistics.median(wall), 4)}
    if kernel:
        row["kernel_ms"] = round(statistics.median(kernel), 4)
        row["kernel_ms_all"] = [round(t, 4) for t in kernel]
    return row


def unpack_kernel(probe, count, sizes, reps):
    """csp_unpack_checksum_dev on an arena and destinations already in HBM,
    at both grid caps, beside csp_pack_dev on the same layout and
    csp_checksum_dev on the same arena."""
    nbytes = [sizes[i % len(sizes)] for i in range(count)]
    offsets, total = probe.pack_layout(nbytes)
    arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    dsts = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in nbytes]
    arena2 = torch.empty(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    segments = [(t.data_ptr(), off, n) for t, off, n in zip(dsts, offsets, nbytes)]
    row = {"segments": count, "bytes": total}
    want = probe.checksum_device(arena.data_ptr(), total)
    caps = (1024, 2048)
    kernel_ms = {cap: [] for cap in caps}
    call_ms = {cap: [] for cap in caps}
    try:
        for rep in range(reps + 1):  # the first round warms; the caps alternate
            for cap in caps:
                probe.unpack_checksum_grid_cap(cap)
                t0 = time.perf_counter()
                out = probe.unpack_checksum_device(arena.data_ptr(), total, segments)
                wall = (time.perf_counter() - t0) * 1000
                assert out["sum"] == want
                if rep:
                    kernel_ms[cap].append(out["kernel_ms"])
                    call_ms[cap].append(wall)
    finally:
        row["default_cap"] = probe.unpack_checksum_grid_cap(0)
    for cap in caps:
        ms = statistics.median(kernel_ms[cap])
        row["unpack_cap_%d" % cap] = {
            "call_ms": round(statistics.median(call_ms[cap]), 4),
            "kernel_ms": round(ms, 4),
            "kernel_ms_all": [round(t, 4) for t in kernel_ms[cap]],
            "gbps_read_plus_write": round(2 * total / (ms / 1000) / 1e9, 1),
        }
    assert torch.equal(dsts[-1], arena[offsets[-1] : offsets[-1] + nbytes[-1]])
    row["pack"] = _median_call(
        lambda: probe.pack_device(segments, arena2.data_ptr(), total), reps
    )
    assert torch.equal(arena2, arena)
    row["checksum"] = _median_call(
        lambda: probe.checksum_device(arena.data_ptr(), total), reps
    )
    return row


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


def kernel(reps):
    from covalent_ssh_plugin_amd.gpu import probe

    probe.load()
    return {
        "reps": reps,
        "66x4MiB": unpack_kernel(probe, 66, [4096 * KIB], reps),
        "200_mix": unpack_kernel(probe, 200, STATE_SIZES, reps),
        "200x4KiB": unpack_kernel(probe, 200, [4 * KIB], reps),
        "hbm_copy_gbps": hbm_copy_ceiling(probe),
    }


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--kernel", action="store_true")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default="", help="also write the JSON here")
    args = parser.parse_args()
    if not (args.measure or args.kernel):
        asyncio.run(demo())
        return
    results = {}
    if args.kernel:
        results["kernel"] = kernel(args.reps)
    if args.measure:
        results["dispatch"] = asyncio.run(measure(args.reps))
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
