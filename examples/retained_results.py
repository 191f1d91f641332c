#!/usr/bin/env python3
"""CUDA tensor results kept in worker HBM for reuse as arguments
(``retain_tensor_results=True``).

Electron A returns CUDA tensors, electron B takes them as arguments: the
common shape of a workflow.  With the option the worker keeps A's result
buffers as argument masters in HBM (one kernel launch gathers, copies and
checksums them), the dispatcher keys the bytes it received in the background,
and B's request names the held buffer instead of carrying its bytes.  The
script runs such a chain and prints what travelled.

``--measure`` turns it into the measurement behind
profiles/retained_results.md: the chain with the option on against off,
alternating, and ``csp_pack_checksum_dev`` against the calls it replaces.
``--measure-kernel`` is the kernel part alone; ``--lib`` loads another build
of the library and ``--cap`` sets the kernel's grid cap, for the store-kind
and grid-cap comparisons.  Needs a GPU on this host (local transport).
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
from covalent_ssh_plugin_amd.remote import workers as worker_pool  # noqa: E402

KIB = 1024
MIB = 1024 * KIB
STATE_SIZES = [4 * KIB, 256 * KIB, 4096 * KIB]  # cycled
STATE_TENSORS = 200


# -- the electrons -----------------------------------------------------------


def produce_one(nbytes, seed):
    """A: one large CUDA tensor."""
    import torch

    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.randint(0, 1 << 30, (nbytes // 4,), dtype=torch.int32, device="cuda",
                        generator=gen)
    torch.cuda.synchronize()
    return out


def produce_state(count, sizes, seed):
    """A: a ``state_dict``-like dict of small CUDA tensors."""
    import torch

    state = {}
    for i in range(count):
        n = sizes[i % len(sizes)] // 4
        state["param%03d" % i] = torch.full((n,), float(seed * 1000 + i), device="cuda")
    torch.cuda.synchronize()
    return state


def consume(value):
    """B: takes what A returned and answers with a few numbers about it."""
    import torch

    tensors = list(value.values()) if isinstance(value, dict) else [value]
    assert all(t.is_cuda for t in tensors)
    torch.cuda.synchronize()
    return [len(tensors), sum(t.numel() * t.element_size() for t in tensors),
            float(tensors[0].reshape(-1)[0]), float(tensors[-1].reshape(-1)[-1])]


def make_executor(home, cache, retain, **kwargs):
    return SSHExecutor(
        transport="local",
        local_home=home,
        cache_dir=cache,
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=True,
        arg_cache_bytes=8 << 30,
        pack_tensor_results=True,
        pack_tensor_args=True,
        patch_tensor_args=True,
        rebase_tensor_args=True,
        retain_tensor_results=retain,
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        **kwargs,
    )


def _counters(ex):
    names = ("arg_cache_hits", "arg_cache_misses", "arg_cache_bytes_saved",
             "arg_cache_rebases", "results_retained", "results_retained_bytes")
    return {name: ex.counters.get(name, 0) for name in names}


_keying_ms = []  # the background hash of each retained reply
_waited_ms = []  # each wait of a dispatch for such a hash


def time_the_keying():
    """Wrap the dispatcher's two keying functions so that the chain can say
    how long the background hash took and how long B waited for it."""
    key_retained = worker_pool._key_retained
    join = worker_pool.join_retained_keying

    def timed_key_retained(items):
        t0 = time.perf_counter()
        try:
            return key_retained(items)
        finally:
            _keying_ms.append((time.perf_counter() - t0) * 1000)

    async def timed_join(handle=None):
        t0 = time.perf_counter()
        await join(handle)
        _waited_ms.append((time.perf_counter() - t0) * 1000)

    worker_pool._key_retained = timed_key_retained
    worker_pool.join_retained_keying = timed_join


async def chain(ex, producer, producer_args, node_id):
    """A then B; the times are from before ``execute()`` until the result is
    in the caller's hands."""
    del _keying_ms[:], _waited_ms[:]
    t0 = time.perf_counter()
    value = await ex.execute(producer, producer_args, {}, dispatch_id="retain", node_id=node_id)
    a_ms = (time.perf_counter() - t0) * 1000
    meta_a = ex.last_task_record.remote_meta
    before = _counters(ex)
    t0 = time.perf_counter()
    answer = await ex.execute(consume, [value], {}, dispatch_id="retain", node_id=node_id + 1)
    b_ms = (time.perf_counter() - t0) * 1000
    meta_b = ex.last_task_record.remote_meta
    after = _counters(ex)
    return {
        "a_ms": a_ms,
        "b_ms": b_ms,
        "a_staging": meta_a.get("staging"),
        "a_retained": meta_a.get("retained"),
        "b_arg_staging": meta_b.get("arg_staging"),
        "b_counters": {k: after[k] - before[k] for k in after},
        # the background hash of A's result, and how long B waited for it
        "keying_ms": sum(_keying_ms),
        "b_waited_ms": sum(_waited_ms),
        "answer": answer,
    }


async def demo():
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        ex = make_executor(home, cache, retain=True)
        await chain(ex, produce_one, [64 * MIB, 1], 0)  # warms the worker
        one = await chain(ex, produce_one, [64 * MIB, 2], 2)
        state = await chain(ex, produce_state, [48, STATE_SIZES, 3], 4)
        await SSHExecutor.close_pool()
    for name, report in (("one 64 MiB tensor", one), ("48-tensor dict", state)):
        print(name)
        print("  A staging:", json.dumps(report["a_staging"]))
        print("  A retained:", json.dumps(report["a_retained"]))
        print("  B arg_staging:", json.dumps(report["b_arg_staging"]))
        print("  B counters:", json.dumps(report["b_counters"]))
        print("  A %.1f ms, B %.1f ms" % (report["a_ms"], report["b_ms"]))


# -- measurements ------------------------------------------------------------


def _med(values):
    return round(statistics.median(values), 4)


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1000, out


def kernel_layout(probe, count, sizes, reps):
    """csp_pack_checksum_dev against csp_pack_dev + csp_checksum_dev on one
    layout: host time of the calls (what the worker waits for), alternating,
    and the kernels' own time where the library reports it."""
    srcs = [
        torch.full((sizes[i % len(sizes)] // 4,), float(i), device="cuda")
        for i in range(count)
    ]
    nbytes = [t.numel() * 4 for t in srcs]
    offsets, total = probe.pack_layout(nbytes)
    arena = torch.empty(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    segments = [(t.data_ptr(), off, n) for t, off, n in zip(srcs, offsets, nbytes)]

    def fused():
        lib.csp_pack_checksum_dev(
            src, off, size, len(segments), arena.data_ptr(), total, out, None
        )
        return int(out[0]), int(out[1])

    def replaced():
        lib.csp_pack_dev(src, off, size, len(segments), arena.data_ptr(), total, None)
        return probe.checksum_device(arena.data_ptr(), total)

    # both sides as the worker calls them: the tables built beforehand, no
    # events around the launch
    lib = probe.load()
    src = (ctypes.c_void_p * len(segments))(*[s[0] for s in segments])
    off = (ctypes.c_uint64 * len(segments))(*offsets)
    size = (ctypes.c_uint64 * len(segments))(*nbytes)
    out = (ctypes.c_uint64 * 2)()
    assert fused() == replaced()  # and both are warm
    rows = {"fused": [], "replaced": [], "fused_kernel": [], "pack_kernel": []}
    for _ in range(reps):
        rows["fused"].append(_timed(fused)[0])
        rows["replaced"].append(_timed(replaced)[0])
        # the kernels' own times, from calls of their own
        rows["fused_kernel"].append(
            probe.pack_checksum_device(segments, arena.data_ptr(), total)["kernel_ms"]
        )
        rows["pack_kernel"].append(
            probe.pack_device(segments, arena.data_ptr(), total)["kernel_ms"]
        )
    return _summary(rows, {"segments": count, "bytes": sum(nbytes)})


def kernel_single(probe, nbytes, offset, reps):
    """One segment: csp_pack_checksum_dev against csp_copy_checksum_dev,
    which has no counterpart when the source is not 16-byte aligned."""
    src = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    src.random_(0, 256)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    segments = [(src.data_ptr() + offset, 0, nbytes)]

    # both sides as bare library calls: nothing but the call is timed
    lib = probe.load()
    one_src = (ctypes.c_void_p * 1)(src.data_ptr() + offset)
    one_off = (ctypes.c_uint64 * 1)(0)
    one_size = (ctypes.c_uint64 * 1)(nbytes)
    out = (ctypes.c_uint64 * 2)()

    def fused():
        lib.csp_pack_checksum_dev(one_src, one_off, one_size, 1, dst.data_ptr(), nbytes, out, None)
        return int(out[0]), int(out[1])

    def replaced():
        lib.csp_copy_checksum_dev(dst.data_ptr(), src.data_ptr(), nbytes, out)
        return int(out[0]), int(out[1])

    rows = {"fused": [], "fused_kernel": []}
    got = fused()
    if offset == 0:
        rows["replaced"] = []
        assert replaced() == got
    for _ in range(reps):
        rows["fused"].append(_timed(fused)[0])
        if offset == 0:
            rows["replaced"].append(_timed(replaced)[0])
        rows["fused_kernel"].append(
            probe.pack_checksum_device(segments, dst.data_ptr(), nbytes)["kernel_ms"]
        )
    return _summary(rows, {"bytes": nbytes, "source_offset": offset})


def _summary(rows, entry):
    for name, values in rows.items():
        entry[name + "_ms"] = _med(values)
        entry[name + "_ms_all"] = [round(v, 4) for v in values]
    if "replaced" in rows:
        spread = max(rows["replaced"]) - min(rows["replaced"])
        entry["replaced_spread_ms"] = round(spread, 4)
        entry["fused_minus_replaced_ms"] = round(
            statistics.median(rows["fused"]) - statistics.median(rows["replaced"]), 4
        )
    return entry


def measure_kernel(reps, lib_path="", cap=0):
    from covalent_ssh_plugin_amd.gpu import probe

    probe.load(lib_path)
    results = {"reps": reps, "lib": lib_path or "in-tree",
               "grid_cap": probe.pack_checksum_grid_cap(cap)}
    results["layouts"] = {
        "state_dict": kernel_layout(probe, STATE_TENSORS, STATE_SIZES, reps),
        "4MiB_only": kernel_layout(probe, 66, [4096 * KIB], reps),
        "200x4KiB": kernel_layout(probe, 200, [4 * KIB], reps),
    }
    results["single"] = {}
    for label, nbytes in (("16MiB", 16 * MIB), ("64MiB", 64 * MIB), ("1GiB", 1024 * MIB)):
        for offset in (0, 1):
            results["single"]["%s+%d" % (label, offset)] = kernel_single(
                probe, nbytes, offset, reps
            )
    probe.pack_checksum_grid_cap(0)
    return results


async def compare_chain(on, off, producer, producer_args, reps, node_id):
    rows = {"off": [], "on": []}
    for rep in range(reps + 1):  # the first pair warms workers and pools
        for name, ex in (("off", off), ("on", on)):
            args = list(producer_args) + [rep * 2 + (name == "on")]
            report = await chain(ex, producer, args, node_id)
            node_id += 2
            if rep:
                rows[name].append(report)
    entry = {}
    for name, reports in rows.items():
        entry[name] = {
            "a_ms": _med([r["a_ms"] for r in reports]),
            "a_ms_all": [round(r["a_ms"], 1) for r in reports],
            "b_ms": _med([r["b_ms"] for r in reports]),
            "b_ms_all": [round(r["b_ms"], 1) for r in reports],
            "a_staging": reports[-1]["a_staging"],
            "b_arg_staging": reports[-1]["b_arg_staging"],
            "b_counters": reports[-1]["b_counters"],
        }
    entry["on"]["keying_ms_all"] = [round(r["keying_ms"], 1) for r in rows["on"]]
    entry["on"]["b_waited_ms_all"] = [round(r["b_waited_ms"], 1) for r in rows["on"]]
    entry["b_ratio_on_over_off"] = round(entry["on"]["b_ms"] / entry["off"]["b_ms"], 4)
    off_a = [r["a_ms"] for r in rows["off"]]
    entry["a_off_spread_ms"] = round(max(off_a) - min(off_a), 1)
    entry["a_on_minus_off_ms"] = round(entry["on"]["a_ms"] - entry["off"]["a_ms"], 1)
    return entry, node_id


async def measure_chain(reps, big_bytes):
    results = {"reps": reps}
    time_the_keying()
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        off = make_executor(home, cache, retain=False)
        on = make_executor(home, cache, retain=True)
        results["one_tensor"], node_id = await compare_chain(
            on, off, produce_one, [big_bytes], reps, 0
        )
        results["one_tensor"]["bytes"] = big_bytes
        results["state_dict"], node_id = await compare_chain(
            on, off, produce_state, [STATE_TENSORS, STATE_SIZES], reps, node_id
        )
        await SSHExecutor.close_pool()
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--measure-kernel", action="store_true")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--lib", default="", help="another build of libcsp_gpu.so")
    parser.add_argument("--cap", type=int, default=0, help="grid cap (0: the default)")
    parser.add_argument("--big-bytes", type=int, default=1024 * MIB)
    parser.add_argument("--out", default="", help="also write the JSON here")
    args = parser.parse_args()
    if not (args.measure or args.measure_kernel):
        asyncio.run(demo())
        return
    if args.measure_kernel:
        results = measure_kernel(args.reps, args.lib, args.cap)
    else:
        results = asyncio.run(measure_chain(args.reps, args.big_bytes))
        results["kernel"] = measure_kernel(args.reps)
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
