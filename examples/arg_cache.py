#!/usr/bin/env python3
"""Repeated tensor arguments kept in worker HBM (``cache_tensor_args=True``).

The same tensor is fanned out to N electrons on one warm worker.  The first
one carries the bytes; the worker keeps them in HBM under a digest of their
content, and every later electron sends that digest alone and gets a private
copy made, and verified against a fresh checksum, by one kernel pass.  The
script prints the hit counters and each dispatch's time.

The measurements behind profiles/arg_cache.md:

``--measure``  p50 of one dispatch per size, alternating the option off (the
               behaviour without the feature) and on, first send and hit
               apart.  Needs a GPU on this host (local transport).
``--kernel``   csp_copy_checksum_dev against clone() + csp_checksum_dev, at
               both candidate grid caps.  Needs a GPU.
``--host``     blake2b key and threaded checksum rates at 1 and 8 threads.
               Host only.
"""

import argparse
import asyncio
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402  (loaded on the dispatcher: tensors are the arguments)

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402


def first_element(t):
    return {"cuda": t.is_cuda, "first": float(t.reshape(-1)[0])}


def make_executor(home, cache, cached, **overrides):
    options = dict(
        transport="local",
        local_home=home,
        cache_dir=cache,
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=cached,
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )
    options.update(overrides)
    return SSHExecutor(**options)


async def dispatch(ex, tensor, node_id):
    t0 = time.perf_counter()
    out = await ex.execute(first_element, [tensor], {}, dispatch_id="arg-cache", node_id=node_id)
    wall_ms = (time.perf_counter() - t0) * 1000
    assert out["cuda"] and out["first"] == float(tensor.reshape(-1)[0])
    record = ex.last_task_record
    return {
        "wall_ms": wall_ms,
        "stage_ms": record.phases.get("stage", 0.0) * 1000,
        "arg_staging": record.remote_meta.get("arg_staging"),
        "arg_cache": record.remote_meta.get("arg_cache"),
    }


async def demo(nbytes, fanout):
    weights = torch.randn(nbytes // 4)
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        ex = make_executor(home, cache, cached=True)
        for node_id in range(fanout):
            report = await dispatch(ex, weights, node_id)
            kind = "hit" if report["arg_cache"]["hits"] else "store"
            print(
                "electron %2d: %-5s %8.1f ms, %d bytes on the wire"
                % (node_id, kind, report["wall_ms"], report["arg_staging"]["bytes"])
            )
        print("counters:", json.dumps(ex.stats()["counters"]))
        await SSHExecutor.close_pool()


def p50(values):
    return round(statistics.median(values), 3)


async def measure(sizes, reps, min_bytes):
    results = {"reps": reps, "sizes": {}}
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        off = make_executor(home, cache, cached=False)
        on = make_executor(home, cache, cached=True, arg_cache_min_bytes=min_bytes)
        node_id = 0
        for nbytes in sizes:
            tensor = torch.randn(nbytes // 4)
            rows = {"off": [], "first_send": [], "hit": [], "hit_new_object": []}
            for rep in range(reps + 1):  # the first round warms workers and pools
                tensor[0] = float(rep)  # new content: the next send stores again
                plan = (
                    ("off", off, tensor),
                    ("first_send", on, tensor),
                    ("hit", on, tensor),  # same object: the key comes from the memo
                    ("hit_new_object", on, tensor.clone()),  # pays the hash again
                )
                for name, ex, arg in plan:
                    report = await dispatch(ex, arg, node_id)
                    node_id += 1
                    if name.startswith("hit"):
                        assert report["arg_staging"]["bytes"] == 0, report
                    elif name == "first_send":
                        assert report["arg_cache"]["stored"], report
                    if rep:
                        rows[name].append(report)
            entry = {}
            for name, reports in rows.items():
                entry[name] = {
                    "wall_ms_p50": p50(r["wall_ms"] for r in reports),
                    "wall_ms_all": [round(r["wall_ms"], 2) for r in reports],
                    "stage_ms_p50": p50(r["stage_ms"] for r in reports),
                }
            entry["hit_beats_off"] = entry["hit"]["wall_ms_p50"] < entry["off"]["wall_ms_p50"]
            results["sizes"][str(nbytes)] = entry
            del tensor
        results["counters"] = dict(on.counters)
        await SSHExecutor.close_pool()
    return results


def measure_kernel(sizes, reps):
    """Host clock around calls that end in a stream synchronise, so each
    figure includes the launch and the 16-byte copy back."""
    from covalent_ssh_plugin_amd.gpu import probe

    probe.load()
    results = {"reps": reps, "sizes": {}}

    def timed(fn):
        fn()  # warm
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return statistics.median(times)

    for nbytes in sizes:
        src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        entry = {}
        for cap in (1024, 2048):
            probe.copy_checksum_grid_cap(cap)
            s = timed(lambda: probe.copy_checksum_device(dst.data_ptr(), src.data_ptr(), nbytes))
            # GB/s of payload; the kernel moves twice that (one read, one write)
            entry["copy_checksum_cap%d" % cap] = {
                "ms": round(s * 1000, 3), "payload_gbps": round(nbytes / s / 1e9, 1),
            }
        probe.copy_checksum_grid_cap(0)
        assert torch.equal(src, dst)

        def clone_then_sum():
            copy = src.clone()
            torch.cuda.synchronize()
            probe.checksum_device(copy.data_ptr(), nbytes)

        s = timed(clone_then_sum)
        entry["clone_plus_checksum"] = {
            "ms": round(s * 1000, 3), "payload_gbps": round(nbytes / s / 1e9, 1),
        }
        s = timed(lambda: probe.checksum_device(src.data_ptr(), nbytes))
        entry["checksum_only"] = {
            "ms": round(s * 1000, 3), "payload_gbps": round(nbytes / s / 1e9, 1),
        }
        results["sizes"][str(nbytes)] = entry
        del src, dst
    return results


def measure_host(nbytes, reps):
    from covalent_ssh_plugin_amd.remote import workers
    from covalent_ssh_plugin_amd.transport import native_io

    data = torch.randint(0, 256, (nbytes,), dtype=torch.uint8).numpy()
    results = {"nbytes": nbytes, "reps": reps, "pool_threads": workers.hash_threads()}

    def rate(fn):
        fn()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return round(nbytes / statistics.median(times) / 1e9, 2)

    for threads in (1, 8):
        results["blake2b_key_gbps_%dt" % threads] = rate(
            lambda: workers.content_key(data, threads=threads)
        )
        if native_io.load() is not None:
            results["threaded_sum_gbps_%dt" % threads] = rate(
                lambda: workers.threaded_checksum(data, threads=threads)
            )
    if native_io.load() is not None:
        results["single_call_sum_gbps"] = rate(lambda: native_io.checksum(data))
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--mib", type=int, default=64, help="argument size for the demo")
    parser.add_argument("--fanout", type=int, default=8, help="electrons in the demo")
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--kernel", action="store_true")
    parser.add_argument("--host", action="store_true")
    parser.add_argument("--sizes-mib", type=int, nargs="+", default=[1, 16, 64, 1024])
    parser.add_argument("--min-bytes", type=int, default=1 << 20,
                        help="arg_cache_min_bytes for --measure")
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default="", help="also write the JSON here")
    args = parser.parse_args()
    sizes = [m << 20 for m in args.sizes_mib]
    if args.measure:
        results = asyncio.run(measure(sizes, args.reps, args.min_bytes))
    elif args.kernel:
        results = measure_kernel(sizes, args.reps)
    elif args.host:
        results = measure_host(max(sizes), args.reps)
    else:
        asyncio.run(demo(args.mib << 20, args.fanout))
        return
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
