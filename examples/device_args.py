#!/usr/bin/env python3
"""Tensor arguments that land in HBM (``device_tensor_args=True``).

The electron below receives its CPU tensor argument as a CUDA tensor: the
worker copied it to the GPU through a pinned ring while it was still being
received, and a kernel checked it there against the checksum the
dispatcher computed.  The script prints the worker's ``arg_staging`` record
and the phase timings of the dispatch.

``--measure`` turns it into the measurement behind
profiles/device_args_h2d.md: for each size it alternates the feature with
the behaviour without it (``device_tensor_args=False`` and the electron
calling ``.cuda()`` first thing) on one warm worker, and reports medians of
the time from dispatch start to the tensor being usable on the device,
plus the host checksum rate and the checksum kernel's time.  Needs a GPU
on this host (local transport).
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


def use_on_gpu(t):
    """The argument is (feature) or becomes (baseline) a CUDA tensor; the
    clock stops once it is usable on the device."""
    import time

    import torch

    arrived_on_device = t.is_cuda
    if not arrived_on_device:
        t = t.cuda()
    torch.cuda.synchronize()
    usable_at = time.time()
    return {
        "usable_at": usable_at,
        "arrived_on_device": arrived_on_device,
        "mean": float(t.float().mean()),
    }


def make_executor(home, cache, device_args):
    return SSHExecutor(
        transport="local",
        local_home=home,
        cache_dir=cache,
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=device_args,
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )


async def dispatch(ex, tensor, node_id):
    t0 = time.time()
    out = await ex.execute(use_on_gpu, [tensor], {}, dispatch_id="device-args", node_id=node_id)
    record = ex.last_task_record
    return {
        "to_usable_ms": (out["usable_at"] - t0) * 1000,
        "total_ms": record.total_s * 1000,
        "phases_ms": {k: round(v * 1000, 3) for k, v in record.phases.items()},
        "arg_staging": record.remote_meta.get("arg_staging"),
        "arrived_on_device": out["arrived_on_device"],
        "mean": out["mean"],
    }


async def demo(nbytes):
    tensor = torch.randn(nbytes // 4)
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        ex = make_executor(home, cache, device_args=True)
        for node_id in range(2):  # the second one meets a warm worker
            report = await dispatch(ex, tensor, node_id)
        await SSHExecutor.close_pool()
    print("mean on the GPU:", report["mean"], "(host:", float(tensor.mean()), ")")
    print("arg_staging:", json.dumps(report["arg_staging"]))
    print("dispatcher phases (ms):", json.dumps(report["phases_ms"]))
    print("dispatch start to usable on the device: %.1f ms" % report["to_usable_ms"])


def median(rows, key):
    return round(statistics.median(r[key] for r in rows), 3)


async def measure(sizes, reps):
    from covalent_ssh_plugin_amd.gpu import probe
    from covalent_ssh_plugin_amd.transport import native_io

    results = {"reps": reps, "sizes": {}}
    with tempfile.TemporaryDirectory() as home, tempfile.TemporaryDirectory() as cache:
        feature = make_executor(home, cache, device_args=True)
        baseline = make_executor(home, cache, device_args=False)
        node_id = 0
        for nbytes in sizes:
            tensor = torch.randn(nbytes // 4)
            rows = {"feature": [], "baseline": []}
            for rep in range(reps + 1):  # the first pair warms worker and pools
                for name, ex in (("baseline", baseline), ("feature", feature)):
                    report = await dispatch(ex, tensor, node_id)
                    node_id += 1
                    assert report["arrived_on_device"] == (name == "feature")
                    if rep:
                        rows[name].append(report)
            entry = {}
            for name in rows:
                entry[name] = {
                    "to_usable_ms": median(rows[name], "to_usable_ms"),
                    "to_usable_ms_all": [round(r["to_usable_ms"], 1) for r in rows[name]],
                    "stage_ms": round(
                        statistics.median(r["phases_ms"].get("stage", 0.0) for r in rows[name]), 3
                    ),
                }
            stages = [r["arg_staging"] for r in rows["feature"]]
            entry["feature"]["read_ms"] = median(stages, "read_ms")
            entry["feature"]["h2d_ms"] = median(stages, "h2d_ms")
            entry["feature"]["verified"] = stages[-1]["verified"]

            # the dispatcher's share: host checksum of the same bytes
            view = tensor.numpy()
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                native_io.checksum(view)
                times.append(time.perf_counter() - t0)
            host_s = statistics.median(times)
            entry["host_checksum_ms"] = round(host_s * 1000, 3)
            entry["host_checksum_gbps"] = round(nbytes / host_s / 1e9, 2)
            entry["host_checksum_share_of_dispatch"] = round(
                host_s * 1000 / entry["feature"]["to_usable_ms"], 3
            )
            results["sizes"][str(nbytes)] = entry
            del tensor
        await SSHExecutor.close_pool()

    # the kernel alone, on a buffer already in HBM (host clock around a call
    # that ends in a stream synchronise; includes the launch and the 16-byte
    # copy back)
    probe.load()
    for nbytes in sizes:
        dev = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        probe.checksum_device(dev.data_ptr(), nbytes)  # warm
        times = []
        for _ in range(max(reps, 5)):
            t0 = time.perf_counter()
            probe.checksum_device(dev.data_ptr(), nbytes)
            times.append(time.perf_counter() - t0)
        kernel_s = statistics.median(times)
        results["sizes"][str(nbytes)]["checksum_kernel_ms"] = round(kernel_s * 1000, 3)
        results["sizes"][str(nbytes)]["checksum_kernel_gbps"] = round(nbytes / kernel_s / 1e9, 1)
        del dev
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--mib", type=int, default=64, help="argument size for the demo")
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--sizes-mib", type=int, nargs="+", default=[64, 1024])
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--out", default="", help="also write the JSON here")
    args = parser.parse_args()
    if not args.measure:
        asyncio.run(demo(args.mib << 20))
        return
    results = asyncio.run(measure([m << 20 for m in args.sizes_mib], args.reps))
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
