#!/usr/bin/env python3
"""A cached argument arena rebased to another layout (``rebase_tensor_args=True``).

The electron below takes a ``state_dict``-like dict of CPU tensors that
``pack_tensor_args`` sends as one arena and ``cache_tensor_args`` keeps in the
worker's HBM under one key.  ``patch_tensor_args`` sends a delta only while
the layout stays the same, and consumes the arena it patches.  With
``rebase_tensor_args`` a tensor may be added, removed or resized: the worker
builds the new arena as a new master from any arena it holds plus a delta of
the tensors that arena lacks, in the same kernel launch that scatters and
verifies it, and keeps the base.  The script resizes one tensor and adds one
between two dispatches, goes back to the first state, and prints the worker's
``arg_staging`` and ``arg_cache`` records.

``--measure`` turns it into the dispatch measurement behind
profiles/rebased_args.md: on two layouts one tensor changes its length before
every dispatch; the executor with the option on alternates with the same
executor with it off (another layout: a full store every time), each on a
warm worker of its own; medians of the ``execute()`` wall time with all
values.  ``--kernel`` measures ``csp_rebase_unpack_checksum_dev`` alone with
none, half and all segments from the delta, with and without a new master,
beside ``csp_unpack_checksum_dev`` and ``csp_patch_unpack_checksum_dev`` (all
segments patched) on the same layout, at both candidate grid caps,
alternating call by call.  Both need a GPU on this host (local transport).
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

KIB = 1024
STATE_SIZES = [4 * KIB, 256 * KIB, 4096 * KIB]  # cycled
# (name, tensors, sizes): the state_dict mix of profiles/packed_args.md and
# its uniform row
ROWS = [
    ("200_mix", 200, STATE_SIZES),
    ("64x256KiB", 64, [256 * KIB]),
]
VARIANTS = ("store", "rebase")


def make_state(count, sizes):
    """``count`` fp32 CPU tensors whose byte sizes cycle through ``sizes``."""
    return {
        "param%03d" % i: torch.full((sizes[i % len(sizes)] // 4,), float(i))
        for i in range(count)
    }


def nbytes_of(t):
    return t.numel() * t.element_size()


def read_one_of_each(state):
    """The electron: one element of every tensor, and where they live."""
    first = torch.stack([t[0] for t in state.values()]).cpu()
    return {"first": first.tolist(), "cuda": all(t.is_cuda for t in state.values())}


def make_executor(root, variant, min_bytes=None):
    home = Path(root) / variant / "home"
    home.mkdir(parents=True)
    kwargs = {}
    if min_bytes is not None:
        kwargs["pack_args_min_bytes"] = min_bytes
    return SSHExecutor(
        transport="local",
        local_home=str(home),
        cache_dir=str(Path(root) / variant / "cache"),
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        pack_tensor_args=True,
        cache_tensor_args=True,
        patch_tensor_args=True,
        rebase_tensor_args=(variant == "rebase"),
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        **kwargs,
    )


async def dispatch(ex, state, node_id):
    want = [float(t[0]) for t in state.values()]
    t0 = time.perf_counter()
    out = await ex.execute(read_one_of_each, [state], {}, dispatch_id="rebase", node_id=node_id)
    wall_ms = (time.perf_counter() - t0) * 1000
    assert out["cuda"] is True
    assert out["first"] == want
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
        ex = make_executor(root, "rebase")
        await dispatch(ex, state, 0)  # store
        other = dict(state)
        other["param001"] = torch.full((256 * KIB // 4 + 1,), 1.0)  # resized
        other["adapter"] = torch.full((1000,), 7.0)  # added
        report = await dispatch(ex, other, 1)  # rebase: two tensors travel
        back = await dispatch(ex, state, 2)  # the base is still held: a hit
        counters = dict(ex.counters)
        await SSHExecutor.close_pool()
    print("tensors in:", len(other), "of", sum(nbytes_of(t) for t in other.values()), "bytes")
    print("arg_staging:", json.dumps(report["arg_staging"]))
    print("arg_cache:", json.dumps(report["arg_cache"]))
    print("back to the first state, arg_cache:", json.dumps(back["arg_cache"]))
    print("counters:", json.dumps({k: v for k, v in counters.items() if "arg_cache" in k}))
    print("dispatcher phases (ms):", json.dumps(report["phases_ms"]))
    print("execute(): %.1f ms" % report["execute_ms"])


async def compare(executors, count, sizes, reps, node_id):
    state = make_state(count, sizes)
    name0 = next(iter(state))
    elems = state[name0].numel()
    version = 0
    rows = {name: [] for name in executors}
    for rep in range(reps + 1):  # the first round stores the arena and warms
        for name, ex in executors.items():
            if rep:
                # before EVERY dispatch: a length that no earlier dispatch
                # had (so no held arena has this layout and the variant
                # without the option cannot patch) and other values
                version += 1
                state[name0] = torch.full((elems + version,), float(version))
            report = await dispatch(ex, state, node_id)
            node_id += 1
            if rep:
                rows[name].append(report)
    entry = {
        "tensors": count, "bytes": sum(nbytes_of(t) for t in state.values()),
        "changed_tensors": 1, "changed_bytes": nbytes_of(state[name0]),
    }
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
            "read_ms": round(
                statistics.median(r["arg_staging"].get("read_ms", 0.0) for r in reports), 3
            ),
            "rebase_ms": round(
                statistics.median(r["arg_staging"].get("rebase_ms", 0.0) for r in reports), 3
            ),
            "unpack_ms": round(
                statistics.median(r["arg_staging"].get("unpack_ms", 0.0) for r in reports), 3
            ),
            "arg_staging": reports[-1]["arg_staging"],
            "arg_cache": reports[-1]["arg_cache"],
        }
    return entry, node_id


async def measure(reps):
    results = {"reps": reps}
    node_id = 0
    with tempfile.TemporaryDirectory() as root:
        # both variants leave a master behind on every dispatch; least
        # recently used ones go
        executors = {v: make_executor(root, v, min_bytes=0) for v in VARIANTS}
        for name, count, sizes in ROWS:
            results[name], node_id = await compare(executors, count, sizes, reps, node_id)
        for v in VARIANTS:
            results["counters_" + v] = {
                k: n for k, n in executors[v].counters.items() if "arg_cache" in k
            }
        await SSHExecutor.close_pool()
    return results


# -- the kernel alone ---------------------------------------------------------


def rebase_kernel(probe, count, sizes, reps):
    """csp_rebase_unpack_checksum_dev with none, half and all segments from
    the delta, with and without a new master, beside csp_unpack_checksum_dev
    and csp_patch_unpack_checksum_dev (all patched); every buffer already in
    HBM, at both grid caps, alternating call by call.  The new arena has the
    base's layout, so that the three kernels do the same scatter."""
    nbytes = [sizes[i % len(sizes)] for i in range(count)]
    offsets, total = probe.pack_layout(nbytes)
    base = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    master = base.clone()  # what the patch kernel overwrites
    out_arena = torch.empty(total, dtype=torch.uint8, device="cuda")
    dsts = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in nbytes]
    masks = {
        "none": [False] * count,
        "half": [k % 2 == 0 for k in range(count)],
        "all": [True] * count,
    }
    calls = {}
    for name, mask in masks.items():
        from_delta = [n for n, m in zip(nbytes, mask) if m]
        delta_offs, delta_bytes = probe.pack_layout(from_delta)
        delta = torch.randint(0, 256, (max(delta_bytes, 16),), dtype=torch.uint8, device="cuda")
        it = iter(delta_offs)
        segments = [
            (t.data_ptr(), off, n, None if m else off, next(it) if m else None)
            for t, off, n, m in zip(dsts, offsets, nbytes, mask)
        ]
        for kept, out_ptr in (("master", out_arena.data_ptr()), ("transient", 0)):
            calls["rebase_%s_%s" % (name, kept)] = (
                lambda d=delta, b=delta_bytes, s=segments, o=out_ptr:
                    probe.rebase_unpack_checksum_device(
                        base.data_ptr(), total, d.data_ptr() if b else 0, b, o, total, s
                    ),
                delta_bytes, total if out_ptr else 0,
            )
        if name == "all":
            patch_segments = [s[:3] + (s[4],) for s in segments]
            calls["patch_all"] = (
                lambda d=delta, b=delta_bytes, s=patch_segments:
                    probe.patch_unpack_checksum_device(
                        master.data_ptr(), total, d.data_ptr(), b, s
                    ),
                delta_bytes, delta_bytes,
            )
    plain = [(t.data_ptr(), off, n) for t, off, n in zip(dsts, offsets, nbytes)]
    calls["unpack"] = (
        lambda: probe.unpack_checksum_device(base.data_ptr(), total, plain), 0, 0
    )
    torch.cuda.synchronize()
    caps = (1024, 2048)
    kernel_ms = {(name, cap): [] for name in calls for cap in caps}
    try:
        for rep in range(reps + 1):  # the first round warms; everything alternates
            for name, (call, _delta_bytes, _written) in calls.items():
                for cap in caps:
                    probe.unpack_checksum_grid_cap(cap)
                    out = call()
                    if name.endswith("_master"):
                        assert out["sum"] == probe.checksum_device(out_arena.data_ptr(), total)
                    if rep:
                        kernel_ms[(name, cap)].append(out["kernel_ms"])
    finally:
        default_cap = probe.unpack_checksum_grid_cap(0)
    row = {"segments": count, "bytes": total, "default_cap": default_cap}
    for name, (_call, delta_bytes, written) in calls.items():
        for cap in caps:
            ms = statistics.median(kernel_ms[(name, cap)])
            # read the arena once (from the base or the delta), write the
            # destinations, and write the new master (or the patched part)
            moved = 2 * total + written
            row["%s_cap_%d" % (name, cap)] = {
                "delta_bytes": delta_bytes,
                "kernel_ms": round(ms, 4),
                "kernel_ms_all": [round(t, 4) for t in kernel_ms[(name, cap)]],
                "gbps_moved": round(moved / (ms / 1000) / 1e9, 1),
            }
    return row


def kernel(reps):
    from covalent_ssh_plugin_amd.gpu import probe

    probe.load()
    return {
        "reps": reps,
        "66x4MiB": rebase_kernel(probe, 66, [4096 * KIB], reps),
        "200_mix": rebase_kernel(probe, 200, STATE_SIZES, reps),
        "200x4KiB": rebase_kernel(probe, 200, [4 * KIB], reps),
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
