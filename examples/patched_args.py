#!/usr/bin/env python3
"""A cached argument arena patched in place (``patch_tensor_args=True``).

The electron below takes a ``state_dict``-like dict of CPU tensors that
``pack_tensor_args`` sends as one arena and ``cache_tensor_args`` keeps in the
worker's HBM under one key.  That cache only hits while no tensor changes: one
changed tensor gives the arena a new key and the whole arena travels again.
With ``patch_tensor_args`` an arena with the layout of one the worker holds
travels as a delta of the changed tensors alone; the worker writes them over
the held arena in place, in the same kernel launch that scatters and verifies
it.  The script changes three tensors between two dispatches and prints the
worker's ``arg_staging`` and ``arg_cache`` records.

``--measure`` turns it into the dispatch measurement behind
profiles/patched_args.md: on two layouts, with one tensor, about 10 % and
about 50 % of the bytes changed before every dispatch (so each pays the
content hash of what changed), the executor with the
option on alternates with the same executor with it off (a full store every
time), each on a warm worker of its own; medians of the ``execute()`` wall
time with all values.  ``--kernel`` measures ``csp_patch_unpack_checksum_dev``
alone with none, half and all segments patched beside
``csp_unpack_checksum_dev`` on the same layout, at both candidate grid caps,
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
SHARES = [("1_tensor", None), ("10_percent", 0.10), ("50_percent", 0.50)]
VARIANTS = ("store", "patch")


def make_state(count, sizes):
    """``count`` fp32 CPU tensors whose byte sizes cycle through ``sizes``."""
    return {
        "param%03d" % i: torch.full((sizes[i % len(sizes)] // 4,), float(i))
        for i in range(count)
    }


def nbytes_of(t):
    return t.numel() * t.element_size()


def pick_changed(state, share):
    """The names that change before every dispatch: the first tensor alone
    (``share`` None), else the largest tensors, in order, while their bytes
    stay at or below ``share`` of the total."""
    names = list(state)
    if share is None:
        return names[:1]
    budget = share * sum(nbytes_of(t) for t in state.values())
    picked, used = [], 0
    for name in sorted(names, key=lambda n: -nbytes_of(state[n])):
        if used + nbytes_of(state[name]) <= budget:
            picked.append(name)
            used += nbytes_of(state[name])
    return picked


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
        patch_tensor_args=(variant == "patch"),
        # one slot: every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        **kwargs,
    )


async def dispatch(ex, state, node_id):
    want = [float(t[0]) for t in state.values()]
    t0 = time.perf_counter()
    out = await ex.execute(read_one_of_each, [state], {}, dispatch_id="patch", node_id=node_id)
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
        ex = make_executor(root, "patch")
        await dispatch(ex, state, 0)  # store
        for name in ("param000", "param001", "param047"):
            state[name] = state[name] + 1
        report = await dispatch(ex, state, 1)  # patch: three tensors travel
        counters = dict(ex.counters)
        await SSHExecutor.close_pool()
    print("tensors in:", len(state), "of", sum(nbytes_of(t) for t in state.values()), "bytes")
    print("arg_staging:", json.dumps(report["arg_staging"]))
    print("arg_cache:", json.dumps(report["arg_cache"]))
    print("counters:", json.dumps({k: v for k, v in counters.items() if "arg_cache" in k}))
    print("dispatcher phases (ms):", json.dumps(report["phases_ms"]))
    print("execute(): %.1f ms" % report["execute_ms"])


async def compare(executors, count, sizes, share, reps, node_id):
    state = make_state(count, sizes)  # the same objects every time
    changed = pick_changed(state, share)
    rows = {name: [] for name in executors}
    for rep in range(reps + 1):  # the first round stores the arena and warms
        for name, ex in executors.items():
            if rep:
                # before EVERY dispatch, so that each variant hashes the
                # changed tensors itself (the key memo is per tensor object)
                for changed_name in changed:
                    state[changed_name].add_(1)  # a new version, a new key
            report = await dispatch(ex, state, node_id)
            node_id += 1
            if rep:
                rows[name].append(report)
    total = sum(nbytes_of(t) for t in state.values())
    entry = {
        "tensors": count, "bytes": total, "changed_tensors": len(changed),
        "changed_bytes": sum(nbytes_of(state[n]) for n in changed),
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
            "arg_staging": reports[-1]["arg_staging"],
            "arg_cache": reports[-1]["arg_cache"],
        }
    return entry, node_id


async def measure(reps):
    results = {"reps": reps}
    node_id = 0
    with tempfile.TemporaryDirectory() as root:
        # the store variant leaves a master behind on every dispatch, as the
        # cache without the option does; least recently used ones go
        executors = {v: make_executor(root, v, min_bytes=0) for v in VARIANTS}
        for name, count, sizes in ROWS:
            results[name] = {}
            for share_name, share in SHARES:
                results[name][share_name], node_id = await compare(
                    executors, count, sizes, share, reps, node_id
                )
        results["counters_patch"] = {
            k: v for k, v in executors["patch"].counters.items() if "arg_cache" in k
        }
        await SSHExecutor.close_pool()
    return results


# -- the kernel alone ---------------------------------------------------------


def patch_kernel(probe, count, sizes, reps):
    """csp_patch_unpack_checksum_dev with none, half and all segments patched
    beside csp_unpack_checksum_dev, master, delta and destinations already in
    HBM, at both grid caps, alternating call by call."""
    nbytes = [sizes[i % len(sizes)] for i in range(count)]
    offsets, total = probe.pack_layout(nbytes)
    master = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    dsts = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in nbytes]
    masks = {
        "none": [False] * count,
        "half": [k % 2 == 0 for k in range(count)],
        "all": [True] * count,
    }
    calls = {}
    for name, mask in masks.items():
        patched = [n for n, m in zip(nbytes, mask) if m]
        delta_offs, delta_bytes = probe.pack_layout(patched)
        delta = torch.randint(0, 256, (max(delta_bytes, 16),), dtype=torch.uint8, device="cuda")
        it = iter(delta_offs)
        segments = [
            (t.data_ptr(), off, n, next(it) if m else None)
            for t, off, n, m in zip(dsts, offsets, nbytes, mask)
        ]
        calls["patch_" + name] = (
            lambda d=delta, b=delta_bytes, s=segments: probe.patch_unpack_checksum_device(
                master.data_ptr(), total, d.data_ptr() if b else 0, b, s
            ),
            delta_bytes,
        )
    plain = [(t.data_ptr(), off, n) for t, off, n in zip(dsts, offsets, nbytes)]
    calls["unpack"] = (
        lambda: probe.unpack_checksum_device(master.data_ptr(), total, plain), 0
    )
    torch.cuda.synchronize()
    caps = (1024, 2048)
    kernel_ms = {(name, cap): [] for name in calls for cap in caps}
    try:
        for rep in range(reps + 1):  # the first round warms; everything alternates
            for name, (call, _delta_bytes) in calls.items():
                for cap in caps:
                    probe.unpack_checksum_grid_cap(cap)
                    out = call()
                    assert out["sum"] == probe.checksum_device(master.data_ptr(), total)
                    if rep:
                        kernel_ms[(name, cap)].append(out["kernel_ms"])
    finally:
        default_cap = probe.unpack_checksum_grid_cap(0)
    row = {"segments": count, "bytes": total, "default_cap": default_cap}
    for name, (_call, delta_bytes) in calls.items():
        for cap in caps:
            ms = statistics.median(kernel_ms[(name, cap)])
            # read the arena once (from the master or the delta), write the
            # destinations, and write the patched part of the master
            moved = 2 * total + delta_bytes
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
        "66x4MiB": patch_kernel(probe, 66, [4096 * KIB], reps),
        "200_mix": patch_kernel(probe, 200, STATE_SIZES, reps),
        "200x4KiB": patch_kernel(probe, 200, [4 * KIB], reps),
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
