"""Kernel-level measurement for narrowing inside the packed result arena.

Probe + pack-narrow (kernel time from device events inside the library, and
the host's time for the call) against ``csp_pack_checksum_dev`` on the same
wide segments, the probe with nontemporal against plain loads (pack-narrow
timed after each), and the loopback round trip with the option on and off.  The
variants alternate within one process; one warm round, then ``--reps``
repetitions; median with the lowest and highest value.  Workloads: a
bf16-valued float32 state dict of 159 tensors and a dict of int64 ids that
take int16.  Prints markdown rows for profiles/packed_narrowed_results.md.

    python tools/packed_narrow_results_bench.py [--reps 7]
"""

import argparse
import asyncio
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402
from covalent_ssh_plugin_amd.gpu import probe  # noqa: E402


def workloads():
    gen = torch.Generator().manual_seed(11)
    shapes = [(64, 3, 7, 7)] + [(c, c, 3, 3) for c in (64, 128, 256) for _ in range(12)]
    shapes += [(c,) for c in (64, 128, 256, 512) for _ in range(30)] + [(1000, 512), (1000,)]
    state = [torch.randn(*s, generator=gen).bfloat16().float().cuda() for s in shapes[:159]]
    ids = [torch.randint(-30000, 30000, (n,), generator=gen).cuda()
           for n in (4096, 30000, 65536, 1000, 250000) * 8]
    return {"float32 state dict from bf16": (state, "float32", "bfloat16"),
            "int64 ids that take int16": (ids, "int64", "int16")}


def timed(fn):
    t0 = time.perf_counter()
    report = fn()
    return (time.perf_counter() - t0) * 1e3, report["kernel_ms"]


def fmt(values):
    return "%.4g (%.4g to %.4g)" % (statistics.median(values), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    reps = ap.parse_args().reps
    for name, (tensors, src, dst) in workloads().items():
        wide = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]
        offs_w, total_w = probe.pack_layout([n for _, n in wide])
        rows = [(t.data_ptr(), t.numel(), src, dst) for t in tensors]
        offs_n, total_n = probe.pack_narrow_layout(rows)
        arena = torch.empty(total_w, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def probed(nt):
            probe.pack_narrow_probe_nt(nt)
            return probe.pack_narrow_probe_device([r[:3] for r in rows])

        def pack_narrow():
            return probe.pack_narrow_checksum_device(
                [r + (o,) for r, o in zip(rows, offs_n)], arena.data_ptr(), total_n)

        # pack-narrow is timed right after each probe variant: what plain loads
        # are for is the second kernel finding the lines in the cache
        variants = {
            "wide pack": lambda: probe.pack_checksum_device(
                [(p, o, n) for (p, n), o in zip(wide, offs_w)], arena.data_ptr(), total_w),
            "probe plain": lambda: probed(0),
            "pack-narrow after plain": pack_narrow,
            "probe nontemporal": lambda: probed(1),
            "pack-narrow after nontemporal": pack_narrow,
        }
        call = {k: [] for k in variants}
        kern = {k: [] for k in variants}
        for rep in range(reps + 1):
            for key, fn in variants.items():
                c, k = timed(fn)
                if rep:  # the first round warms
                    call[key].append(c)
                    kern[key].append(k)
        probe.pack_narrow_probe_nt(-1)
        print("| %s: %d tensors, %d wide bytes, %d narrow bytes |" % (
            name, len(tensors), total_w, total_n))
        for key in variants:
            print("| %s | %s | %s |" % (key, fmt(kern[key]), fmt(call[key])))
        for how in ("plain", "nontemporal"):
            both = [a + b for a, b in zip(kern["probe " + how], kern["pack-narrow after " + how])]
            print("| probe %s + pack-narrow, kernels | %s | ratio to wide pack %.3g |" % (
                how, fmt(both), statistics.median(both) / statistics.median(kern["wide pack"])))
    round_trip(reps)


def electron(name):
    """The workload, built once per worker: the round trip times the return."""
    import builtins

    cache = builtins.__dict__.setdefault("_packed_narrow_bench", {})
    if name not in cache:
        cache[name] = workloads()[name][0]
    return cache[name]


def round_trip(reps):
    """One electron returns each workload over the loopback transport, with
    narrow_tensor_results on and off (pack_tensor_results on in both), the two
    executors taking turns."""

    async def run(home):
        executors = {}
        for on in (True, False):
            Path(home, str(on)).mkdir()
            executors[on] = SSHExecutor(
                transport="local", local_home="%s/%s" % (home, on), cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, pack_tensor_results=True,
                pinned_staging_threshold_bytes=8 << 20, narrow_tensor_results=on,
                hip_visible_devices_policy="fixed", fixed_gpu=0)
        print("| result | narrow_tensor_results | round trip ms | frame bytes | narrow_ms |")
        for name in workloads_names():
            times, meta = {True: [], False: []}, {}
            for rep in range(reps + 1):  # the first round starts and warms the workers
                for on, ex in executors.items():
                    t0 = time.perf_counter()
                    value = await ex.execute(electron, [name], {}, dispatch_id="b", node_id=rep)
                    if rep:
                        times[on].append((time.perf_counter() - t0) * 1e3)
                    meta[on] = ex.last_task_record.remote_meta
                    del value
            for on in (True, False):
                print("| %s | %s | %s | %d | %s |" % (
                    name, "on" if on else "off", fmt(times[on]),
                    meta[on]["buffers"][0]["nbytes"], meta[on]["staging"].get("narrow_ms", "")))
        await SSHExecutor.close_pool()

    with tempfile.TemporaryDirectory() as home:
        asyncio.run(run(home))


def workloads_names():
    return ("float32 state dict from bf16", "int64 ids that take int16")


if __name__ == "__main__":
    main()
