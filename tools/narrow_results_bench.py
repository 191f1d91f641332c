"""Measurements for ``narrow_tensor_results`` on one MI355X; writes the tables
of ``profiles/narrowed_results.md`` (``--out``).

Kernel table, per pair at ``--mib`` of source: csp_narrow_checksum_dev's kernel
alone (device events inside the library), against the copy floor for the same
bytes read plus written at the rate the probe's HBM sweep reaches here, and
against what torch offers, ``.to(target)`` followed by csp_checksum_dev (device
events around both), alternating after a warm-up.  Integers also get the probe.

Round-trip table: one electron returning ``--mib`` of bf16-exact float32, and
one returning as many bytes of int64 ids, over the loopback transport with the
option on and off, alternating in one process; and the dispatcher's widening
alone, on the host.
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
from covalent_ssh_plugin_amd.remote.workers import widen_result  # noqa: E402

PAIRS = [("float32", "bfloat16"), ("float64", "float32"), ("int64", "int32"),
         ("int64", "int16"), ("int64", "uint8"), ("int32", "int16"), ("int32", "uint8")]
LIMIT = {"int32": 1 << 31, "int16": 1 << 15, "uint8": 1 << 8}


def fmt(values):
    return "%.4g (%.4g to %.4g)" % (statistics.median(values), min(values), max(values))


def exact_source(src, dst, numel):
    """``numel`` elements of ``src`` on the GPU that are exact as ``dst``."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    if src.startswith("float"):
        t = torch.randn(numel, device="cuda", generator=gen, dtype=getattr(torch, dst))
        return t.to(getattr(torch, src))
    return torch.randint(0, LIMIT[dst], (numel,), device="cuda", generator=gen,
                         dtype=getattr(torch, src))


def copy_rate(nbytes, reps):
    """Bytes per ms, read plus write, of the probe's sweep kernel."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probe.hbm_sweep_device(-1, src.data_ptr(), dst.data_ptr(), nbytes // 16)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return 2 * nbytes / statistics.median(times), times


def measure_kernel(mib, reps, out):
    nbytes = mib << 20
    rate, sweep = copy_rate(nbytes, reps)
    out.append("Sweep copy of %d MiB: %s ms, %.0f GB/s read plus write.\n" % (
        mib, fmt(sweep), rate / 1e6))
    out.append("| pair | narrow kernel ms | narrow call ms | copy floor ms | kernel / floor | "
               "torch .to + checksum ms | probe kernel ms |")
    out.append("|---|---|---|---|---|---|---|")
    for src, dst in PAIRS:
        numel = nbytes // probe.NARROW_ELEM_SIZE[src]
        t = exact_source(src, dst, numel)
        total = probe.narrow_bytes(numel, dst)
        flat = torch.empty(total, dtype=torch.uint8, device="cuda")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rows = {"narrow": [], "call": [], "torch": [], "probe": []}
        for rep in range(reps + 1):  # the first round warms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            report = probe.narrow_checksum_device(
                t.data_ptr(), numel, src, dst, flat.data_ptr(), total)
            call_ms = (time.perf_counter() - t0) * 1e3
            assert dst in report["fits"], (src, dst, report)
            start.record()
            narrow = t.to(getattr(torch, dst))
            torch.cuda.synchronize()
            sums = probe.checksum_device(narrow.data_ptr(), total)
            stop.record()
            torch.cuda.synchronize()
            assert sums == report["sum"], (src, dst, sums, report)
            probed = probe.narrow_checksum_device(t.data_ptr(), numel, src)
            if rep:
                rows["narrow"].append(report["kernel_ms"])
                rows["call"].append(call_ms)
                rows["torch"].append(start.elapsed_time(stop))
                rows["probe"].append(probed["kernel_ms"])
            del narrow
        floor = (nbytes + total) / rate
        out.append("| %s to %s | %s | %s | %.4g | %.3g | %s | %s |" % (
            src, dst, fmt(rows["narrow"]), fmt(rows["call"]), floor,
            statistics.median(rows["narrow"]) / floor,
            fmt(rows["torch"]), fmt(rows["probe"]) if src.startswith("int") else ""))
        del t, flat
        torch.cuda.empty_cache()


def electron(kind, numel):
    import torch

    if kind == "float32":
        return torch.randn(numel, device="cuda", dtype=torch.bfloat16).float()
    return torch.randint(0, 32_000, (numel,), device="cuda")


def measure_round_trip(mib, reps, out):
    async def run(home):
        for on in (True, False):
            Path(home, str(on)).mkdir()
        executors = {
            on: SSHExecutor(
                transport="local", local_home="%s/%s" % (home, on), cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
                narrow_tensor_results=on, hip_visible_devices_policy="fixed", fixed_gpu=0)
            for on in (True, False)
        }
        out.append("| result | option | round trip ms | frame bytes | worker narrow_ms |")
        out.append("|---|---|---|---|---|")
        for kind, size in (("float32", 4), ("int64", 8)):
            numel = (mib << 20) // size
            times = {True: [], False: []}
            meta = {}
            for rep in range(reps + 1):  # the first round starts and warms the workers
                for on, ex in executors.items():
                    t0 = time.perf_counter()
                    value = await ex.execute(electron, [kind, numel], {}, dispatch_id="b",
                                             node_id=rep)
                    if rep:
                        times[on].append((time.perf_counter() - t0) * 1e3)
                    meta[on] = ex.last_task_record.remote_meta
                    assert str(value.dtype) == "torch." + kind and value.numel() == numel
                    del value
            for on in (True, False):
                staging = meta[on]["staging"]
                frame = numel * size - staging.get("narrow_saved_bytes", 0)
                out.append("| %d MiB %s | %s | %s | %d | %s |" % (
                    mib, kind, "on" if on else "off", fmt(times[on]), frame,
                    staging.get("narrow_ms", "")))
        await SSHExecutor.close_pool()

    with tempfile.TemporaryDirectory() as home:
        asyncio.run(run(home))
    out.append("")
    out.append("| widening on the dispatcher (host, the event loop's thread) | ms |")
    out.append("|---|---|")
    for wire, dtype, size in (("bfloat16", "float32", 2), ("int16", "int64", 2)):
        numel = (mib << 20) // (4 if dtype == "float32" else 8)
        data = bytearray(numel * size)
        times = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            widen_result(data, {"wire": wire, "dtype": dtype, "shape": [numel]})
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        out.append("| %s to %s, %d elements | %s |" % (wire, dtype, numel, fmt(times)))


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--mib", type=int, default=256)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--out", default="profiles/narrowed_results.md")
    parser.add_argument("--skip-round-trip", action="store_true")
    args = parser.parse_args()
    out = []
    measure_kernel(args.mib, args.reps, out)
    out.append("")
    Path(args.out).write_text("\n".join(out) + "\n")
    if not args.skip_round_trip:
        measure_round_trip(args.mib, args.reps, out)
    text = "\n".join(out) + "\n"
    print(text)
    Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
