"""Measurements for ``narrow_tensor_args`` on one MI355X; writes the tables
of ``profiles/narrowed_args.md`` (``--out``).

Kernel table, per pair at ``--mib`` of WIDE bytes, with one destination and
with two (the cache's master and the electron's tensor): csp_widen_checksum_dev's
kernel alone (device events inside the library), against the copy floor for
the narrow bytes read plus the wide bytes written once or twice at the rate the
probe's HBM sweep reaches here, and against what can be done without the
kernel: ``narrow.to(wide)`` followed by csp_checksum_dev and, with two
destinations, csp_copy_checksum_dev (device events around all of it),
alternating after a warm-up.

Round-trip table: one electron taking ``--mib`` of int64 ids below 32 000, and
one taking as many bytes of bf16-exact float32, over the loopback transport
with the option on and off, the two executors taking turns in one process;
without the cache and, every tensor new, as a cache store.
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

PAIRS = [("bfloat16", "float32"), ("float32", "float64"), ("int32", "int64"),
         ("int16", "int64"), ("uint8", "int64"), ("int16", "int32"), ("uint8", "int32")]
LIMIT = {"int32": 1 << 31, "int16": 1 << 15, "uint8": 1 << 8}


def fmt(values):
    return "%.4g (%.4g to %.4g)" % (statistics.median(values), min(values), max(values))


def spread(values):
    return max(values) - min(values)


def narrow_source(narrow, numel):
    """``numel`` elements of ``narrow`` on the GPU in a buffer rounded up to 16 bytes."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    if narrow in LIMIT:
        t = torch.randint(0, LIMIT[narrow], (numel,), device="cuda", generator=gen,
                          dtype=getattr(torch, narrow))
    else:
        t = torch.randn(numel, device="cuda", generator=gen, dtype=getattr(torch, narrow))
    flat = torch.zeros(probe.narrow_bytes(numel, narrow), dtype=torch.uint8, device="cuda")
    flat[: t.numel() * t.element_size()] = t.view(torch.uint8)
    return flat, flat[: t.numel() * t.element_size()].view(getattr(torch, narrow))


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
    out.append("| pair | destinations | widen kernel ms | widen call ms | copy floor ms | "
               "kernel / floor | torch .to + checksum (+ copy) ms | below by more than the "
               "spreads |")
    out.append("|---|---|---|---|---|---|---|---|")
    for narrow, wide in PAIRS:
        numel = nbytes // probe.NARROW_ELEM_SIZE[wide]
        flat, typed = narrow_source(narrow, numel)
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst2 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for two in (False, True):
            rows = {"widen": [], "call": [], "torch": []}
            for rep in range(reps + 1):  # the first round warms
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                report = probe.widen_checksum_device(
                    flat.data_ptr(), numel, narrow, wide, dst.data_ptr(),
                    dst2.data_ptr() if two else 0)
                call_ms = (time.perf_counter() - t0) * 1e3
                start.record()
                widened = typed.to(getattr(torch, wide))
                torch.cuda.synchronize()  # the library's stream does not wait on torch's
                sums = probe.checksum_device(widened.data_ptr(), nbytes)
                if two:
                    sums = probe.copy_checksum_device(dst2.data_ptr(), widened.data_ptr(), nbytes)
                stop.record()
                torch.cuda.synchronize()
                assert tuple(sums) == report["sum"], (narrow, wide, sums, report)
                if rep:
                    rows["widen"].append(report["kernel_ms"])
                    rows["call"].append(call_ms)
                    rows["torch"].append(start.elapsed_time(stop))
                del widened
            floor = (flat.numel() + nbytes * (2 if two else 1)) / rate
            gain = statistics.median(rows["torch"]) - statistics.median(rows["widen"])
            out.append("| %s to %s | %d | %s | %s | %.4g | %.3g | %s | %s |" % (
                narrow, wide, 2 if two else 1, fmt(rows["widen"]), fmt(rows["call"]), floor,
                statistics.median(rows["widen"]) / floor, fmt(rows["torch"]),
                "yes" if gain > spread(rows["torch"]) + spread(rows["widen"]) else "NO"))
        del flat, typed, dst, dst2
        torch.cuda.empty_cache()


def electron(t):
    return [t.is_cuda, int(t.numel())]


def make_arg(kind, numel, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "float32":
        return torch.randn(numel, generator=gen, dtype=torch.bfloat16).float()
    return torch.randint(0, 32_000, (numel,), generator=gen)


def measure_round_trip(mib, reps, out):
    async def run(home, cached):
        for on in (True, False):
            Path(home, str(on)).mkdir()
        extra = dict(cache_tensor_args=True, arg_cache_bytes=4 * (mib << 20)) if cached else {}
        executors = {
            on: SSHExecutor(
                transport="local", local_home="%s/%s" % (home, on), cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
                narrow_tensor_args=on, hip_visible_devices_policy="fixed", fixed_gpu=0, **extra)
            for on in (True, False)
        }
        for kind, size in (("int64", 8), ("float32", 4)):
            numel = (mib << 20) // size
            times = {True: [], False: []}
            narrow_ms = {True: [], False: []}
            meta = {}
            for rep in range(reps + 1):  # the first round starts and warms the workers
                arg = make_arg(kind, numel, rep)  # new bytes every round: a store, never a hit
                for on, ex in executors.items():
                    before = ex.counters["arg_narrow_ms"]
                    t0 = time.perf_counter()
                    seen = await ex.execute(electron, [arg], {}, dispatch_id="b", node_id=rep)
                    if rep:
                        times[on].append((time.perf_counter() - t0) * 1e3)
                        narrow_ms[on].append(ex.counters["arg_narrow_ms"] - before)
                    meta[on] = ex.last_task_record.remote_meta
                    assert seen == [True, numel], seen
            for on in (True, False):
                stage = meta[on]["arg_staging"]
                out.append("| %d MiB %s | %s | %s | %s | %d | %s | %s |" % (
                    mib, kind, "store" if cached else "no cache", "on" if on else "off",
                    fmt(times[on]), stage.get("wire_bytes", stage["bytes"]),
                    fmt(narrow_ms[on]) if on else "", "%.4g" % stage["widen_ms"] if on else ""))
            gain = statistics.median(times[False]) - statistics.median(times[True])
            out.append("| | | on beats off by more than the spreads: %s | | | | |" % (
                "yes" if gain > spread(times[True]) + spread(times[False]) else "NO"))
        await SSHExecutor.close_pool()

    out.append("| argument | cache | option | round trip ms | frame bytes | dispatcher "
               "arg_narrow_ms | worker widen_ms |")
    out.append("|---|---|---|---|---|---|---|")
    for cached in (False, True):
        with tempfile.TemporaryDirectory() as home:
            asyncio.run(run(home, cached))


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--mib", type=int, default=256)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--out", default="profiles/narrowed_args.md")
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
