"""Measurements for bool tensors sent as ``"bits"`` on one MI355X; writes the
tables of ``profiles/bool_bits.md`` (``--out``).

Kernel table at ``--mib`` of bool: csp_bool_pack_checksum_dev's kernel alone
(device events inside the library), its probe, and csp_bool_unpack_checksum_dev
with one destination and with two, each against the copy floor for the bytes it
reads plus writes at the rate the probe's HBM sweep reaches here, and against
what is done for the same tensor without them: on the result side
csp_pack_checksum_dev of the wide bytes, on the argument side the wide H2D copy
from pinned memory followed by csp_copy_checksum_dev, against the H2D copy of
the bits followed by the unpack kernel (host time with synchronisation).

Round-trip table: one electron returning ``--mib`` of bool and one taking as
much, over the loopback transport with ``narrow_tensor_results`` /
``narrow_tensor_args`` on and off, the two executors taking turns in one
process.  With the option off a bool tensor travels as it did before the
kernels existed.
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


def fmt(values):
    return "%.4g (%.4g to %.4g)" % (statistics.median(values), min(values), max(values))


def spread(values):
    return max(values) - min(values)


def beats(new, old):
    gain = statistics.median(old) - statistics.median(new)
    return "yes" if gain > spread(new) + spread(old) else "NO"


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
    numel = mib << 20
    total = probe.bool_bits_bytes(numel)
    rate, sweep = copy_rate(numel, reps)
    out.append("Sweep copy of %d MiB: %s ms, %.0f GB/s read plus write.\n" % (
        mib, fmt(sweep), rate / 1e6))
    gen = torch.Generator(device="cuda").manual_seed(5)
    mask = torch.rand(numel, device="cuda", generator=gen) > 0.5
    bits = torch.empty(total, dtype=torch.uint8, device="cuda")
    wide = torch.empty(numel, dtype=torch.uint8, device="cuda")
    wide2 = torch.empty(numel, dtype=torch.uint8, device="cuda")
    host_wide = torch.empty(numel, dtype=torch.uint8).pin_memory()
    host_wide.copy_(mask.view(torch.uint8))
    host_bits = torch.empty(total, dtype=torch.uint8).pin_memory()
    rows = {k: [] for k in ("pack", "probe", "pack_wide", "unpack1", "unpack2", "arg_bits",
                            "arg_wide")}
    for rep in range(reps + 1):  # the first round warms
        torch.cuda.synchronize()
        packed = probe.bool_pack_checksum_device(mask.data_ptr(), numel, bits.data_ptr(), total)
        assert packed["bad"] == 0, packed
        probed = probe.bool_pack_checksum_device(mask.data_ptr(), numel)
        whole = probe.pack_checksum_device([(mask.data_ptr(), 0, numel)], wide.data_ptr(), numel)
        one = probe.bool_unpack_checksum_device(bits.data_ptr(), numel, wide.data_ptr())
        two = probe.bool_unpack_checksum_device(
            bits.data_ptr(), numel, wide.data_ptr(), wide2.data_ptr())
        assert one["sum"] == two["sum"] == tuple(whole["sum"]), (one, two, whole)
        assert torch.equal(wide2, mask.view(torch.uint8))
        host_bits.copy_(bits)
        torch.cuda.synchronize()
        t0 = time.perf_counter()  # the argument as bits: H2D of an eighth, one launch
        bits.copy_(host_bits, non_blocking=True)
        torch.cuda.synchronize()
        probe.bool_unpack_checksum_device(bits.data_ptr(), numel, wide.data_ptr(), wide2.data_ptr())
        t1 = time.perf_counter()  # the argument whole: H2D of all of it, the checksummed copy
        wide.copy_(host_wide, non_blocking=True)
        torch.cuda.synchronize()
        probe.copy_checksum_device(wide2.data_ptr(), wide.data_ptr(), numel)
        t2 = time.perf_counter()
        if rep:
            rows["pack"].append(packed["kernel_ms"])
            rows["probe"].append(probed["kernel_ms"])
            rows["pack_wide"].append(whole["kernel_ms"])
            rows["unpack1"].append(one["kernel_ms"])
            rows["unpack2"].append(two["kernel_ms"])
            rows["arg_bits"].append((t1 - t0) * 1e3)
            rows["arg_wide"].append((t2 - t1) * 1e3)
    out.append("| kernel | ms | bytes read + written | copy floor ms | kernel / floor |")
    out.append("|---|---|---|---|---|")
    for name, key, moved in (
        ("bool pack", "pack", numel + total), ("bool pack, probe", "probe", numel),
        ("bool unpack, one destination", "unpack1", total + numel),
        ("bool unpack, two destinations", "unpack2", total + 2 * numel),
        ("csp_pack_checksum_dev of the wide bytes", "pack_wide", 2 * numel),
    ):
        floor = moved / rate
        out.append("| %s | %s | %d | %.4g | %.3g |" % (
            name, fmt(rows[key]), moved, floor, statistics.median(rows[key]) / floor))
    out.append("")
    out.append("| same tensor, two ways | new ms | without the kernels ms | below by more than "
               "the spreads |")
    out.append("|---|---|---|---|")
    out.append("| result: bool pack against csp_pack_checksum_dev of the wide bytes (kernels) "
               "| %s | %s | %s |" % (fmt(rows["pack"]), fmt(rows["pack_wide"]),
                                     beats(rows["pack"], rows["pack_wide"])))
    out.append("| argument: H2D of the bits + unpack into two against wide H2D + "
               "csp_copy_checksum_dev (host time) | %s | %s | %s |" % (
                   fmt(rows["arg_bits"]), fmt(rows["arg_wide"]),
                   beats(rows["arg_bits"], rows["arg_wide"])))


def produce(numel):
    import torch

    return torch.rand(numel, device="cuda") > 0.5


def consume(t):
    return [t.is_cuda, str(t.dtype), int(t.numel())]


def measure_round_trip(mib, reps, out):
    numel = mib << 20

    async def run(home):
        for on in (True, False):
            Path(home, str(on)).mkdir()
        executors = {
            on: SSHExecutor(
                transport="local", local_home="%s/%s" % (home, on), cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
                narrow_tensor_results=on, narrow_tensor_args=on,
                hip_visible_devices_policy="fixed", fixed_gpu=0)
            for on in (True, False)
        }
        times = {(side, on): [] for side in ("result", "argument") for on in (True, False)}
        frame = {}
        for rep in range(reps + 1):  # the first round starts and warms the workers
            arg = torch.rand(numel, generator=torch.Generator().manual_seed(rep)) > 0.5
            for on, ex in executors.items():
                t0 = time.perf_counter()
                value = await ex.execute(produce, [numel], {}, dispatch_id="b", node_id=2 * rep)
                t1 = time.perf_counter()
                staging = ex.last_task_record.remote_meta["staging"]
                frame["result", on] = numel - staging.get("narrow_saved_bytes", 0)
                assert value.dtype == torch.bool and value.numel() == numel
                del value
                t2 = time.perf_counter()
                seen = await ex.execute(consume, [arg], {}, dispatch_id="b", node_id=2 * rep + 1)
                t3 = time.perf_counter()
                stage = ex.last_task_record.remote_meta["arg_staging"]
                frame["argument", on] = stage.get("wire_bytes", stage["bytes"])
                assert seen == [True, "torch.bool", numel], seen
                if rep:
                    times["result", on].append((t1 - t0) * 1e3)
                    times["argument", on].append((t3 - t2) * 1e3)
        await SSHExecutor.close_pool()
        out.append("| %d MiB bool | option | round trip ms | frame bytes | on beats off by more "
                   "than the spreads |" % mib)
        out.append("|---|---|---|---|---|")
        for side in ("result", "argument"):
            for on in (True, False):
                out.append("| %s | %s | %s | %d | %s |" % (
                    side, "on" if on else "off", fmt(times[side, on]), frame[side, on],
                    beats(times[side, True], times[side, False]) if on else ""))

    with tempfile.TemporaryDirectory() as home:
        asyncio.run(run(home))


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--mib", type=int, default=256)
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--out", default="profiles/bool_bits.md")
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
