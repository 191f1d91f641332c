"""``gather_tensor_results``: an electron returns a transposed CUDA tensor and
the worker lays it out with one checksummed gather kernel, where torch's
``contiguous()`` costs a second allocation and a second pass.

    python examples/strided_results.py            # one round trip, with the stats
    python examples/strided_results.py --measure  # the tables of profiles/strided_results.md
    python examples/strided_results.py --measure-short-inner [--parent-lib libcsp_gpu.so]
                                                  # those of profiles/short_inner_results.md

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  ``--measure`` times
``csp_gather_checksum_dev`` against ``contiguous()`` followed by
``csp_pack_checksum_dev`` (the path before the option) on six layouts, and the
round trip of a 256 MiB transposed result with the option on against off: one
warm call first, then 5 alternating repetitions, medians with all values.
``--measure-short-inner`` times the slab path (tools' force value 2) on a ``(512, 512, 3, 3)``
``channels_last`` weight in bf16 and float32 against the host's choice, the direct path,
against ``csp_copy_checksum_dev`` on the same byte count and, with
``--parent-lib``, against another build of the library on the same input.
"""

import argparse
import asyncio
import importlib.util
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from covalent_ssh_plugin_amd import SSHExecutor  # noqa: E402
from covalent_ssh_plugin_amd.gpu import probe  # noqa: E402

REPS = 5

SHAPES = {
    "(8192, 8192) f32 .t()": lambda: torch.randn(8192, 8192, device="cuda").t(),
    "(4096, 16384) bf16 .t()": lambda: torch.randn(
        4096, 16384, device="cuda", dtype=torch.bfloat16).t(),
    "(16384, 16384) u8 .t()": lambda: torch.randint(
        0, 256, (16384, 16384), device="cuda", dtype=torch.uint8).t(),
    "(8, 32, 2048, 128) bf16 .permute(0, 2, 1, 3)": lambda: torch.randn(
        8, 32, 2048, 128, device="cuda", dtype=torch.bfloat16).permute(0, 2, 1, 3),
    "(8192, 8192) f32 [:, :4096]": lambda: torch.randn(8192, 8192, device="cuda")[:, :4096],
    "(64, 256, 56, 56) bf16 channels_last": lambda: torch.randn(
        64, 256, 56, 56, device="cuda", dtype=torch.bfloat16
    ).contiguous(memory_format=torch.channels_last),
}


# 3 x 3 weights: after collapsing (512, 512, 9) with strides (4608, 1, 512)
SHORT_INNER = {
    "(512, 512, 3, 3) bf16 channels_last": torch.bfloat16,
    "(512, 512, 3, 3) f32 channels_last": torch.float32,
}
CALLS = 20  # a value of the short-inner table is the mean of this many calls


def transposed(n):
    """The electron: an ``n x n`` float32 matrix, returned transposed."""
    import torch

    return torch.randn(n, n, device="cuda").t()


def peak_reserved():
    import torch

    return torch.cuda.max_memory_reserved()


def make_executor(home, gather):
    return SSHExecutor(
        transport="local",
        local_home=home,
        cache_dir=home + "/cache",
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=True,
        arg_cache_bytes=8 << 30,
        retain_tensor_results=True,
        gather_tensor_results=gather,
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )


def fmt(values):
    return "%.4g (%s)" % (statistics.median(values), " ".join("%.4g" % v for v in values))


def gather(t, master, nbytes):
    torch.cuda.synchronize()
    return probe.gather_checksum_device(
        t.data_ptr(), t.element_size(), list(t.shape), list(t.stride()), master.data_ptr(), nbytes)


def parent(t, master, nbytes):
    """What the worker does without the option."""
    flat = t.contiguous()
    torch.cuda.synchronize()
    return probe.pack_checksum_device([(flat.data_ptr(), 0, nbytes)], master.data_ptr(), nbytes)


def copy_rate(nbytes=256 << 20):
    """Bytes per ms (read plus write) of the probe's sweep kernel."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    times = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        probe.hbm_sweep_device(-1, src.data_ptr(), dst.data_ptr(), nbytes // 16)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    print("sweep copy of %d bytes: %s ms" % (nbytes, fmt(times)))
    return 2 * nbytes / statistics.median(times)


def measure_kernel():
    """Host time of the calls as the worker sees them, synchronisation
    included, alternating; and the gather kernel alone."""
    rate = copy_rate()
    print("| layout | bytes | path | gather ms | parent ms | parent spread | gather kernel ms "
          "| floor gather / parent ms | direct forced ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for label, make in SHAPES.items():
        t = make()
        nbytes = t.numel() * t.element_size()
        master = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        rows = {"gather": [], "parent": [], "kernel": [], "direct": []}
        for rep in range(REPS + 1):  # the first round warms
            t0 = time.perf_counter()
            report = gather(t, master, nbytes)
            t1 = time.perf_counter()
            sums = parent(t, master, nbytes)["sum"]
            t2 = time.perf_counter()
            assert report["sums"] == sums, (label, report, sums)
            forced = None
            if report["path"] in ("transpose", "slab"):
                probe.gather_checksum_path(1)
                t3 = time.perf_counter()
                forced = gather(t, master, nbytes)
                t4 = time.perf_counter()
                probe.gather_checksum_path(0)
                assert forced["sums"] == sums and forced["path"] == "direct"
            if rep:
                rows["gather"].append((t1 - t0) * 1e3)
                rows["parent"].append((t2 - t1) * 1e3)
                rows["kernel"].append(report["kernel_ms"])
                if forced:
                    rows["direct"].append((t4 - t3) * 1e3)
        print("| %s | %d | %s | %s | %s | %.4g | %s | %.4g / %.4g | %s |" % (
            label, nbytes, report["path"], fmt(rows["gather"]), fmt(rows["parent"]),
            max(rows["parent"]) - min(rows["parent"]), fmt(rows["kernel"]),
            2 * nbytes / rate, 4 * nbytes / rate,
            fmt(rows["direct"]) if rows["direct"] else ""))
        del t, master
        torch.cuda.empty_cache()


def measure_short_inner(parent_lib=""):
    """The slab path (force value 2) against the host's choice (direct), the copy with
    checksum of as many bytes, and optionally the library at ``parent_lib``:
    host time per call and the kernel alone, alternating within one process."""
    variants = {"slab forced": (probe, 2), "host's choice": (probe, 0)}
    if parent_lib:  # a second copy of the bindings, bound to the other build
        spec = importlib.util.spec_from_file_location("probe_parent", probe.__file__)
        other = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(other)
        other.load(parent_lib)
        variants["parent"] = (other, 0)
    print("| layout | bytes | variant | path | call ms | kernel ms | call / copy | spread of call |")
    print("|---|---|---|---|---|---|---|---|")
    for label, dtype in SHORT_INNER.items():
        t = torch.randn(512, 512, 3, 3, device="cuda").to(dtype).contiguous(
            memory_format=torch.channels_last)
        nbytes = t.numel() * t.element_size()
        flat = t.contiguous().view(torch.uint8)
        master = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rows = {name: ([], []) for name in variants}
        copies, paths, sums = [], {}, set()
        for rep in range(REPS + 1):  # the first round warms
            for name, (lib, force) in variants.items():
                lib.gather_checksum_path(force)
                kernel = 0.0
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    report = lib.gather_checksum_device(
                        t.data_ptr(), t.element_size(), list(t.shape), list(t.stride()),
                        master.data_ptr(), nbytes)
                    kernel += report["kernel_ms"]
                call = (time.perf_counter() - t0) * 1e3 / CALLS
                lib.gather_checksum_path(0)
                paths[name] = report["path"]
                sums.add(report["sums"])
                if rep:
                    rows[name][0].append(call)
                    rows[name][1].append(kernel / CALLS)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                sums.add(probe.copy_checksum_device(master.data_ptr(), flat.data_ptr(), nbytes))
            if rep:
                copies.append((time.perf_counter() - t0) * 1e3 / CALLS)
        assert len(sums) == 1, (label, sums)
        assert torch.equal(master, flat.reshape(-1))
        floor = statistics.median(copies)
        print("| %s | %d | copy with checksum | | %s | | 1 | %.4g |" % (
            label, nbytes, fmt(copies), max(copies) - min(copies)))
        for name, (calls, kernels) in rows.items():
            print("| %s | %d | %s | %s | %s | %s | %.3g | %.4g |" % (
                label, nbytes, name, paths[name], fmt(calls), fmt(kernels),
                statistics.median(calls) / floor, max(calls) - min(calls)))


async def measure_round_trip(n=8192):
    """One 256 MiB transposed float32 result with retain_tensor_results,
    option on against off, each with its own warm worker."""
    print("| variant | round trip ms | gathered | worker peak reserved MiB |")
    print("|---|---|---|---|")
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        variants = {"on": make_executor(a, True), "off": make_executor(b, False)}
        times = {"on": [], "off": []}
        last = {}
        node = 0
        for rep in range(REPS + 1):  # the first round warms
            for name, ex in variants.items():
                node += 1
                t0 = time.perf_counter()
                out = await ex.execute(transposed, [n], {}, dispatch_id="rt", node_id=node)
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
                last[name] = ex.last_task_record.remote_meta["staging"]
                assert out.shape == (n, n)
                del out
        for name, ex in variants.items():
            node += 1
            peak = await ex.execute(peak_reserved, [], {}, dispatch_id="rt", node_id=node)
            print("| %s | %s | %s | %.0f |" % (
                name, fmt(times[name]), last[name].get("gathered_tensors", 0), peak / 2**20))
        for ex in variants.values():
            await ex.close_pool()


async def hbm_footprint(n=8192):
    """Device-wide HBM in use (csp_mem_info) after ONE such result, a fresh
    worker per variant, one after the other."""
    for name, on in (("on", True), ("off", False)):
        with tempfile.TemporaryDirectory() as home:
            ex = make_executor(home, on)
            await ex.execute(peak_reserved, [], {}, dispatch_id="m", node_id=1)  # worker up
            before = probe.mem_info(0)["hbm_free_gb"]
            out = await ex.execute(transposed, [n], {}, dispatch_id="m", node_id=2)
            after = probe.mem_info(0)["hbm_free_gb"]
            del out
            await ex.close_pool()
        print("HBM taken by one result, option %s: %.3f GB" % (name, before - after))


async def demo():
    with tempfile.TemporaryDirectory() as home:
        ex = make_executor(home, True)
        out = await ex.execute(transposed, [2048], {}, dispatch_id="demo", node_id=1)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
    print("result:", tuple(out.shape), out.dtype, "contiguous:", out.is_contiguous())
    print("buffer:", meta["buffers"][0])
    print("staging:", {k: v for k, v in meta["staging"].items() if k.startswith("gather")})


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--measure-short-inner", action="store_true")
    parser.add_argument("--parent-lib", default="", help="another build of libcsp_gpu.so")
    opts = parser.parse_args()
    if opts.measure_short_inner:
        measure_short_inner(opts.parent_lib)
    elif opts.measure:
        measure_kernel()
        measure_short_inner(opts.parent_lib)
        asyncio.run(measure_round_trip())
        asyncio.run(hbm_footprint())
    else:
        asyncio.run(demo())
