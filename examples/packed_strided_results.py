"""``gather_tensor_results`` inside the packed result arena: an electron
returns a ``channels_last`` state dict and the worker fills the arena from
contiguous and non-contiguous tensors with one checksummed kernel launch,
where torch's ``contiguous()`` costs a launch, an allocation and a second pass
per non-contiguous tensor.

    python examples/packed_strided_results.py            # one round trip, with the stats
    python examples/packed_strided_results.py --measure  # profiles/packed_strided_results.md

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  ``--measure`` times
``csp_pack_gather_checksum_dev`` against ``contiguous()`` per tensor followed
by ``csp_pack_checksum_dev`` (the path before it) and against the same call
with the slab path allowed (the tools' force value 2) on five fixed workloads: one warm round first,
then 5 alternating repetitions, medians with all values.  ``--parent-lib``
adds the same call through another build of the library.
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

# (out channels, in channels, kernel height, kernel width) of a ResNet-50-like
# stack: the stem, then per stage a 1x1 reduce, a 3x3 and a 1x1 expand, each
# repeated as often as the stage has blocks, and the downsample projections
CONVS = [(64, 3, 7, 7)] + [
    shape
    for width, blocks, cin in ((64, 3, 256), (128, 4, 512), (256, 6, 1024), (512, 3, 2048))
    for shape in [(width, cin, 1, 1), (width, width, 3, 3), (4 * width, width, 1, 1)] * blocks
] + [(256, 64, 1, 1), (512, 256, 1, 1), (1024, 512, 1, 1), (2048, 1024, 1, 1)]
LINEARS = [(4096, 1024), (1024, 4096), (3072, 1024), (1024, 1024)] * 6  # (out, in)


def channels_last_state_dict(dtype, device="cuda"):
    """Conv weights in channels_last with a contiguous bias and norm scale
    between them."""
    out = {}
    for k, shape in enumerate(CONVS):
        weight = torch.randn(*shape, device=device).to(dtype)
        out["conv%d.weight" % k] = weight.to(memory_format=torch.channels_last)
        out["conv%d.bias" % k] = torch.randn(shape[0], device=device).to(dtype)
        out["norm%d.weight" % k] = torch.randn(shape[0], device=device)
    return out


def conv3x3_state_dict(dtype, device="cuda"):
    """Only the 3 x 3 weights of the stack, in channels_last: every tensor has
    a 9-element inner dimension under the unit-stride one."""
    return {
        "conv%d.weight" % k: torch.randn(*shape, device=device).to(dtype).to(
            memory_format=torch.channels_last)
        for k, shape in enumerate(CONVS) if shape[2:] == (3, 3)
    }


def transposed_linears(device="cuda"):
    return {
        "fc%d.weight_t" % k: torch.randn(*shape, device=device).t()
        for k, shape in enumerate(LINEARS)
    }


WORKLOADS = {
    "channels_last state dict, bf16": lambda: channels_last_state_dict(torch.bfloat16),
    "channels_last state dict, f32": lambda: channels_last_state_dict(torch.float32),
    "3 x 3 channels_last weights only, bf16": lambda: conv3x3_state_dict(torch.bfloat16),
    "3 x 3 channels_last weights only, f32": lambda: conv3x3_state_dict(torch.float32),
    "transposed Linear weights, f32": transposed_linears,
}


def fmt(values):
    return "%.4g (%s)" % (statistics.median(values), " ".join("%.4g" % v for v in values))


def layout(tensors):
    sizes = [t.numel() * t.element_size() for t in tensors]
    offsets, total = probe.pack_layout(sizes)
    return sizes, offsets, total


def packed_gather(tensors, arena, lib=probe, force=0):
    """The new call: strided tensors stay as they are.  ``force`` 2 takes the
    slab path, which the host does not choose by itself, where its rule holds."""
    sizes, offsets, total = layout(tensors)
    segments = [
        (t.data_ptr(), off, n) if t.is_contiguous()
        else (t.data_ptr(), off, n, t.element_size(), list(t.shape), list(t.stride()))
        for t, off, n in zip(tensors, offsets, sizes)
    ]
    torch.cuda.synchronize()
    lib.pack_gather_checksum_path(force)
    try:
        return lib.pack_gather_checksum_device(segments, arena.data_ptr(), total)
    finally:
        lib.pack_gather_checksum_path(0)


def before(tensors, arena):
    """What the worker does without it: contiguous() per tensor, then the
    pack kernel with its checksum."""
    sizes, offsets, total = layout(tensors)
    flats = [t.contiguous() for t in tensors]
    torch.cuda.synchronize()
    segments = [(f.data_ptr(), off, n) for f, off, n in zip(flats, offsets, sizes)]
    return probe.pack_checksum_device(segments, arena.data_ptr(), total)


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


def measure(parent_lib=""):
    """Host time of the calls as the worker sees them, synchronisation
    included, alternating; and the new kernel alone."""
    rate = copy_rate()
    others = {"slab forced": (probe, 2)}
    if parent_lib:  # a second copy of the bindings, bound to the other build
        spec = importlib.util.spec_from_file_location("probe_parent", probe.__file__)
        other = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(other)
        other.load(parent_lib)
        others["parent library"] = (other, 0)
    print("| workload | tensors (strided) | arena bytes | strided bytes | paths | new ms "
          "| before ms | spread of before | new kernel ms | floor new / before ms | "
          + " | ".join("%s ms | %s kernel ms" % (name, name) for name in others) + " |")
    print("|---|---|---|---|---|---|---|---|---|---|" + "---|---|" * len(others))
    for label, make in WORKLOADS.items():
        tensors = list(make().values())
        sizes, _, total = layout(tensors)
        strided = sum(n for t, n in zip(tensors, sizes) if not t.is_contiguous())
        arena = torch.empty(total, dtype=torch.uint8, device="cuda")
        rows = {"new": [], "before": [], "kernel": []}
        rows.update({name: ([], []) for name in others})
        for rep in range(REPS + 1):  # the first round warms
            t0 = time.perf_counter()
            report = packed_gather(tensors, arena)
            t1 = time.perf_counter()
            sums = before(tensors, arena)["sum"]
            t2 = time.perf_counter()
            assert report["sums"] == sums, (label, report["sums"], sums)
            for name, (lib, force) in others.items():
                t3 = time.perf_counter()
                again = packed_gather(tensors, arena, lib, force)
                t4 = time.perf_counter()
                assert again["sums"] == sums, (label, name, again["sums"], sums)
                if rep:
                    rows[name][0].append((t4 - t3) * 1e3)
                    rows[name][1].append(again["kernel_ms"])
            if rep:
                rows["new"].append((t1 - t0) * 1e3)
                rows["before"].append((t2 - t1) * 1e3)
                rows["kernel"].append(report["kernel_ms"])
        paths = {p: report["paths"].count(p) for p in sorted(set(report["paths"]))}
        print("| %s | %d (%d) | %d | %d | %s | %s | %s | %.4g | %s | %.4g / %.4g | %s |" % (
            label, len(tensors), sum(not t.is_contiguous() for t in tensors), total, strided,
            " ".join("%s:%d" % kv for kv in paths.items()), fmt(rows["new"]),
            fmt(rows["before"]), max(rows["before"]) - min(rows["before"]), fmt(rows["kernel"]),
            2 * total / rate, 2 * (total + strided) / rate,
            " | ".join("%s | %s" % (fmt(rows[name][0]), fmt(rows[name][1])) for name in others)))
        del tensors, arena
        torch.cuda.empty_cache()


def small_state_dict():
    """The electron: a few conv weights in channels_last with their biases."""
    import torch

    out = {}
    for k, shape in enumerate([(64, 3, 7, 7), (64, 64, 3, 3), (256, 64, 1, 1)]):
        weight = torch.randn(*shape, device="cuda")
        out["conv%d.weight" % k] = weight.to(memory_format=torch.channels_last)
        out["conv%d.bias" % k] = torch.randn(shape[0], device="cuda")
    return out


async def demo():
    with tempfile.TemporaryDirectory() as home:
        ex = SSHExecutor(
            transport="local", local_home=home, cache_dir=home + "/cache",
            python_path=sys.executable, persistent_workers=True, pack_tensor_results=True,
            gather_tensor_results=True, hip_visible_devices_policy="fixed", fixed_gpu=0,
        )
        out = await ex.execute(small_state_dict, [], {}, dispatch_id="demo", node_id=1)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
    print("result:", {k: tuple(v.shape) for k, v in out.items()})
    print("staging:", {k: v for k, v in meta["staging"].items()
                       if k.startswith(("gather", "packed"))})


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--measure", action="store_true")
    parser.add_argument("--parent-lib", default="", help="another build of libcsp_gpu.so")
    opts = parser.parse_args()
    if opts.measure:
        measure(opts.parent_lib)
    else:
        asyncio.run(demo())
