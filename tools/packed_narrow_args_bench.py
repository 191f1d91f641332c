"""Measurement for narrowing inside the packed argument arena.

Kernel level: ``csp_unpack_widen_checksum_dev`` on the narrow arena, without and
with a master, against ``csp_unpack_checksum_dev`` on the same tensors' wide
arena (the path without the option; that kernel is the parent commit's, line
for line).  Kernel time from device events inside the library, and the host's
time for the call.  Then the loopback round trip of one electron that takes
the workload as its argument, ``narrow_tensor_args`` on and off
(``pack_tensor_args`` on in both).  The variants alternate within one process;
one warm round, then ``--reps`` repetitions; median with the lowest and highest
value.  Workloads as in tools/packed_narrow_results_bench.py: a bf16-valued
float32 state dict of 159 tensors and a dict of int64 ids that take int16.
Prints markdown rows for profiles/packed_narrowed_args.md.

    python tools/packed_narrow_args_bench.py [--reps 7]
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
from covalent_ssh_plugin_amd.remote import workers  # noqa: E402

NAMES = ("float32 state dict from bf16", "int64 ids that take int16")


def workload(name):
    gen = torch.Generator().manual_seed(11)
    if name == NAMES[0]:
        shapes = [(64, 3, 7, 7)] + [(c, c, 3, 3) for c in (64, 128, 256) for _ in range(12)]
        shapes += [(c,) for c in (64, 128, 256, 512) for _ in range(30)] + [(1000, 512), (1000,)]
        return [torch.randn(*s, generator=gen).bfloat16().float() for s in shapes[:159]]
    return [torch.randint(-30000, 30000, (n,), generator=gen)
            for n in (4096, 30000, 65536, 1000, 250000) * 8]


def fmt(values):
    return "%.4g (%.4g to %.4g)" % (statistics.median(values), min(values), max(values))


def kernels(reps):
    for name in NAMES:
        tensors = workload(name)
        _, _, meta, bufs = workers.extract_arg_buffers(
            [tensors], {}, 8 << 20, to_device=True, pack_min_bytes=0)
        _, _, nmeta, nbufs = workers.extract_arg_buffers(
            [tensors], {}, 8 << 20, to_device=True, pack_min_bytes=0, narrow=True)
        info, ninfo = meta[0], nmeta[0]
        wide = torch.frombuffer(bytearray(bufs[0][0].tobytes()), dtype=torch.uint8).cuda()
        narrow = torch.frombuffer(bytearray(nbufs[0][0].tobytes()), dtype=torch.uint8).cuda()
        dsts = [torch.empty_like(t, device="cuda") for t in tensors]
        master = torch.empty(info["nbytes"], dtype=torch.uint8, device="cuda")
        rows = [(seg["nbytes"] // probe.NARROW_ELEM_SIZE[seg["dtype"]], seg["wire"], seg["dtype"])
                if seg.get("wire") else (seg["nbytes"], "", "") for seg in ninfo["packed"]]
        src_off, narrow_total, dst_off, wide_total = probe.unpack_widen_layout(rows)
        assert (narrow_total, wide_total) == (ninfo["wire_nbytes"], info["nbytes"])
        segs = [(d.data_ptr(), s, o) + r for d, s, o, r in zip(dsts, src_off, dst_off, rows)]
        plain = [(d.data_ptr(), seg["offset"], seg["nbytes"]) for d, seg in zip(dsts, info["packed"])]
        torch.cuda.synchronize()
        variants = {
            "wide unpack (`csp_unpack_checksum_dev`)": lambda: probe.unpack_checksum_device(
                wide.data_ptr(), wide_total, plain),
            "unpack-widen, tensors only": lambda: probe.unpack_widen_checksum_device(
                segs, narrow.data_ptr(), narrow_total, 0, wide_total),
            "unpack-widen, tensors and master": lambda: probe.unpack_widen_checksum_device(
                segs, narrow.data_ptr(), narrow_total, master.data_ptr(), wide_total),
        }
        call = {k: [] for k in variants}
        kern = {k: [] for k in variants}
        for rep in range(reps + 1):
            for key, fn in variants.items():
                t0 = time.perf_counter()
                report = fn()
                if rep:  # the first round warms
                    call[key].append((time.perf_counter() - t0) * 1e3)
                    kern[key].append(report["kernel_ms"])
                assert list(report["sum"]) == info["sum"], key
        assert torch.equal(master, wide) and all(
            torch.equal(d.cpu(), t) for d, t in zip(dsts, tensors))
        print("| %s: %d tensors, %d wide bytes, %d narrow bytes |" % (
            name, len(tensors), wide_total, narrow_total))
        for key in variants:
            print("| %s | %s | %s |" % (key, fmt(kern[key]), fmt(call[key])))


def electron(state):
    return [len(state), sum(t.numel() for t in state), all(t.is_cuda for t in state)]


def round_trip(reps):
    """One electron takes each workload over the loopback transport, with
    narrow_tensor_args on and off, the two executors taking turns."""

    async def run(home):
        executors = {}
        for on in (True, False):
            Path(home, str(on)).mkdir()
            executors[on] = SSHExecutor(
                transport="local", local_home="%s/%s" % (home, on), cache_dir=home + "/cache",
                python_path=sys.executable, persistent_workers=True, device_tensor_args=True,
                pack_tensor_args=True, pack_args_min_bytes=0,
                pinned_staging_threshold_bytes=8 << 20, narrow_tensor_args=on,
                hip_visible_devices_policy="fixed", fixed_gpu=0)
        print("| argument | narrow_tensor_args | round trip ms | frame bytes | dispatcher "
              "arg_narrow_ms per call | worker widen_ms |")
        for name in NAMES:
            state = workload(name)
            times, meta = {True: [], False: []}, {}
            before = executors[True].counters["arg_narrow_ms"]
            for rep in range(reps + 1):  # the first round starts and warms the workers
                for on, ex in executors.items():
                    t0 = time.perf_counter()
                    await ex.execute(electron, [state], {}, dispatch_id="b", node_id=rep)
                    if rep:
                        times[on].append((time.perf_counter() - t0) * 1e3)
                    meta[on] = ex.last_task_record.remote_meta["arg_staging"]
            spent = (executors[True].counters["arg_narrow_ms"] - before) / (reps + 1)
            for on in (True, False):
                print("| %s | %s | %s | %d | %s | %s |" % (
                    name, "on" if on else "off", fmt(times[on]),
                    meta[on].get("wire_bytes", meta[on]["bytes"]),
                    "%.3g" % spent if on else "", meta[on].get("widen_ms", "")))
        await SSHExecutor.close_pool()

    with tempfile.TemporaryDirectory() as home:
        asyncio.run(run(home))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    reps = ap.parse_args().reps
    kernels(reps)
    round_trip(reps)
