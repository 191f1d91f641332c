"""``delta_tensor_results``: an electron returns its cached argument with a
little of it changed, and only the changed 4 KiB blocks travel back.

    python examples/delta_results.py            # one round trip, with the stats
    python examples/delta_results.py --measure  # the tables of profiles/delta_results.md

Needs one MI355X and the built libraries (``python -m
covalent_ssh_plugin_amd.ops.build``).  ``--measure`` times the kernel against
``csp_checksum_dev`` on the same buffer, and the round trip of a 256 MiB
result with the option on against off (off is the behaviour before the option):
one warm call first, then 5 alternating repetitions, medians with all values.
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

REPS = 5


def step(state, rows):
    """The electron: ``rows`` rows of the state change, the rest is returned
    as it came."""
    state[:rows] += 1
    return state


def make_executor(home, delta):
    return SSHExecutor(
        transport="local",
        local_home=home,
        cache_dir=home + "/cache",
        python_path=sys.executable,
        persistent_workers=True,
        device_tensor_args=True,
        cache_tensor_args=True,
        arg_cache_bytes=8 << 30,
        delta_tensor_results=delta,
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
    )


def fmt(values):
    return "%.4g (%s)" % (statistics.median(values), " ".join("%.4g" % v for v in values))


def measure_kernel():
    """csp_diff_checksum_dev against csp_checksum_dev on the same ``cur``:
    host time of the bare calls, and the diff kernel alone."""
    block = probe.diff_block_bytes()
    print("| bytes | changed | diff call | checksum call | ratio | diff kernel |")
    print("|---|---|---|---|---|---|")
    for nbytes in (16 << 20, 64 << 20, 1 << 30):
        nblocks = nbytes // block
        base = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        for percent in (0, 1, 50):
            cur = base.clone()
            every = 100 // percent if percent else 0
            if every:
                cur.view(nblocks, block)[::every, 17] ^= 1
            delta = torch.empty((nblocks // 2 + 1) * (block + 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            args = (cur.data_ptr(), base.data_ptr(), nbytes, delta.data_ptr(), nblocks // 2 + 1)
            rows = {"diff": [], "sum": [], "kernel": []}
            for rep in range(REPS + 1):  # the first round warms
                t0 = time.perf_counter()
                report = probe.diff_checksum_device(*args)
                t1 = time.perf_counter()
                sums = probe.checksum_device(cur.data_ptr(), nbytes)
                t2 = time.perf_counter()
                assert report["rc"] == 0 and report["sum"] == sums
                assert report["changed"] == len(range(0, nblocks, every)) if every else True
                if rep:
                    rows["diff"].append((t1 - t0) * 1e3)
                    rows["sum"].append((t2 - t1) * 1e3)
                    rows["kernel"].append(report["kernel_ms"])
            print("| %d | %d %% | %s | %s | %.2f | %s |" % (
                nbytes, percent, fmt(rows["diff"]), fmt(rows["sum"]),
                statistics.median(rows["diff"]) / statistics.median(rows["sum"]),
                fmt(rows["kernel"])))


async def measure_round_trip(nbytes=256 << 20):
    """A result of ``nbytes`` with 1 % and with 100 % of its rows changed,
    option on against off, each with its own warm worker."""
    rows_total = nbytes // 4096
    state = torch.randn(rows_total, 1024)
    print("| changed | variant | round trip ms | on the wire | delta_ms |")
    print("|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        variants = {"on": make_executor(a, True), "off": make_executor(b, False)}
        for label, rows in (("1 %", rows_total // 100), ("100 %", rows_total)):
            times = {"on": [], "off": []}
            last = {}
            node = 0
            for rep in range(REPS + 1):  # the first round warms
                for name, ex in variants.items():
                    node += 1
                    t0 = time.perf_counter()
                    out = await ex.execute(step, [state, rows], {}, dispatch_id=label, node_id=node)
                    if rep:
                        times[name].append((time.perf_counter() - t0) * 1e3)
                    last[name] = ex.last_task_record.remote_meta["staging"]
                    assert out.shape == state.shape
            for name in variants:
                print("| %s | %s | %s | %s | %s |" % (
                    label, name, fmt(times[name]),
                    last[name].get("delta_bytes") or nbytes if name == "on" else nbytes,
                    last[name].get("delta_ms", "")))
        for ex in variants.values():
            await ex.close_pool()


async def demo():
    state = torch.randn(4096, 1024)  # 16 MiB
    with tempfile.TemporaryDirectory() as home:
        ex = make_executor(home, True)
        out = await ex.execute(step, [state, 3], {}, dispatch_id="demo", node_id=1)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
    want = state.clone()
    want[:3] += 1
    print("result equal:", torch.equal(out, want))
    print("delta meta:", meta["buffers"][0].get("delta"))
    print("staging:", {k: v for k, v in meta["staging"].items() if k.startswith("delta")})


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--measure", action="store_true")
    opts = parser.parse_args()
    if opts.measure:
        measure_kernel()
        asyncio.run(measure_round_trip())
    else:
        asyncio.run(demo())
