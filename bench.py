#!/usr/bin/env python3
"""Flagship benchmark: electron dispatch throughput + p50 round-trip
latency through the MI355X-native SSH executor (BASELINE.json metric).

One "step" = one complete no-op electron round trip through the full
executor pipeline: cloudpickle staging, transport round trip to the
per-GPU-slot persistent worker (or a freshly spawned stub with
--config noop-stub), GPU slot pinning via CSP_GPU_SLOT ->
HIP_VISIBLE_DEVICES, result pickle return, cleanup.  With N ranks
(one per GPU, launched by torch.distributed.run), each rank drives its
own GPU slot concurrently; the whole-job metric is electrons/sec
aggregated over all ranks, timed over the max across ranks.

No sshd exists in the benchmark image, so the default measured transport
is the REAL OpenSSH transport driven through the PATH-shim ssh client
(tests/sshim/ssh): real client argv, env-export prefix, tar-on-stdin
staging and worker channels — only the network hop is faked (stated in
the "data" field).  ``--transport local`` measures the loopback
transport for comparison.  The reference publishes no numbers
(BASELINE.md): vs_baseline is null.

A plain run does only what the headline figure needs: set up, warm up,
time ``--steps`` steps, print one JSON line.  With ``--full`` and one
rank on a GPU box the main (noop) line also carries a "secondary" list:
short runs of the mm and staging configs (BASELINE.json configs 2 and 4)
so a single invocation observes GPU-work dispatch, not only no-ops.

On a GPU box a run loads the in-tree CDNA4 library in this process and
lets it count the devices (no GPU work): the workers' GPU path needs it,
and a run without it is an error, not a figure for a reduced pipeline.

``--dump-outputs DIR`` writes what the caller of the last timed step
received as ``DIR/<name>.npy`` (float32/float64, at most 64 MB in all; a
larger array is cut to a fixed seeded sample): ``result`` is the
electron's return value, ``worker_gpu`` and ``worker_served`` come from
the task record (see caller_view).  Electrons that draw
random inputs are seeded in that mode, so two builds can be compared
output for output.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W]
        [--config noop|noop-stub|mm|staging|fan|rccl]
        [--transport sshim|local] [--full [--no-secondary]]
        [--dump-outputs DIR]
(--no-secondary only matters with --full; without it there are no
secondary runs to skip.)
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import statistics
import sys
import tempfile
import time

REPO_ROOT = os.path.dirname(os.path.abspath(__file__))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

SSHIM_DIR = os.path.join(REPO_ROOT, "tests", "sshim")

# Env the fake-remote side needs on a ROCm box (the shim sanitizes the
# environment like sshd would; these are what a real MI355X node's login
# env would provide).
SSHIM_PASS_ENV = (
    "HSA_ENABLE_IPC_MODE_LEGACY,HIP_VISIBLE_DEVICES,ROCR_VISIBLE_DEVICES,"
    "CUDA_VISIBLE_DEVICES,LD_LIBRARY_PATH,PYTORCH_ROCM_ARCH,TMPDIR"
)


def build_electron(config: str, seed=None):
    """Electron bodies are defined inside a factory so cloudpickle
    serializes them by value.  ``seed`` (set with --dump-outputs) pins
    the inputs of electrons that draw random ones."""
    if config in ("noop", "noop-stub", "noop-isolated", "fan"):

        def noop():
            return 0

        return noop, [], {}

    if config == "mm":
        # BASELINE config 2: single torch.mm(4096x4096, bf16) on one MI355X
        def mm_electron(n=4096, seed=None):
            import torch

            if seed is not None:
                torch.manual_seed(seed)
            a = torch.randn(n, n, device="cuda", dtype=torch.bfloat16)
            b = torch.randn(n, n, device="cuda", dtype=torch.bfloat16)
            c = a @ b
            torch.cuda.synchronize()
            return float(c.float().mean().item())

        return mm_electron, [], ({} if seed is None else {"seed": seed})

    if config == "staging":
        # BASELINE config 4: 1 GB tensor return through pinned staging
        def staging_electron(nbytes=1 << 30):
            import torch

            t = torch.ones(nbytes // 2, device="cuda", dtype=torch.bfloat16)
            torch.cuda.synchronize()
            return t

        return staging_electron, [], {}

    if config == "rccl":
        from covalent_ssh_plugin_amd.parallel.rccl_smoke import (
            make_rccl_smoke_electron,
        )

        import torch

        world = torch.cuda.device_count() if torch.cuda.is_available() else 2
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        return (
            make_rccl_smoke_electron(),
            [],
            {"world_size": max(1, world), "backend": backend},
        )

    raise SystemExit(f"unknown --config {config}")


def default_steps(config: str) -> int:
    # long enough to amortize ~30 ms OS hiccups for the fast configs,
    # bounded wall time for the heavy ones
    return {"staging": 8, "rccl": 3, "fan": 64, "mm": 256,
            "noop-isolated": 512}.get(config, 2048)


def default_warmup(config: str) -> int:
    return {"staging": 2, "rccl": 1, "fan": 4, "mm": 16}.get(config, 64)


def setup_sshim(rank: int) -> dict:
    """Point PATH at the shim client and create the fake remote home.
    Returns executor kwargs for the shim-SSH transport."""
    home = tempfile.mkdtemp(prefix=f"sshim-home-r{rank}-")
    keyfile = os.path.join(home, ".bench-key")
    with open(keyfile, "w") as f:
        f.write("bench fake key\n")
    os.environ["PATH"] = SSHIM_DIR + os.pathsep + os.environ.get("PATH", "")
    os.environ["SSHIM_HOME"] = home
    os.environ["SSHIM_PASS_ENV"] = SSHIM_PASS_ENV
    return {
        "transport": "ssh",
        "hostname": f"bench-node-r{rank}.sshim",
        "username": "mi355x",
        "ssh_key_file": keyfile,
    }


async def bench_once(
    *,
    config: str,
    steps: int,
    warmup: int,
    fan: int,
    transport_kwargs: dict,
    cache_dir: str,
    rank: int,
    local_rank: int,
    has_cuda: bool,
    gpu_count: int,
    seed=None,
) -> dict:
    """Run one config through the executor; returns elapsed/latencies/
    warm-path phase means (warmup records excluded) and what the last
    step handed back to its caller."""
    from covalent_ssh_plugin_amd import SSHExecutor

    fn, fargs, fkwargs = build_electron(config, seed)
    last = {"result": None}
    ex = SSHExecutor(
        cache_dir=cache_dir,
        python_path=sys.executable,
        hip_visible_devices_policy=(
            ("roundrobin" if config == "fan" else "fixed") if has_cuda else "none"
        ),
        fixed_gpu=local_rank % max(1, gpu_count) if has_cuda else local_rank,
        gpu_slots=max(1, gpu_count) if has_cuda else 1,
        # dispatch-throughput metric: slot pinning yes, per-task clock
        # warm-up no (measured separately by --config mm)
        warmup_gpu=config in ("mm", "staging"),
        pinned_staging_threshold_bytes=1 << 20,
        # warm worker per GPU slot (the production dispatch path);
        # "noop-stub" measures the classic spawn-per-task stub;
        # "noop-isolated" measures fork-isolated dispatch (fresh child
        # process per electron off a warm zygote)
        persistent_workers=config != "noop-stub",
        isolate_tasks=config == "noop-isolated",
        # noop electrons don't need torch in the children; "none" makes
        # forks millisecond-cheap (preloading torch-ROCm costs ~250 ms
        # of address-space copying per fork on MI355X)
        isolate_preload="none" if config == "noop-isolated" else "",
        **transport_kwargs,
    )

    async def one_step() -> float:
        last["result"] = None  # drop the previous step's result first
        t0 = time.perf_counter()
        if config == "fan":
            # BASELINE config 3: a fan of no-op electrons spread
            # round-robin across the node's GPU slots
            last["result"] = await asyncio.gather(
                *[
                    ex.execute(fn, list(fargs), dict(fkwargs),
                               dispatch_id=f"bench{rank}", node_id=i)
                    for i in range(fan)
                ]
            )
        else:
            last["result"] = await ex.execute(
                fn, list(fargs), dict(fkwargs),
                dispatch_id=f"bench{rank}", node_id=0,
            )
        return time.perf_counter() - t0

    for _ in range(warmup):
        await one_step()
    # phase means must describe the WARM path only: warmup records carry
    # one-time worker spawn + GPU prologue costs
    n_warm_records = len(ex.task_records)

    t_start = time.perf_counter()
    lat = [await one_step() for _ in range(steps)]
    elapsed = time.perf_counter() - t_start
    from covalent_ssh_plugin_amd.utils.timing import summarize

    phase_means = summarize(ex.task_records[n_warm_records:]).get(
        "phase_mean_ms", {}
    )
    record = ex.last_task_record
    return {"elapsed": elapsed, "latencies": lat, "phases": phase_means,
            "last_result": last["result"],
            "last_meta": (record.remote_meta if record else None) or {}}


# .npy payload budget for --dump-outputs: under 64 MB with room for headers
DUMP_LIMIT_BYTES = 48 << 20
DUMP_SAMPLE_SEED = 0


def _named_leaves(value, name):
    """Flatten an electron's return value into (name, leaf) pairs, a leaf
    being a CPU tensor or a float64 ndarray: dicts and sequences that
    hold tensors recurse, numeric scalars/sequences become arrays;
    non-numeric leaves (strings, None) carry nothing to compare and are
    left out."""
    import numpy as np
    import torch

    if isinstance(value, torch.Tensor):
        yield name, value.detach().cpu()
    elif isinstance(value, dict):
        for k in sorted(value, key=str):
            yield from _named_leaves(value[k], f"{name}_{k}")
    elif isinstance(value, (list, tuple)) and any(
        isinstance(v, (torch.Tensor, dict, list, tuple)) for v in value
    ):
        for i, v in enumerate(value):
            yield from _named_leaves(v, f"{name}_{i}")
    elif isinstance(value, (bool, int, float, np.number, np.ndarray, list, tuple)):
        try:
            yield name, np.asarray(value, dtype=np.float64)
        except (TypeError, ValueError):
            pass


# Device properties the remote side's CDNA4 library probe reports with
# every task: fixed for a given GPU, unlike its measured bandwidth/TFLOPs.
WORKER_GPU_PROPS = ("cu_count", "max_clock_mhz", "lds_per_cu_kb", "wavefront_size")


def caller_view(result, remote_meta: dict) -> dict:
    """What the caller of the last timed step received, by output name:
    the electron's return value and, from the task record the executor
    keeps for it, the run-to-run stable part of the remote side's report
    — the device properties read by the CDNA4 library on the worker's
    pinned GPU and the number of electrons that worker had served (one
    warm worker serving every step gives warmup + steps).

    The two worker_* outputs are not numerics of the electron.  They say
    that the same remote path ran: ``worker_gpu`` that the worker's
    native probe saw the same device, ``worker_served`` that one warm
    worker took every electron.  A worker respawned mid-run (a transport
    event, e.g. a dropped channel) lowers ``worker_served``; read a
    difference there as that, not as a numerical change between builds."""
    gpu = remote_meta.get("gpu") or {}
    return {
        "result": result,
        "worker_gpu": [gpu[k] for k in WORKER_GPU_PROPS] if gpu else None,
        "worker_served": remote_meta.get("served"),
    }


def dump_outputs(out_dir: str, outputs: dict) -> list:
    """Write ``outputs`` (name -> value) as ``<name>.npy`` files in
    float32/float64, at most DUMP_LIMIT_BYTES in all.  A leaf over
    its share of the budget is cut to a fixed sample of its elements
    (seeded, distinct indices in ascending order, so the sample keeps
    the leaf's order)."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    leaves = [
        leaf for name in sorted(outputs)
        for leaf in _named_leaves(outputs[name], name)
    ]
    share = DUMP_LIMIT_BYTES // max(1, len(leaves))
    written = []
    for name, leaf in leaves:
        is_tensor = isinstance(leaf, torch.Tensor)
        wide = not is_tensor or leaf.dtype in (torch.float64, torch.int64)
        size = leaf.numel() if is_tensor else leaf.size
        keep = share // (8 if wide else 4)
        if size > keep:
            # one seeded pick from each of `keep` equal strata: distinct,
            # ascending, spread over the whole leaf, O(keep) to draw
            rng = np.random.default_rng(DUMP_SAMPLE_SEED)
            starts = np.arange(keep, dtype=np.int64) * size // keep
            idx = starts + rng.integers(0, size // keep, size=keep)
            leaf = leaf.reshape(-1)[torch.from_numpy(idx) if is_tensor else idx]
        if is_tensor:
            leaf = leaf.to(torch.float64 if wide else torch.float32).numpy()
        path = os.path.join(out_dir, f"{name}.npy")
        np.save(path, leaf)
        written.append(path)
    return written


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=None)
    parser.add_argument("--warmup", type=int, default=None)
    parser.add_argument("--config", default="noop")
    parser.add_argument(
        "--transport", choices=["sshim", "local"], default="sshim",
        help="sshim: real OpenSSH transport via the PATH-shim ssh client "
             "(default); local: loopback transport",
    )
    parser.add_argument("--full", action="store_true",
                        help="after the timed steps also run everything "
                             "beside the headline figure (the secondary "
                             "mm/staging GPU runs)")
    parser.add_argument("--no-secondary", action="store_true",
                        help="with --full: skip the secondary mm/staging GPU runs")
    parser.add_argument("--dump-outputs", default="", metavar="DIR",
                        help="write what the last timed step returned as "
                             "DIR/<name>.npy (rank 0)")
    parser.add_argument("--dump-latencies", default="",
                        help="write per-step latencies (seconds, one per line)")
    parser.add_argument("--fan", type=int, default=64,
                        help="concurrent electrons per step for --config fan")
    args = parser.parse_args()
    if args.steps is None:
        args.steps = default_steps(args.config)
    if args.warmup is None:
        args.warmup = default_warmup(args.config)
    if args.steps < 1 or args.warmup < 0:
        parser.error("--steps must be >= 1 and --warmup >= 0")

    import torch

    # dmabuf IPC is required for RCCL on this host driver generation
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    distributed = world_size > 1

    has_cuda = torch.cuda.is_available()
    gpu_count = torch.cuda.device_count() if has_cuda else 0
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # nccl needs one distinct device per rank; fall back to gloo when
        # ranks outnumber visible GPUs (degenerate test topologies)
        backend = "nccl" if has_cuda and world_size <= gpu_count else "gloo"
        dist.init_process_group(backend=backend)
        if has_cuda:
            # modulo: degenerate topologies (more ranks than GPUs, gloo
            # fallback) must not address nonexistent devices
            torch.cuda.set_device(local_rank % max(1, gpu_count))

    def require_gpu_library():
        """The workers' GPU prologue and pinned staging come from the
        in-tree CDNA4 library.  Without it the executor only logs a
        warning and dispatches all the same, so the figures would
        describe a pipeline with no native code in it.  With a GPU
        present, load the library in this process and let it count the
        devices (no kernels, no allocations); a missing or broken
        library raises GpuLibError instead of being measured around."""
        if has_cuda:
            from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

            if gpu_probe.device_count() < 1:
                raise SystemExit("CDNA4 library loaded but sees no GPU")

    def barrier_sync():
        if distributed:
            import torch.distributed as dist

            dist.barrier()
        if has_cuda:
            torch.cuda.synchronize()

    from covalent_ssh_plugin_amd import SSHExecutor

    if args.transport == "sshim":
        transport_kwargs = setup_sshim(rank)
        transport_note = (
            "shim-SSH transport (real OpenSSH transport via PATH-shim ssh "
            "client; no sshd in image)"
        )
    else:
        local_home = tempfile.mkdtemp(prefix=f"bench-home-r{rank}-")
        transport_kwargs = {"transport": "local", "local_home": local_home}
        transport_note = "loopback transport (no sshd in image)"
    cache_dir = tempfile.mkdtemp(prefix=f"bench-cache-r{rank}-")

    common = dict(
        transport_kwargs=transport_kwargs,
        cache_dir=cache_dir,
        rank=rank,
        local_rank=local_rank,
        has_cuda=has_cuda,
        gpu_count=gpu_count,
    )

    async def run_all() -> dict:
        out = {}
        # warmup (untimed), then the timed region, bracketed by
        # barrier+synchronize on both sides
        await bench_once(  # warmup pass against the shared pools
            config=args.config, steps=0, warmup=args.warmup, fan=args.fan,
            **common,
        )
        # checked here, where this process first touches the GPU anyway
        require_gpu_library()
        barrier_sync()
        timed = await bench_once(
            config=args.config, steps=args.steps, warmup=0, fan=args.fan,
            seed=0 if args.dump_outputs else None,
            **common,
        )
        barrier_sync()
        out["main"] = timed

        # secondary GPU configs: driver-observed mm + staging dispatch in
        # the same invocation (VERDICT r1 "Next round" #7); single-rank
        # GPU runs only, so the flagship timing above stays undisturbed.
        # Only with --full: a plain run stops at its headline figure.
        out["secondary"] = []
        if (
            args.full
            and args.config == "noop"
            and not args.no_secondary
            and not distributed
            and has_cuda
        ):
            for cfg in ("mm", "staging"):
                res = await bench_once(
                    config=cfg,
                    steps=default_steps(cfg),
                    warmup=default_warmup(cfg),
                    fan=args.fan,
                    **common,
                )
                n = default_steps(cfg)
                out["secondary"].append(
                    {
                        "config": cfg,
                        "electrons_per_sec": round(n / res["elapsed"], 3),
                        "p50_ms": round(
                            statistics.median(res["latencies"]) * 1000, 3
                        ),
                        "steps": n,
                        "phase_mean_ms": {
                            k: round(v, 3) for k, v in res["phases"].items()
                        },
                    }
                )
        await SSHExecutor.close_pool()
        return out

    # NOTE on the warmup split above: bench_once(steps=0, warmup=W) runs
    # the warmup electrons against the same pooled workers/transports the
    # timed bench_once then reuses (module-level pools persist across
    # executor instances by design), so the timed region sees steady state.
    out = asyncio.run(run_all())
    timed = out["main"]
    elapsed = timed["elapsed"]

    if distributed:
        import torch.distributed as dist

        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cuda" if has_cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    electrons_per_step = args.fan if args.config == "fan" else 1
    if args.dump_latencies and rank == 0:
        with open(args.dump_latencies, "w") as f:
            f.write("\n".join(f"{x:.9f}" for x in timed["latencies"]))
    if args.dump_outputs and rank == 0:
        dump_outputs(
            args.dump_outputs,
            caller_view(timed["last_result"], timed["last_meta"]),
        )

    total_electrons = args.steps * world_size * electrons_per_step
    eps = total_electrons / elapsed
    lat_sorted = sorted(timed["latencies"])
    p50_ms = statistics.median(lat_sorted) * 1000.0
    p99_ms = lat_sorted[min(len(lat_sorted) - 1, int(len(lat_sorted) * 0.99))] * 1000.0
    p999_ms = lat_sorted[min(len(lat_sorted) - 1, int(len(lat_sorted) * 0.999))] * 1000.0
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        line = {
            "metric": "electrons_per_sec",
            "value": round(eps, 3),
            "unit": "electrons/s",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.config in ("mm", "staging") else "n/a",
            "data": (
                f"synthetic electrons, {transport_note}, "
                + {
                    "noop-stub": "spawn-per-task stub dispatch",
                    "noop-isolated": "fork-isolated dispatch (fresh child per electron)",
                }.get(args.config, "persistent-worker dispatch")
            ),
            "p50_ms": round(p50_ms, 3),
            "p99_ms": round(p99_ms, 3),
            "p999_ms": round(p999_ms, 3),
            "phase_mean_ms": {k: round(v, 3) for k, v in timed.get("phases", {}).items()},
            "secondary": out.get("secondary", []),
            "config": {
                "model": f"{args.config}-electron-dispatch",
                "global_batch": world_size,
                "seq_len": 0,
                "parallelism": f"slots{world_size}",
            },
        }
        print(json.dumps(line))

    if distributed:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
