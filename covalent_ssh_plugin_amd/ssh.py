"""MI355X-native Covalent SSH executor.

Drop-in replacement for the reference SSHExecutor
(/root/reference/covalent_ssh_plugin/ssh.py) with the same public
constructor surface (reference ssh.py:75-92), the same config keys under
``[executors.ssh]`` (reference ssh.py:39-50), and the same on-disk
function/result pickle contract (reference ssh.py:147-150, exec.py:44-46)
— re-architected for a remote 8×MI355X node:

* **Pooled, multiplexed transport** — one OpenSSH ControlMaster per
  (host, user, key) shared by all tasks and executor instances, instead
  of one asyncssh connection per task (reference ssh.py:497, 585-587).
* **Fused single-round-trip dispatch** — staging (tar on stdin), remote
  execution, result + meta streaming and remote cleanup happen in ONE
  ssh command, vs ~10-11 sequential round trips per electron in the
  reference.
* **GPU slot scheduling** — each task acquires one of the node's MI355X
  GPUs and runs with ``HIP_VISIBLE_DEVICES`` pinned to it; slot tables
  are shared module-level state keyed by endpoint.
* **CDNA4 warm-up/device-probe kernel + hipHostMalloc-pinned staging**
  in the remote stub (see remote/stub_template.py and ops/hip/).
* Per-endpoint environment checks (python version, conda env, GPU lib
  provisioning) are hoisted out of the per-task path and cached.
* The reference's connection leak when the task raised (reference
  ssh.py:581-587) does not exist here: transports are pooled, never
  per-task, and slots release via try/finally.
"""

from __future__ import annotations

import asyncio
import functools
import os
import pickle as stdlib_pickle
import shlex
import time
import uuid
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Tuple

import cloudpickle

from .compat import RemoteExecutor, app_log, get_config, update_config_defaults
from .gpu import slots as gpu_slots
from .remote import workers as worker_pool
from .remote.stub import DEFAULT_STAGING_THRESHOLD, render_stub, render_worker
from .transport import (
    CompletedCommand,
    LocalTransport,
    OpenSSHTransport,
    Transport,
    TransportConnectError,
)
from .transport import pool as transport_pool
from .utils.timing import PhaseTimer, TaskRecord

EXECUTOR_PLUGIN_NAME = "SSHExecutor"

# Config defaults registered under [executors.ssh].  The first ten keys
# mirror the reference exactly (reference ssh.py:39-50); the rest are
# MI355X-native additions (SURVEY.md §5 "Config / flag system").
_EXECUTOR_PLUGIN_DEFAULTS = {
    "username": "",
    "hostname": "",
    "ssh_key_file": os.path.join(os.path.expanduser("~"), ".ssh", "id_rsa"),
    "cache_dir": os.path.join(
        os.environ.get("XDG_CACHE_HOME", os.path.join(os.path.expanduser("~"), ".cache")),
        "covalent",
    ),
    "python_path": "python",
    "conda_env": "",
    "remote_cache": ".cache/covalent",
    "run_local_on_ssh_fail": False,
    "remote_workdir": "covalent-workdir",
    "create_unique_workdir": False,
    # --- MI355X-native additions -------------------------------------
    "transport": "ssh",  # "ssh" (OpenSSH ControlMaster) | "local" (loopback)
    "ssh_port": 22,
    "gpu_slots": 8,  # GPUs on the remote node (8×MI355X)
    "slots_per_gpu": 1,  # 288 GB HBM3E/GPU: 1 electron per GPU by default
    # "roundrobin": each task ACQUIRES a slot (bounded concurrency, FIFO
    #   fair, spreads across GPUs).  "fixed": every task pins to
    #   `fixed_gpu` WITHOUT slot accounting — unbounded concurrency on
    #   that one GPU, intended for per-rank bench/embarrassing-parallel
    #   drivers that do their own admission control.  "none": no pinning.
    "hip_visible_devices_policy": "roundrobin",
    "warmup_gpu": True,  # run the CDNA4 warm-up/probe kernel pre-task
    "pinned_staging_threshold_bytes": DEFAULT_STAGING_THRESHOLD,
    "batch_roundtrips": True,  # fused single-round-trip dispatch
    "persistent_workers": False,  # warm worker process per GPU slot
    # Fork-isolated dispatch: persistent ZYGOTE worker (python + torch
    # imported, HIP untouched) forks a fresh child per electron —
    # spawn-per-task's fresh-process semantics (no state/HIP/module
    # leakage between electrons, crashes contained) at fork cost
    # (~ms) instead of a full interpreter + torch import start.
    # Implies worker-channel dispatch.
    "isolate_tasks": False,
    # Zygote preload for isolate mode: "torch" (children inherit a
    # loaded torch — saves multi-second imports for torch electrons, but
    # each fork copies the torch-ROCm address space, ~250 ms on MI355X)
    # or "none" (millisecond forks; torch electrons import themselves).
    "isolate_preload": "torch",
    # CPU torch tensors in an electron's args/kwargs arrive in the electron
    # as CUDA tensors on the worker's GPU: received straight into HBM
    # through a pinned ring (the copy overlaps the receive) and verified
    # there against a checksum computed here.  Needs persistent_workers or
    # isolate_tasks (the fused and stub paths keep arguments inside the
    # pickle file).  The run_local_on_ssh_fail fallback runs the function
    # with the original CPU tensors.
    "device_tensor_args": False,
    # The CUDA tensors of a result that are below
    # pinned_staging_threshold_bytes (a state_dict, a list of gradients)
    # are gathered on the GPU into one arena and sent as a single streamed
    # frame with a checksum that the dispatcher verifies, instead of one
    # pageable copy each inside the pickle.  They come back as views into
    # one shared buffer.  Needs persistent_workers or isolate_tasks.
    "pack_tensor_results": False,
    # Pack only when those tensors total at least this many bytes (below
    # it the reply is a single small frame anyway).
    "pack_results_min_bytes": 65536,
    # With device_tensor_args on persistent workers: a worker keeps the
    # tensor arguments it has received in HBM, keyed by a digest of their
    # bytes, and the dispatcher sends a repeated argument (the same weights
    # or dataset fanned out to many electrons) as that key alone.  Every
    # electron still gets a private CUDA tensor, copied from the cached
    # master and verified against a fresh checksum in one pass over HBM.
    # Not with isolate_tasks: the zygote may not touch HIP and its children
    # do not outlive a task.
    "cache_tensor_args": False,
    # Per-worker budget in bytes for the cached masters (8 GiB is under 3 %
    # of one MI355X's HBM); least recently used entries go first.
    "arg_cache_bytes": 8 << 30,
    # Tensors below this many bytes travel as without a cache.  16 MiB is
    # the smallest measured size at which every kind of hit beat the
    # dispatch without the cache (profiles/arg_cache.md): from 1 MiB a hit
    # on the same tensor object already does, but a hit on an equal tensor
    # that is another object pays the content hash again and does not.
    "arg_cache_min_bytes": 16 << 20,
    # With device_tensor_args: the CPU tensor arguments of one electron that
    # are below pinned_staging_threshold_bytes (and, with cache_tensor_args,
    # below arg_cache_min_bytes) travel as ONE frame that lands in HBM as one
    # arena; one kernel launch scatters it into private per-tensor
    # allocations and verifies its checksum in the same pass, instead of one
    # frame, one copy and one checksum launch per tensor.  With
    # cache_tensor_args an arena of at least arg_cache_min_bytes is cached
    # under one key.
    "pack_tensor_args": False,
    # Pack only when at least two tensors qualify and their arena is at
    # least this many bytes.  64 KiB is the smallest total measured
    # (16 x 4 KiB, profiles/packed_args.md): packing already halves the
    # dispatch there (0.89 against 1.76 ms), and no larger measured total
    # has it slower.  Below 64 KiB nothing was measured.
    "pack_args_min_bytes": 65536,
    # With cache_tensor_args and pack_tensor_args: a packed argument arena
    # with the layout of an arena that the worker already holds (a frozen
    # base plus a few adapter, optimizer or step tensors that change every
    # dispatch) travels as a delta of only the changed tensors.  The worker
    # patches the held arena in place, in the same kernel launch that
    # scatters and verifies it, and holds it under the new key.
    "patch_tensor_args": False,
    # Patch only when the changed tensors are at most this fraction of the
    # arena, else send it whole.  0.5 is a policy default, not a
    # measurement: a patch always sends fewer bytes than a store, but it
    # consumes the base, which a store would have left in the cache.
    "patch_args_max_fraction": 0.5,
    # With patch_tensor_args: a packed argument arena whose key the worker
    # does not hold is built on the worker as a NEW master from any held
    # arena plus a delta of the tensors that arena lacks, whatever the two
    # layouts (a tensor added, removed or resized), in the same kernel launch
    # that scatters and verifies it.  The base stays cached under its own
    # key, so alternating between states costs a delta once and hits after.
    # Replaces the in-place patch; bounded by patch_args_max_fraction.
    "rebase_tensor_args": False,
    # With cache_tensor_args: a worker keeps the CUDA tensors it RETURNS in
    # HBM as argument masters (one kernel launch gathers, copies and
    # checksums them), and when a later electron on that worker takes them
    # as arguments, whoever handled them in between, only their name
    # travels.  Results are split into buffers where the argument side
    # splits them: a tensor of at least min(pinned_staging_threshold_bytes,
    # arg_cache_min_bytes) is its own buffer, smaller ones share the packed
    # arena (pack_tensor_results).  Every retained buffer carries a checksum
    # that the dispatcher verifies.  Shares the arg_cache_bytes budget.
    "retain_tensor_results": False,
    "cpu_workers": 4,  # worker-set size when no GPU policy is active
    # Sample HBM occupancy (hipMemGetInfo) into the task meta every Nth
    # electron per worker; 0 = off (keeps the no-op hot path minimal).
    "gpu_telemetry_every": 0,
    "task_timeout": 0,  # seconds; 0 = unlimited
    "worker_idle_timeout": 0,  # seconds; 0 = workers never exit on idle
    # Opt-in: re-run a task whose worker died AFTER execution had started
    # (the worker acks each request before running user code; a task that
    # never acked is always safe to retry and always is).  Off by default
    # because a non-idempotent task could execute twice.
    "retry_on_worker_death": False,
}

update_config_defaults("executors.ssh", _EXECUTOR_PLUGIN_DEFAULTS)


def _conf(key: str, explicit: Any, default: Any = None) -> Any:
    """Reference resolution order: explicit ctor arg -> config -> default
    (reference ssh.py:94-124), hardened against missing config keys."""
    if explicit is not None and explicit != "":
        return explicit
    try:
        value = get_config(f"executors.ssh.{key}")
    except KeyError:
        value = None
    if value is None or value == "":
        return default if default is not None else _EXECUTOR_PLUGIN_DEFAULTS.get(key)
    return value


@functools.lru_cache(maxsize=64)
def _script_digest(text: str) -> str:
    import hashlib

    return hashlib.sha256(text.encode()).hexdigest()[:12]


class SSHTaskError(RuntimeError):
    """Dispatcher-side failure of the SSH pipeline (not the user task)."""


class SSHConnectError(SSHTaskError):
    """The endpoint could not be reached / verified BEFORE any task code
    could have started (connect exhaustion, environment-check failure).
    Safe to fail over to another node — nothing executed."""


class FusedStreamParser:
    """Incremental splitter for the fused dispatch's stdout stream:
    ``<task stdout> s_result <result bytes> s_meta <meta json>``.

    Result bytes go to ``result_writer`` (a callable, normally a lazy
    file writer) as they arrive, with an incremental sha256 — a
    multi-GiB result never accumulates in memory.
    Task stdout and meta are kept in RAM, bounded by ``cap``.  Sentinels
    may straddle chunk boundaries (a ``len(sentinel)-1`` tail is always
    retained for rescanning).
    """

    def __init__(self, s_result: bytes, s_meta: bytes, result_writer, cap: int = 4 << 20):
        import hashlib

        self.s_result = s_result
        self.s_meta = s_meta
        self.writer = result_writer
        self.cap = cap
        self.state = 0  # 0 = task stdout, 1 = result bytes, 2 = meta
        self.task_out = bytearray()
        self._meta = bytearray()
        self.sha = hashlib.sha256()
        self._buf = b""

    def _bounded(self, acc: bytearray, data: bytes) -> None:
        if len(acc) < self.cap:
            acc.extend(data[: self.cap - len(acc)])

    def _write_result(self, data: bytes) -> None:
        if data:
            self.writer(data)
            self.sha.update(data)

    def feed(self, chunk: bytes) -> None:
        buf = self._buf + chunk
        progress = True
        while buf and progress:
            progress = False
            if self.state == 0:
                idx = buf.find(self.s_result)
                if idx >= 0:
                    self._bounded(self.task_out, buf[:idx])
                    buf = buf[idx + len(self.s_result):]
                    self.state = 1
                    progress = True
                else:
                    emit = len(buf) - (len(self.s_result) - 1)
                    if emit > 0:
                        self._bounded(self.task_out, buf[:emit])
                        buf = buf[emit:]
            elif self.state == 1:
                idx = buf.find(self.s_meta)
                if idx >= 0:
                    self._write_result(buf[:idx])
                    buf = buf[idx + len(self.s_meta):]
                    self.state = 2
                    progress = True
                else:
                    emit = len(buf) - (len(self.s_meta) - 1)
                    if emit > 0:
                        self._write_result(buf[:emit])
                        buf = buf[emit:]
            else:
                self._bounded(self._meta, buf)
                buf = b""
        self._buf = buf

    def finish(self) -> None:
        """Flush the retained tail at EOF."""
        buf, self._buf = self._buf, b""
        if self.state == 0:
            self._bounded(self.task_out, buf)
        elif self.state == 1:
            self._write_result(buf)
        else:
            self._bounded(self._meta, buf)

    @property
    def have_result(self) -> bool:
        return self.state >= 1

    @property
    def sha_hex(self) -> Optional[str]:
        return self.sha.hexdigest() if self.have_result else None

    @property
    def meta_bytes(self) -> Optional[bytes]:
        return bytes(self._meta) if self.state == 2 else None


class _LazyFileWriter:
    """Opens the target file only when the first byte arrives, so a
    failed task never leaves a stray empty result file."""

    def __init__(self, path: str):
        self.path = path
        self.f = None

    def __call__(self, data: bytes) -> None:
        if self.f is None:
            self.f = open(self.path, "wb")
        self.f.write(data)

    def close(self) -> None:
        if self.f is not None:
            self.f.close()
            self.f = None


class SSHExecutor(RemoteExecutor):
    """Async executor running one covalent electron per call on a remote
    (8×MI355X) host over pooled SSH."""

    def __init__(
        self,
        username: str = "",
        hostname: str = "",
        ssh_key_file: str = "",
        cache_dir: str = "",
        python_path: str = "",
        conda_env: str = "",
        remote_cache: str = "",
        run_local_on_ssh_fail: Optional[bool] = None,
        remote_workdir: str = "",
        create_unique_workdir: Optional[bool] = None,
        poll_freq: int = 15,
        do_cleanup: bool = True,
        retry_connect: bool = True,
        max_connection_attempts: int = 5,
        retry_wait_time: int = 5,
        *,
        transport: str = "",
        ssh_port: Optional[int] = None,
        gpu_slots: Optional[int] = None,
        slots_per_gpu: Optional[int] = None,
        hip_visible_devices_policy: str = "",
        warmup_gpu: Optional[bool] = None,
        pinned_staging_threshold_bytes: Optional[int] = None,
        batch_roundtrips: Optional[bool] = None,
        persistent_workers: Optional[bool] = None,
        isolate_tasks: Optional[bool] = None,
        isolate_preload: str = "",
        device_tensor_args: Optional[bool] = None,
        pack_tensor_results: Optional[bool] = None,
        pack_results_min_bytes: Optional[int] = None,
        cache_tensor_args: Optional[bool] = None,
        arg_cache_bytes: Optional[int] = None,
        arg_cache_min_bytes: Optional[int] = None,
        pack_tensor_args: Optional[bool] = None,
        pack_args_min_bytes: Optional[int] = None,
        patch_tensor_args: Optional[bool] = None,
        patch_args_max_fraction: Optional[float] = None,
        rebase_tensor_args: Optional[bool] = None,
        retain_tensor_results: Optional[bool] = None,
        cpu_workers: Optional[int] = None,
        gpu_telemetry_every: Optional[int] = None,
        task_timeout: Optional[float] = None,
        worker_idle_timeout: Optional[float] = None,
        retry_on_worker_death: Optional[bool] = None,
        fixed_gpu: int = 0,
        ssh_extra_options: Optional[List[str]] = None,
        local_home: str = "",
    ) -> None:
        remote_cache = _conf("remote_cache", remote_cache)
        super().__init__(poll_freq=poll_freq, remote_cache=remote_cache)

        self.username = _conf("username", username, default="")
        self.hostname = _conf("hostname", hostname, default="")
        self.python_path = _conf("python_path", python_path)
        self.conda_env = _conf("conda_env", conda_env, default="")
        self.run_local_on_ssh_fail = bool(
            _conf("run_local_on_ssh_fail", run_local_on_ssh_fail, default=False)
        )
        self.remote_workdir = _conf("remote_workdir", remote_workdir)
        self.create_unique_workdir = bool(
            _conf("create_unique_workdir", create_unique_workdir, default=False)
        )
        self.do_cleanup = do_cleanup
        self.retry_connect = retry_connect
        self.max_connection_attempts = max_connection_attempts
        self.retry_wait_time = retry_wait_time

        cache = _conf("cache_dir", cache_dir)
        self.cache_dir = str(Path(cache).expanduser().resolve())
        key_file = _conf("ssh_key_file", ssh_key_file)
        self.ssh_key_file = str(Path(key_file).expanduser()) if key_file else ""

        # MI355X-native knobs
        self.transport_kind = _conf("transport", transport)
        self.ssh_port = int(_conf("ssh_port", ssh_port))
        self.gpu_slots = int(_conf("gpu_slots", gpu_slots))
        self.slots_per_gpu = int(_conf("slots_per_gpu", slots_per_gpu))
        self.hip_visible_devices_policy = _conf(
            "hip_visible_devices_policy", hip_visible_devices_policy
        )
        self.warmup_gpu = bool(_conf("warmup_gpu", warmup_gpu, default=True))
        self.pinned_staging_threshold_bytes = int(
            _conf("pinned_staging_threshold_bytes", pinned_staging_threshold_bytes)
        )
        self.batch_roundtrips = bool(_conf("batch_roundtrips", batch_roundtrips, default=True))
        self.isolate_tasks = bool(_conf("isolate_tasks", isolate_tasks, default=False))
        self.isolate_preload = _conf("isolate_preload", isolate_preload)
        self.persistent_workers = bool(
            _conf("persistent_workers", persistent_workers, default=False)
        ) or self.isolate_tasks  # isolation rides the worker channel
        self.device_tensor_args = bool(
            _conf("device_tensor_args", device_tensor_args, default=False)
        )
        if self.device_tensor_args and not self.persistent_workers:
            raise ValueError(
                "device_tensor_args needs persistent_workers or isolate_tasks: "
                "only the worker channel carries tensor arguments out of band"
            )
        self.pack_tensor_results = bool(
            _conf("pack_tensor_results", pack_tensor_results, default=False)
        )
        if self.pack_tensor_results and not self.persistent_workers:
            raise ValueError(
                "pack_tensor_results needs persistent_workers or isolate_tasks: "
                "only the worker channel carries result tensors out of band"
            )
        self.pack_results_min_bytes = int(
            _conf("pack_results_min_bytes", pack_results_min_bytes)
        )
        self.cache_tensor_args = bool(
            _conf("cache_tensor_args", cache_tensor_args, default=False)
        )
        if self.cache_tensor_args and self.isolate_tasks:
            raise ValueError(
                "cache_tensor_args cannot be combined with isolate_tasks: the "
                "zygote may not touch HIP, and the forked children that do "
                "hold the tensors do not outlive a task"
            )
        if self.cache_tensor_args and not (
            self.device_tensor_args and self.persistent_workers
        ):
            raise ValueError(
                "cache_tensor_args needs device_tensor_args=True and "
                "persistent_workers=True: the cache holds tensor arguments in "
                "the HBM of a worker that outlives the task"
            )
        self.arg_cache_bytes = int(_conf("arg_cache_bytes", arg_cache_bytes))
        self.arg_cache_min_bytes = int(
            _conf("arg_cache_min_bytes", arg_cache_min_bytes)
        )
        if self.cache_tensor_args and self.arg_cache_bytes <= 0:
            raise ValueError("arg_cache_bytes must be positive with cache_tensor_args")
        if self.cache_tensor_args and self.arg_cache_min_bytes < 0:
            raise ValueError("arg_cache_min_bytes must not be negative")
        self.pack_tensor_args = bool(
            _conf("pack_tensor_args", pack_tensor_args, default=False)
        )
        if self.pack_tensor_args and not self.device_tensor_args:
            raise ValueError(
                "pack_tensor_args needs device_tensor_args=True: it packs the "
                "tensor arguments that land in the worker's HBM"
            )
        self.pack_args_min_bytes = int(
            _conf("pack_args_min_bytes", pack_args_min_bytes)
        )
        if self.pack_args_min_bytes < 0:
            raise ValueError("pack_args_min_bytes must not be negative")
        self.patch_tensor_args = bool(
            _conf("patch_tensor_args", patch_tensor_args, default=False)
        )
        if self.patch_tensor_args and not (
            self.cache_tensor_args and self.pack_tensor_args
        ):
            raise ValueError(
                "patch_tensor_args needs cache_tensor_args=True and "
                "pack_tensor_args=True: it patches a packed argument arena "
                "that the worker holds in its cache"
            )
        self.patch_args_max_fraction = float(
            _conf("patch_args_max_fraction", patch_args_max_fraction, default=0.5)
        )
        if not 0.0 < self.patch_args_max_fraction <= 1.0:
            raise ValueError("patch_args_max_fraction must be in (0, 1]")
        self.rebase_tensor_args = bool(
            _conf("rebase_tensor_args", rebase_tensor_args, default=False)
        )
        if self.rebase_tensor_args and not self.patch_tensor_args:
            raise ValueError(
                "rebase_tensor_args needs patch_tensor_args=True: it builds a "
                "packed argument arena from one that the worker holds in its "
                "cache plus a delta"
            )
        self.retain_tensor_results = bool(
            _conf("retain_tensor_results", retain_tensor_results, default=False)
        )
        if self.retain_tensor_results and not self.cache_tensor_args:
            raise ValueError(
                "retain_tensor_results needs cache_tensor_args=True: a retained "
                "result is held as a master in the worker's argument cache and "
                "reused through its references"
            )
        self.cpu_workers = int(_conf("cpu_workers", cpu_workers))
        self.gpu_telemetry_every = int(
            _conf("gpu_telemetry_every", gpu_telemetry_every, default=0) or 0
        )
        self.task_timeout = float(_conf("task_timeout", task_timeout, default=0) or 0)
        self.worker_idle_timeout = float(
            _conf("worker_idle_timeout", worker_idle_timeout, default=0) or 0
        )
        self.retry_on_worker_death = bool(
            _conf("retry_on_worker_death", retry_on_worker_death, default=False)
        )
        self.fixed_gpu = int(fixed_gpu)
        #: raw `ssh -o`/flag passthrough, e.g. ["-o", "StrictHostKeyChecking=yes",
        #: "-J", "bastion"] (the default host-key policy matches the
        #: reference: known_hosts disabled, reference ssh.py:267)
        self.ssh_extra_options = list(ssh_extra_options or [])
        self.local_home = local_home

        #: in-flight worker-dispatched tasks: operation_id -> worker key
        self._inflight: Dict[str, Tuple] = {}
        #: in-flight stub/fused tasks: operation_id -> remote pidfile
        self._inflight_fused: Dict[str, str] = {}
        #: operation_ids cancelled while in flight
        self._cancelled: set = set()
        #: most recent completed task's per-phase timing record
        self.last_task_record: Optional[TaskRecord] = None
        #: bounded history of task records (bench reads this)
        self.task_records: List[TaskRecord] = []
        #: operational counters (observability)
        self.counters: Dict[str, int] = {
            "tasks": 0,
            "task_exceptions": 0,
            "worker_respawns": 0,
            "cancellations": 0,
            "ssh_failures": 0,
            # cache_tensor_args: arguments sent as a key alone, references
            # the worker no longer held (each costs one resend), and the
            # argument bytes that did not travel
            "arg_cache_hits": 0,
            "arg_cache_misses": 0,
            "arg_cache_bytes_saved": 0,
            # patch_tensor_args: packed arenas sent as a delta against an
            # arena the worker held (the bytes left out count as saved)
            "arg_cache_patches": 0,
            # rebase_tensor_args: packed arenas built on the worker from a
            # held arena plus a delta (the bytes left out count as saved)
            "arg_cache_rebases": 0,
            # retain_tensor_results: result buffers the worker kept in HBM
            # for reuse as arguments, and their bytes
            "results_retained": 0,
            "results_retained_bytes": 0,
        }

    # ------------------------------------------------------------------
    # Endpoint identity / pooled state
    # ------------------------------------------------------------------

    def _pool_key(self) -> Tuple[str, ...]:
        if self.transport_kind == "local":
            return ("local", self.local_home or os.path.expanduser("~"))
        return (
            "ssh",
            self.hostname,
            self.username,
            self.ssh_key_file,
            str(self.ssh_port),
            ",".join(self.ssh_extra_options),
        )

    def _make_transport(self) -> Transport:
        if self.transport_kind == "local":
            return LocalTransport(home=self.local_home or None)
        return OpenSSHTransport(
            hostname=self.hostname,
            username=self.username,
            ssh_key_file=self.ssh_key_file,
            port=self.ssh_port,
            extra_options=self.ssh_extra_options,
        )

    def _slot_table(self) -> gpu_slots.SlotTable:
        return gpu_slots.get_slot_table(
            self._pool_key(), num_gpus=self.gpu_slots, slots_per_gpu=self.slots_per_gpu
        )

    # ------------------------------------------------------------------
    # Failure policy (reference ssh.py:181-208)
    # ------------------------------------------------------------------

    async def _on_ssh_fail(
        self,
        function: Callable,
        args: list,
        kwargs: dict,
        message: str,
        error_cls: type = SSHTaskError,
    ) -> Any:
        """If ``run_local_on_ssh_fail``, run the task on the dispatcher
        host; otherwise raise (reference ssh.py:202-208; the reference
        raises RuntimeError — SSHTaskError/SSHConnectError are
        RuntimeError subclasses, so the surface is compatible while the
        cluster's failover can distinguish pre-execution failures)."""
        self.counters["ssh_failures"] += 1
        app_log.warning("SSH dispatch failed: %s", message)
        if self.run_local_on_ssh_fail:
            return await asyncio.to_thread(function, *args, **kwargs)
        raise error_cls(message)

    # ------------------------------------------------------------------
    # RemoteExecutor template methods (reference ssh.py:317-464)
    # ------------------------------------------------------------------

    async def _validate_credentials(self, raise_exception: bool = True) -> bool:
        """SSH key file must exist (reference ssh.py:317-335).  The local
        transport needs no credentials."""
        if self.transport_kind == "local":
            return True
        if self.ssh_key_file and os.path.exists(self.ssh_key_file):
            return True
        if raise_exception:
            raise RuntimeError(f"no SSH key file found at {self.ssh_key_file}")
        return False

    async def _client_connect(self) -> Optional[Transport]:
        """Connect (or fetch from pool) with the reference's retry policy:
        up to ``max_connection_attempts`` attempts spaced by
        ``retry_wait_time`` (reference ssh.py:237-282); returns None on
        exhaustion, raises immediately if ``retry_connect`` is False."""
        attempts = self.max_connection_attempts if self.retry_connect else 1
        last_error: Optional[Exception] = None
        for attempt in range(attempts):
            try:
                return await transport_pool.get_transport(
                    self._pool_key(), self._make_transport
                )
            except (TransportConnectError, OSError, asyncio.TimeoutError) as e:
                last_error = e
                if not self.retry_connect:
                    raise
                app_log.warning(
                    "connect attempt %d/%d to %s failed: %s",
                    attempt + 1,
                    attempts,
                    self.hostname or "local",
                    e,
                )
                if attempt + 1 < attempts:
                    await asyncio.sleep(self.retry_wait_time)
        app_log.error("connection exhausted after %d attempts: %s", attempts, last_error)
        return None

    async def _upload_task(
        self, transport: Transport, files: List[Tuple[str, str]]
    ) -> None:
        """Batched upload of the staged task files (replaces the
        reference's two scp calls, ssh.py:360-361)."""
        await transport.put_files(files)

    def _submit_command(self, remote_script_file: str) -> str:
        """Remote command string: ``{python_path} {script}`` with the
        conda activation wrapper when ``conda_env`` is set (reference
        ssh.py:377-380)."""
        return self._wrap_conda(
            f"{self.python_path} {shlex.quote(remote_script_file)}"
        )

    @staticmethod
    def _setsid_fragment(inner: str, pidfile: str) -> str:
        """Launch ``inner`` in its own session (process group) and record
        the PGID, so ``cancel()`` can kill the whole remote task tree
        (the reference cannot cancel at all, reference
        ssh.py:460-464).  Leaves the task's exit status in ``$_csp_rc``.

        A task exiting 255 is remapped to 254: the ssh client reserves
        255 for its own connection failures, and an un-remapped 255 would
        make the dispatcher treat a completed task as a dropped
        connection (transport/openssh.py:145).
        """
        q = shlex.quote
        return (
            f"setsid bash -c {q(inner)} < /dev/null & _csp_pid=$!; "
            f"echo $_csp_pid > {q(pidfile)}; "
            f"wait $_csp_pid; _csp_rc=$?; rm -f {q(pidfile)}; "
            f'if [ "$_csp_rc" -eq 255 ]; then _csp_rc=254; fi'
        )

    def _pidfile(self, operation_id: str) -> str:
        return f"{self.remote_cache}/pid_{operation_id}"

    async def _kill_remote_group(self, transport: Transport, pidfile: str) -> None:
        """Best-effort TERM-then-KILL of the remote process group whose
        PGID is recorded in ``pidfile`` (cancel / timeout path)."""
        q = shlex.quote
        try:
            await asyncio.wait_for(
                transport.run(
                    f"if [ -f {q(pidfile)} ]; then _p=$(cat {q(pidfile)}); "
                    f'kill -TERM -- "-$_p" 2>/dev/null || true; sleep 0.5; '
                    f'kill -KILL -- "-$_p" 2>/dev/null || true; '
                    f"rm -f {q(pidfile)}; fi"
                ),
                timeout=15,
            )
        except Exception:  # noqa: BLE001 - the task error is what matters
            app_log.debug("remote group kill failed", exc_info=True)

    async def submit_task(
        self,
        transport: Transport,
        remote_script_file: str,
        env: Optional[dict] = None,
        operation_id: Optional[str] = None,
    ) -> CompletedCommand:
        """Synchronous submit: awaits the remote process exit (reference
        ssh.py:363-386).  With an ``operation_id`` the task runs under
        setsid with its PGID recorded, making it cancellable."""
        if operation_id is None:
            return await transport.run(
                self._submit_command(remote_script_file), env=env
            )
        pidfile = self._pidfile(operation_id)
        cmd = (
            self._setsid_fragment(
                self._submit_command(remote_script_file), pidfile
            )
            + "; exit $_csp_rc"
        )
        self._inflight_fused[operation_id] = pidfile
        try:
            return await transport.run(
                cmd, env=env, timeout=self.task_timeout or None
            )
        except asyncio.TimeoutError:
            # take the remote process group down with the timed-out wait
            await self._kill_remote_group(transport, pidfile)
            raise SSHTaskError(
                f"task {operation_id} exceeded task_timeout="
                f"{self.task_timeout}s"
            )
        finally:
            self._inflight_fused.pop(operation_id, None)

    async def get_status(self, transport: Transport, remote_result_file: str) -> bool:
        """True iff the remote result file exists (the reference compares
        ``ls`` output for equality, ssh.py:402-406)."""
        proc = await transport.run(f"ls {shlex.quote(remote_result_file)}")
        return proc.ok and proc.text_out().strip() == remote_result_file

    async def _poll_task(
        self, transport: Transport, remote_result_file: str, retries: int = 5
    ) -> bool:
        """Poll for the result file.  First check is immediate (submit is
        synchronous, so the file normally exists already — SURVEY.md §7
        latency note); then sleep ``poll_freq`` between at most
        ``retries`` further checks (reference ssh.py:408-432)."""
        for attempt in range(retries + 1):
            if await self.get_status(transport, remote_result_file):
                return True
            if attempt < retries:
                await asyncio.sleep(self.poll_freq)
        return False

    async def query_result(
        self, transport: Transport, remote_result_file: str, local_result_file: str
    ) -> Tuple[Any, Optional[Exception]]:
        """Fetch and unpickle the ``(result, exception)`` 2-tuple
        (reference ssh.py:434-458)."""
        await transport.get_file(remote_result_file, local_result_file)
        with open(local_result_file, "rb") as f:
            return stdlib_pickle.load(f)

    async def cancel(self, task_metadata: Optional[dict] = None, *args: Any, **kwargs: Any) -> None:
        """Cancel a running task.

        The reference leaves this unimplemented (reference ssh.py:460-464).
        Here, a task dispatched through a persistent worker CAN be
        cancelled: the worker process serving it is killed (the in-flight
        request fails with ChannelClosed and a fresh worker replaces it
        for subsequent electrons).  If OTHER electrons were pipelined on
        the same worker, any that had already started execution fail
        loudly with an explanatory SSHTaskError instead of being silently
        re-executed (worker A1 ack protocol); electrons the worker had
        not yet started are transparently re-dispatched — always safe.
        Stub/fused-dispatched tasks run under ``setsid`` with their
        remote PGID recorded, and cancel kills that whole process group
        (VERDICT r1 item 5 — the reference raises NotImplementedError
        everywhere).
        """
        task_metadata = task_metadata or {}
        operation_id = (
            f"{task_metadata.get('dispatch_id', 'dispatch')}_"
            f"{task_metadata.get('node_id', 0)}"
        )
        key = self._inflight.get(operation_id)
        if key is not None:
            self._cancelled.add(operation_id)
            self.counters["cancellations"] += 1
            await worker_pool.kill(key)
            return
        pidfile = self._inflight_fused.get(operation_id)
        if pidfile is not None:
            # stub/fused task: the remote ran under setsid with its PGID
            # recorded — kill the whole remote process group (TERM, then
            # KILL after a grace period).
            self._cancelled.add(operation_id)
            self.counters["cancellations"] += 1
            transport = await transport_pool.get_transport(
                self._pool_key(), self._make_transport
            )
            await self._kill_remote_group(transport, pidfile)
            return
        raise NotImplementedError(
            f"no in-flight task {operation_id!r} to cancel"
        )

    # ------------------------------------------------------------------
    # Staging (reference ssh.py:126-179)
    # ------------------------------------------------------------------

    def _task_paths(self, operation_id: str) -> Dict[str, str]:
        rc = self.remote_cache
        return {
            "function_local": os.path.join(self.cache_dir, f"function_{operation_id}.pkl"),
            "script_local": os.path.join(self.cache_dir, f"exec_{operation_id}.py"),
            "result_local": os.path.join(self.cache_dir, f"result_{operation_id}.pkl"),
            "meta_local": os.path.join(self.cache_dir, f"meta_{operation_id}.json"),
            "function_remote": f"{rc}/function_{operation_id}.pkl",
            "script_remote": f"{rc}/exec_{operation_id}.py",
            "result_remote": f"{rc}/result_{operation_id}.pkl",
            "meta_remote": f"{rc}/meta_{operation_id}.json",
        }

    def _write_function_files(
        self,
        operation_id: str,
        fn: Callable,
        args: list,
        kwargs: dict,
        current_remote_workdir: str,
        gpu_lib_path: str = "",
    ) -> Dict[str, str]:
        """Serialize ``(fn, args, kwargs)`` with cloudpickle and render
        the exec stub (reference ssh.py:126-179; same file names and
        pickle layout)."""
        paths = self._task_paths(operation_id)
        Path(self.cache_dir).mkdir(parents=True, exist_ok=True)
        with open(paths["function_local"], "wb") as f:
            cloudpickle.dump((fn, args, kwargs), f)
        script = render_stub(
            remote_result_file=paths["result_remote"],
            remote_function_file=paths["function_remote"],
            current_remote_workdir=current_remote_workdir,
            remote_meta_file=paths["meta_remote"],
            gpu_lib_path=gpu_lib_path,
            warmup=self.warmup_gpu,
            staging_threshold=self.pinned_staging_threshold_bytes,
        )
        Path(paths["script_local"]).write_text(script)
        return paths

    # ------------------------------------------------------------------
    # One-time per-endpoint environment checks (hoisted out of the
    # per-task path; reference does these per task at ssh.py:508-532)
    # ------------------------------------------------------------------

    async def _ensure_environment(self, transport: Transport) -> Tuple[str, bool]:
        """Verify python/conda once per endpoint and provision the GPU
        library.  Returns ``(remote_gpu_lib_path_or_empty, has_gpu)`` —
        the two are independent: slot scheduling keys off ``has_gpu``
        (the endpoint exposes /dev/kfd), library provisioning only adds
        the warm-up/pinned-staging fast path (pinning must
        not silently disappear when the dispatcher-side .so is absent)."""
        key = self._pool_key()
        cached = transport_pool.cached_check(key, "env")
        if cached is not None:
            ok, detail, gpu_lib, has_gpu = cached
            if not ok:
                raise SSHTaskError(detail)
            return gpu_lib, has_gpu

        async with transport_pool.check_lock(key):
            cached = transport_pool.cached_check(key, "env")
            if cached is not None:
                ok, detail, gpu_lib, has_gpu = cached
                if not ok:
                    raise SSHTaskError(detail)
                return gpu_lib, has_gpu
            return await self._ensure_environment_locked(transport, key)

    async def _ensure_environment_locked(
        self, transport: Transport, key
    ) -> Tuple[str, bool]:
        # conda env existence (reference ssh.py:508-519)
        if self.conda_env:
            proc = await transport.run(
                f'eval "$(conda shell.bash hook)" && conda env list | grep {shlex.quote(self.conda_env)}'
            )
            if not proc.ok:
                detail = f"conda environment {self.conda_env!r} not found on {transport.endpoint}"
                transport_pool.store_check(key, "env", (False, detail, "", False), ok=False)
                raise SSHTaskError(detail)

        # python3 sanity (reference ssh.py:521-524) + remote cache dir +
        # GPU presence, all in one round trip
        proc = await transport.run(
            self._wrap_conda(f"{self.python_path} --version")
            + f" && mkdir -p {shlex.quote(self.remote_cache)}"
            + " && { test -e /dev/kfd && echo CSP_HAS_GPU || true; }"
        )
        if not proc.ok or "3" not in (proc.text_out() + proc.text_err()):
            detail = (
                f"no python3 at {self.python_path!r} on {transport.endpoint}: "
                f"{proc.text_err().strip()}"
            )
            transport_pool.store_check(key, "env", (False, detail, "", False), ok=False)
            raise SSHTaskError(detail)

        # Only provision the CDNA4 library when the endpoint actually has
        # an AMD GPU stack; slot scheduling follows has_gpu alone.
        has_gpu = "CSP_HAS_GPU" in proc.text_out()
        gpu_lib = await self._provision_gpu_lib(transport) if has_gpu else ""
        if has_gpu and not gpu_lib:
            app_log.warning(
                "endpoint %s has a GPU stack but the CDNA4 warm-up/staging "
                "library (libcsp_gpu.so) is not built on the dispatcher — "
                "GPU slot pinning stays ACTIVE, but tasks run without the "
                "warm-up kernel and pinned staging fast path",
                transport.endpoint,
            )
        transport_pool.store_check(key, "env", (True, "", gpu_lib, has_gpu))
        return gpu_lib, has_gpu

    def _wrap_conda(self, cmd: str) -> str:
        if self.conda_env:
            return (
                'eval "$(conda shell.bash hook)" && '
                f"conda activate {shlex.quote(self.conda_env)} && {cmd}"
            )
        return cmd

    async def _provision_gpu_lib(self, transport: Transport) -> str:
        """Ship the in-tree libcsp_gpu.so (CDNA4 probe/warm-up + pinned
        staging) to the endpoint once, content-addressed."""
        from .gpu.probe import local_gpu_lib_path

        local_lib = local_gpu_lib_path()
        if not local_lib:
            return ""
        import hashlib

        digest = hashlib.sha256(Path(local_lib).read_bytes()).hexdigest()[:12]
        remote_lib = f"{self.remote_cache}/lib/csp_gpu-{digest}.so"
        # mkdir -p here, not left to tar: two endpoints that share a remote
        # filesystem (two names for one home) provision at the same time,
        # and concurrent tar extractions race creating the same lib/ dir
        probe = await transport.run(
            f"mkdir -p {shlex.quote(self.remote_cache + '/lib')} && "
            f"test -f {shlex.quote(remote_lib)}"
        )
        if not probe.ok:
            # publish atomically (rename) so a concurrent stub can never
            # ctypes-load a half-written library
            remote_tmp = f"{remote_lib}.tmp-{uuid.uuid4().hex[:8]}"
            await transport.put_files([(local_lib, remote_tmp)])
            await transport.run(
                f"mv -f {shlex.quote(remote_tmp)} {shlex.quote(remote_lib)}"
            )
        return remote_lib

    async def _provision_worker_script(self, transport: Transport, gpu_lib: str) -> str:
        """Ship the rendered persistent-worker script once per endpoint,
        content-addressed (re-ships automatically when config that
        affects the rendering changes)."""
        import hashlib

        text = render_worker(
            gpu_lib_path=gpu_lib,
            warmup=self.warmup_gpu,
            staging_threshold=self.pinned_staging_threshold_bytes,
            idle_timeout=self.worker_idle_timeout,
            isolate=self.isolate_tasks,
            isolate_preload=self.isolate_preload,
            telemetry_every=self.gpu_telemetry_every,
            pack_results=self.pack_tensor_results,
            pack_min_bytes=self.pack_results_min_bytes,
            arg_cache_bytes=self.arg_cache_bytes if self.cache_tensor_args else 0,
            retain_min_bytes=(
                self.arg_cache_min_bytes if self.retain_tensor_results else None
            ),
        )
        digest = _script_digest(text)
        key = self._pool_key()
        check_name = f"worker_script:{digest}"
        cached = transport_pool.cached_check(key, check_name)
        if cached:
            return cached
        # Serialize provisioning per endpoint: a cold-start fan of N
        # electrons must upload once, not N times — and concurrent tar
        # extractions creating the same remote lib/ dir can race inside
        # tar's mkdir and fail spuriously.
        async with transport_pool.check_lock(key):
            cached = transport_pool.cached_check(key, check_name)
            if cached:
                return cached
            remote_path = f"{self.remote_cache}/lib/worker-{digest}.py"
            probe = await transport.run(f"test -f {shlex.quote(remote_path)}")
            if not probe.ok:
                Path(self.cache_dir).mkdir(parents=True, exist_ok=True)
                # unique temp names local AND remote; the remote rename
                # makes the publish atomic (no reader ever sees a
                # half-written file)
                nonce = uuid.uuid4().hex[:8]
                local_tmp = os.path.join(
                    self.cache_dir, f"worker-{digest}-{nonce}.py"
                )
                remote_tmp = f"{remote_path}.tmp-{nonce}"
                Path(local_tmp).write_text(text)
                try:
                    await transport.put_files([(local_tmp, remote_tmp)])
                    await transport.run(
                        f"mv -f {shlex.quote(remote_tmp)} {shlex.quote(remote_path)}"
                    )
                finally:
                    try:
                        os.remove(local_tmp)
                    except OSError:
                        pass
            transport_pool.store_check(key, check_name, remote_path)
            return remote_path

    async def _dispatch_worker(
        self,
        transport: Transport,
        operation_id: str,
        function_blob: bytes,
        workdir: str,
        env: Optional[dict],
        gpu_lib: str,
        worker_tag: object,
        arg_meta=None,
        arg_bufs=None,
    ):
        """Run one electron on the persistent worker for ``worker_tag``
        (a GPU slot id, or a CPU worker index).  Respawns a dead worker
        once before giving up."""
        from .transport.channel import ChannelClosed

        script_remote = await self._provision_worker_script(transport, gpu_lib)
        # key includes the script identity so config changes (which ship a
        # new content-addressed script) spawn fresh workers instead of
        # talking a new protocol to a stale process
        key = (self._pool_key(), worker_tag, script_remote)
        cmd = self._wrap_conda(
            f"{self.python_path} {shlex.quote(script_remote)}"
        )

        async def launcher():
            return await transport.open_channel(cmd, env=env)

        self._inflight[operation_id] = key
        try:
            for attempt in (0, 1):
                try:
                    handle = await worker_pool.get_worker(key, launcher)
                except worker_pool.WorkerStartupError:
                    # transient spawn failure (loaded machine, dropped
                    # channel): one clean retry before surfacing
                    if attempt == 1:
                        raise
                    await asyncio.sleep(0.5)
                    continue
                ack_state = {"started": False}
                try:
                    return await worker_pool.run_task(
                        handle,
                        operation_id,
                        workdir,
                        function_blob,
                        timeout=self.task_timeout or None,
                        arg_buffer_meta=arg_meta,
                        arg_buffers=arg_bufs,
                        ack_state=ack_state,
                        cache_stats=self.counters,
                        **(
                            {"retain_segments": self.patch_tensor_args}
                            if self.retain_tensor_results
                            else {}
                        ),
                    )
                except asyncio.TimeoutError:
                    # the worker is wedged on this task: kill it so the
                    # slot/worker is usable again, then surface
                    await worker_pool.kill(key)
                    raise SSHTaskError(
                        f"task {operation_id} exceeded task_timeout="
                        f"{self.task_timeout}s"
                    )
                except ChannelClosed:
                    worker_pool.drop(key)
                    if operation_id in self._cancelled:
                        self._cancelled.discard(operation_id)
                        raise SSHTaskError(f"task {operation_id} was cancelled")
                    # Re-dispatch policy: the worker acks each
                    # request before executing user code.  No ack => the
                    # task never started and a retry cannot re-execute
                    # anything.  Ack received => user code may have
                    # partially run; re-running a non-idempotent task is
                    # only done when the user opted in.
                    if ack_state["started"] and not self.retry_on_worker_death:
                        raise SSHTaskError(
                            f"worker serving task {operation_id} died after "
                            "execution had started (possibly killed by a "
                            "cancel of a co-resident electron); not "
                            "re-executing automatically — the task may have "
                            "partially run.  Set retry_on_worker_death=True "
                            "to opt in to re-execution of idempotent tasks."
                        )
                    if attempt == 1:
                        raise
                    self.counters["worker_respawns"] += 1
                    app_log.warning(
                        "worker %s died %s task %s; respawning once",
                        key,
                        "during" if ack_state["started"] else "before",
                        operation_id,
                    )
        finally:
            self._inflight.pop(operation_id, None)

    # ------------------------------------------------------------------
    # Fused single-round-trip dispatch (streaming)
    # ------------------------------------------------------------------

    #: keep at most this much task stdout / stderr / meta in memory
    _STREAM_CAP = 4 << 20
    _IO_CHUNK = 1 << 20

    async def _dispatch_fused(
        self,
        transport: Transport,
        paths: Dict[str, str],
        env: Optional[dict],
        operation_id: str,
    ) -> Tuple[CompletedCommand, bool, Optional[str], Optional[bytes]]:
        """Stage + execute + fetch + clean in ONE transport round trip,
        with bounded dispatcher memory.

        stdin carries the staged files as a tar stream (spooled to disk
        beyond 32 MiB); stdout carries the task's own stdout, then
        sentinel-delimited result and meta bytes.  The result bytes are
        STREAMED straight into ``paths["result_local"]`` with an
        incremental sha256 — a multi-GiB return never exists as a second
        in-RAM copy (the reference scp'd to a file too, reference
        ssh.py:451; round 1 buffered the whole stream in memory).

        The task runs under setsid with its PGID recorded in a remote
        pidfile, so ``cancel()`` can kill it.

        Returns ``(CompletedCommand(rc, task_stdout, stderr),
        have_result, result_sha256, meta_bytes)``.
        """
        from .transport.base import make_tar_spool

        files = [
            (paths["function_local"], paths["function_remote"]),
            (paths["script_local"], paths["script_remote"]),
        ]
        spool, base = make_tar_spool(files)
        untar = "tar -xf - -C /" if base == "/" else "tar -xf -"

        token = uuid.uuid4().hex
        s_result = f"\n--CSP-RESULT-{token}--\n".encode()
        s_meta = f"\n--CSP-META-{token}--\n".encode()
        q = shlex.quote
        pidfile = self._pidfile(operation_id)
        rm_files = " ".join(
            q(paths[k]) for k in ("function_remote", "script_remote", "result_remote", "meta_remote")
        )
        cleanup = f"rm -f {rm_files}; " if self.do_cleanup else ""
        # NB: the staging prefix must be an `if` statement, not a `&& `
        # chain into the setsid fragment — `A && B && setsid C &` would
        # background the ENTIRE list (and a backgrounded tar reads
        # /dev/null, not our stream).
        cmd = (
            f"if mkdir -p {q(self.remote_cache)} && {untar}; then "
            + self._setsid_fragment(
                self._submit_command(paths["script_remote"]), pidfile
            )
            + "; else _csp_rc=$?; fi"
            + f"; if [ -f {q(paths['result_remote'])} ]; then "
            f"printf '%s' {q(s_result.decode())}; cat {q(paths['result_remote'])}; "
            f"printf '%s' {q(s_meta.decode())}; cat {q(paths['meta_remote'])} 2>/dev/null || true; "
            f"fi; {cleanup}exit $_csp_rc"
        )
        self._inflight_fused[operation_id] = pidfile
        proc = None
        try:
            proc = await transport.open_pipe(cmd, env=env)
            out = await asyncio.wait_for(
                self._stream_fused_io(
                    proc, spool, s_result, s_meta, paths["result_local"]
                ),
                timeout=self.task_timeout or None,
            )
        except asyncio.TimeoutError:
            if proc is not None and proc.returncode is None:
                proc.kill()
                await proc.wait()
            # killing the local client does not kill the remote task —
            # take down its recorded process group too
            await self._kill_remote_group(transport, pidfile)
            raise
        finally:
            self._inflight_fused.pop(operation_id, None)
            spool.close()

        rc, task_out, stderr, have_result, sha_hex, meta_bytes = out
        if rc == 255 and isinstance(transport, OpenSSHTransport):
            # ssh client connection failure (remote task rcs are remapped
            # away from 255 by _setsid_fragment): flag the pooled
            # transport so the retry policy reconnects.
            transport._connected = False
            raise TransportConnectError(
                f"ssh channel to {transport.endpoint} failed during task "
                f"{operation_id}: {stderr.decode(errors='replace').strip()}"
            )
        if task_out:
            app_log.debug("task stdout: %s", task_out.decode(errors="replace"))
        return (
            CompletedCommand(rc, bytes(task_out), bytes(stderr)),
            have_result,
            sha_hex,
            meta_bytes,
        )

    async def _stream_fused_io(
        self, proc, spool, s_result: bytes, s_meta: bytes, result_local: str
    ):
        """Drive one fused-dispatch subprocess: feed the tar, split
        stdout at the sentinels (FusedStreamParser), spool result bytes
        to disk."""
        CHUNK = self._IO_CHUNK
        CAP = self._STREAM_CAP

        async def feed_stdin():
            try:
                while True:
                    chunk = await asyncio.to_thread(spool.read, CHUNK)
                    if not chunk:
                        break
                    proc.stdin.write(chunk)
                    await proc.stdin.drain()
                proc.stdin.close()
            except (BrokenPipeError, ConnectionResetError):
                pass  # remote died early; rc/stderr will tell the story

        stderr_acc = bytearray()

        async def drain_stderr():
            while True:
                chunk = await proc.stderr.read(CHUNK)
                if not chunk:
                    break
                if len(stderr_acc) < CAP:
                    stderr_acc.extend(chunk[: CAP - len(stderr_acc)])

        feeder = asyncio.ensure_future(feed_stdin())
        err_task = asyncio.ensure_future(drain_stderr())
        writer = _LazyFileWriter(result_local)
        parser = FusedStreamParser(s_result, s_meta, writer, cap=CAP)
        try:
            while True:
                chunk = await proc.stdout.read(CHUNK)
                if not chunk:
                    break
                # GIL-released file writes happen inside feed()
                await asyncio.to_thread(parser.feed, chunk)
            parser.finish()
            await feeder
            await err_task
            rc = await proc.wait()
            return (
                rc,
                parser.task_out,
                stderr_acc,
                parser.have_result,
                parser.sha_hex,
                parser.meta_bytes,
            )
        finally:
            writer.close()
            # On cancellation/timeout the setsid'd remote task still
            # holds the stderr pipe open — cancel the drains instead of
            # waiting for a 60 s sleep to release them.
            for t in (feeder, err_task):
                if not t.done():
                    t.cancel()
            await asyncio.gather(feeder, err_task, return_exceptions=True)

    # ------------------------------------------------------------------
    # run() — the dispatcher-invoked entry point (reference ssh.py:466-591)
    # ------------------------------------------------------------------

    async def run(
        self,
        function: Callable,
        args: list,
        kwargs: dict,
        task_metadata: Optional[dict] = None,
    ) -> Any:
        task_metadata = task_metadata or {}
        dispatch_id = task_metadata.get("dispatch_id", "dispatch")
        node_id = task_metadata.get("node_id", 0)
        operation_id = f"{dispatch_id}_{node_id}"

        if self.create_unique_workdir:
            current_remote_workdir = (
                f"{self.remote_workdir}/{dispatch_id}/node_{node_id}"
            )
        else:
            current_remote_workdir = self.remote_workdir

        timer = PhaseTimer()
        record = TaskRecord(operation_id=operation_id)

        with timer.phase("validate"):
            await self._validate_credentials()

        with timer.phase("connect"):
            try:
                transport = await self._client_connect()
            except (TransportConnectError, OSError) as e:
                return await self._on_ssh_fail(
                    function, args, kwargs,
                    f"Could not connect to {self.hostname}: {e}",
                    error_cls=SSHConnectError,
                )
        if transport is None:
            return await self._on_ssh_fail(
                function,
                args,
                kwargs,
                f"Could not connect to {self.hostname} after "
                f"{self.max_connection_attempts} attempts",
                error_cls=SSHConnectError,
            )

        with timer.phase("env_checks"):
            try:
                gpu_lib, has_gpu = await self._ensure_environment(transport)
            except SSHTaskError as e:
                # pre-execution: nothing has run yet -> failover-safe
                return await self._on_ssh_fail(
                    function, args, kwargs, str(e), error_cls=SSHConnectError
                )

        slot = None
        # Slot policy keys off GPU PRESENCE, not library provisioning:
        # concurrency limiting + HIP_VISIBLE_DEVICES pinning must hold
        # even when the warm-up .so is unavailable.
        policy = self.hip_visible_devices_policy if has_gpu else "none"
        try:
            if policy == "roundrobin":
                with timer.phase("slot_wait"):
                    slot = await self._slot_table().acquire()
                env = slot.env()
                record.gpu_id = slot.gpu_id
            elif policy == "fixed":
                env = {"CSP_GPU_SLOT": str(self.fixed_gpu)}
                record.gpu_id = self.fixed_gpu
            else:
                env = None

            result: Any = None
            exception: Optional[Exception] = None
            paths: Optional[Dict[str, str]] = None

            if self.persistent_workers:
                if self.retain_tensor_results:
                    # results still being keyed in the background may be these
                    # arguments: their keys then come from the memo, unhashed
                    await worker_pool.join_retained_keying()
                with timer.phase("stage"):
                    # large CPU-tensor arguments travel as raw frames, not
                    # inside the pickle (mirror of the result staging)
                    s_args, s_kwargs, arg_meta, arg_bufs = (
                        worker_pool.extract_arg_buffers(
                            args, kwargs, self.pinned_staging_threshold_bytes,
                            to_device=self.device_tensor_args,
                            cache_min_bytes=(
                                self.arg_cache_min_bytes
                                if self.cache_tensor_args
                                else None
                            ),
                            pack_min_bytes=(
                                self.pack_args_min_bytes
                                if self.pack_tensor_args
                                else None
                            ),
                            patch_max_fraction=(
                                self.patch_args_max_fraction
                                if self.patch_tensor_args
                                else None
                            ),
                            **({"rebase": True} if self.rebase_tensor_args else {}),
                            **({"retain": True} if self.retain_tensor_results else {}),
                        )
                    )
                    function_blob = cloudpickle.dumps((function, s_args, s_kwargs))
                try:
                    with timer.phase("dispatch"):
                        result, exception, meta = await self._dispatch_worker(
                            transport,
                            operation_id,
                            function_blob,
                            current_remote_workdir,
                            env,
                            gpu_lib,
                            arg_meta=arg_meta,
                            arg_bufs=arg_bufs,
                            worker_tag=(
                                slot.worker_tag
                                if slot is not None
                                else record.gpu_id
                                if record.gpu_id is not None
                                else worker_pool.pick_cpu_tag(
                                    self._pool_key(), self.cpu_workers
                                )
                            ),
                        )
                    record.remote_meta = meta
                except (worker_pool.WorkerStartupError, ConnectionError) as e:
                    return await self._on_ssh_fail(
                        function, args, kwargs, f"persistent worker failed: {e}"
                    )
            if not self.persistent_workers:
                with timer.phase("stage"):
                    paths = self._write_function_files(
                        operation_id, function, args, kwargs, current_remote_workdir, gpu_lib
                    )

            if not self.persistent_workers and self.batch_roundtrips:
                try:
                    with timer.phase("dispatch"):
                        proc, have_result, result_sha, meta_bytes = (
                            await self._dispatch_fused(
                                transport, paths, env, operation_id
                            )
                        )
                except asyncio.TimeoutError:
                    self._cleanup_local(paths)
                    raise SSHTaskError(
                        f"task {operation_id} exceeded task_timeout="
                        f"{self.task_timeout}s"
                    )
                except (TransportConnectError, OSError) as e:
                    self._cleanup_local(paths)
                    if operation_id in self._cancelled:
                        self._cancelled.discard(operation_id)
                        raise SSHTaskError(f"task {operation_id} was cancelled")
                    return await self._on_ssh_fail(
                        function, args, kwargs,
                        f"transport failed during task {operation_id}: {e}",
                    )
                if operation_id in self._cancelled:
                    self._cancelled.discard(operation_id)
                    self._cleanup_local(paths)
                    raise SSHTaskError(f"task {operation_id} was cancelled")
                if proc.returncode != 0 or not have_result:
                    message = (
                        f"remote task {operation_id} failed "
                        f"(rc={proc.returncode}): {proc.text_err().strip()}"
                    )
                    self._cleanup_local(paths)
                    return await self._on_ssh_fail(function, args, kwargs, message)
                with timer.phase("fetch"):
                    if meta_bytes:
                        record.load_meta(meta_bytes)
                    expected = (record.remote_meta or {}).get("result_sha256")
                    if expected and result_sha != expected:
                        self._cleanup_local(paths)
                        return await self._on_ssh_fail(
                            function, args, kwargs,
                            f"result stream for {operation_id} failed its "
                            f"integrity check ({result_sha[:12]} != {expected[:12]})",
                        )
                    # the streamed result file IS the local result file;
                    # unpickle straight from disk (one in-RAM copy: the
                    # deserialized object itself)
                    with open(paths["result_local"], "rb") as f_res:
                        result, exception = stdlib_pickle.load(f_res)
            elif not self.persistent_workers:
                # Template path: discrete upload/submit/poll/fetch/cleanup
                # round trips (reference §3.1 flow).
                with timer.phase("upload"):
                    await self._upload_task(
                        transport,
                        [
                            (paths["function_local"], paths["function_remote"]),
                            (paths["script_local"], paths["script_remote"]),
                        ],
                    )
                with timer.phase("dispatch"):
                    proc = await self.submit_task(
                        transport, paths["script_remote"], env=env,
                        operation_id=operation_id,
                    )
                if operation_id in self._cancelled:
                    self._cancelled.discard(operation_id)
                    self._cleanup_local(paths)
                    raise SSHTaskError(f"task {operation_id} was cancelled")
                if proc.returncode != 0:
                    self._cleanup_local(paths)
                    return await self._on_ssh_fail(
                        function,
                        args,
                        kwargs,
                        f"remote task {operation_id} failed "
                        f"(rc={proc.returncode}): {proc.text_err().strip()}",
                    )
                with timer.phase("poll"):
                    ready = await self._poll_task(transport, paths["result_remote"])
                if not ready:
                    self._cleanup_local(paths)
                    return await self._on_ssh_fail(
                        function, args, kwargs, f"result for {operation_id} never appeared"
                    )
                with timer.phase("fetch"):
                    result, exception = await self.query_result(
                        transport, paths["result_remote"], paths["result_local"]
                    )
                    try:
                        await transport.get_file(paths["meta_remote"], paths["meta_local"])
                        record.load_meta_file(paths["meta_local"])
                    except Exception:
                        pass
                if self.do_cleanup:
                    with timer.phase("cleanup"):
                        await transport.run(
                            "rm -f "
                            + " ".join(
                                shlex.quote(paths[k])
                                for k in (
                                    "function_remote",
                                    "script_remote",
                                    "result_remote",
                                    "meta_remote",
                                )
                            )
                        )
        finally:
            if slot is not None:
                await slot.release()

        if self.do_cleanup and paths is not None:
            self._cleanup_local(paths)

        record.phases = timer.snapshot()
        record.total_s = timer.total()
        self.counters["tasks"] += 1
        if exception is not None:
            self.counters["task_exceptions"] += 1
        self.last_task_record = record
        self.task_records.append(record)
        log_path = os.environ.get("CSP_AMD_TASK_LOG")
        if log_path:
            # structured per-task trace (SURVEY.md §5 tracing row)
            try:
                with open(log_path, "a") as f:
                    f.write(record.to_json() + "\n")
            except OSError:
                app_log.debug("task log write failed", exc_info=True)
        if len(self.task_records) > 10000:
            del self.task_records[: len(self.task_records) // 2]

        if exception is not None:
            raise exception
        return result

    def _cleanup_local(self, paths: Dict[str, str]) -> None:
        for key in ("function_local", "script_local", "result_local", "meta_local"):
            try:
                os.remove(paths[key])
            except OSError:
                pass

    async def prewarm(self, slots: Optional[int] = None) -> int:
        """Spin up transports, env checks and persistent workers (with
        their GPU prologue) ahead of the first electron, so first-task
        latency matches steady state.  Returns the number of workers
        started.  No-op unless ``persistent_workers`` is enabled."""
        await self._validate_credentials()
        transport = await self._client_connect()
        if transport is None:
            raise RuntimeError(f"could not connect to {self.hostname}")
        gpu_lib, has_gpu = await self._ensure_environment(transport)
        if not self.persistent_workers:
            return 0
        script_remote = await self._provision_worker_script(transport, gpu_lib)
        cmd = self._wrap_conda(f"{self.python_path} {shlex.quote(script_remote)}")
        if self.hip_visible_devices_policy == "roundrobin" and has_gpu:
            n_gpus = slots if slots is not None else self.gpu_slots
            tags_envs = []
            for gpu in range(n_gpus):
                if self.slots_per_gpu == 1:
                    tags_envs.append((gpu, {"CSP_GPU_SLOT": str(gpu)}))
                else:
                    # oversubscription: one warm worker per (gpu, sub-slot)
                    for sub in range(self.slots_per_gpu):
                        tags_envs.append(((gpu, sub), {"CSP_GPU_SLOT": str(gpu)}))
        elif self.hip_visible_devices_policy == "fixed" and has_gpu:
            tags_envs = [(self.fixed_gpu, {"CSP_GPU_SLOT": str(self.fixed_gpu)})]
        else:
            tags_envs = [
                (f"cpu{i}", None)
                for i in range(slots if slots is not None else self.cpu_workers)
            ]

        async def start(tag, env):
            key = (self._pool_key(), tag, script_remote)

            async def launcher():
                return await transport.open_channel(cmd, env=env)

            await worker_pool.get_worker(key, launcher)

        await asyncio.gather(*[start(t, e) for t, e in tags_envs])
        return len(tags_envs)

    def stats(self) -> dict:
        """Latency percentiles + per-phase means over this executor's
        completed tasks (observability; SURVEY.md §5 metrics row)."""
        from .utils.timing import summarize

        out = summarize(self.task_records)
        out["counters"] = dict(self.counters)
        return out

    # Convenience for closing pooled transports (e.g. at interpreter exit
    # or between tests).  The reference closes per-task; pooled transports
    # outlive tasks by design.
    @staticmethod
    async def close_pool() -> None:
        await worker_pool.close_all()
        await transport_pool.close_all()
