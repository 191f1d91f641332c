"""Pooled SSH transport over the OpenSSH client with ControlMaster
multiplexing.

Design (vs the reference, /root/reference/covalent_ssh_plugin/ssh.py):

* The reference opens ONE FRESH asyncssh connection per task (ssh.py:497)
  and closes it at the end (ssh.py:585-587) — every electron pays a full
  TCP+SSH handshake plus ~10-11 sequential round trips.
* This transport establishes one OpenSSH **ControlMaster** per
  (hostname, username, key) and multiplexes every subsequent command and
  file transfer over it (``-o ControlMaster=auto -o ControlPath=…``):
  per-task cost drops to command round trips only, with no re-handshake,
  and many concurrent tasks share the one TCP connection.
* File staging is batched: a single ``ssh host 'mkdir -p … && tar -xf -'``
  with the files streamed as an in-memory tar on stdin replaces the
  reference's two scp sessions + mkdir (3 round trips → 1).

Host-key policy matches the reference (``known_hosts=None``, ssh.py:267):
``StrictHostKeyChecking=no`` with a throwaway known-hosts file.
"""

from __future__ import annotations

import asyncio
import hashlib
import os
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

from .base import (
    CompletedCommand,
    Transport,
    TransportConnectError,
    make_tar_stream,
)

# Exit code the ssh client itself uses for connection/usage failure.  A
# remote command's own exit status passes through < 255.
_SSH_CLIENT_ERR = 255


class OpenSSHTransport(Transport):
    def __init__(
        self,
        hostname: str,
        username: str = "",
        ssh_key_file: str = "",
        port: int = 22,
        control_dir: Optional[str] = None,
        control_persist: str = "300",
        connect_timeout: float = 20.0,
        extra_options: Optional[List[str]] = None,
    ):
        self.hostname = hostname
        self.username = username
        self.ssh_key_file = ssh_key_file
        self.port = port
        self.connect_timeout = connect_timeout
        self.control_persist = control_persist
        self.extra_options = list(extra_options or [])
        self._connected = False

        cdir = Path(control_dir or os.path.join(os.path.expanduser("~"), ".cache", "covalent-ssh-amd"))
        cdir.mkdir(parents=True, exist_ok=True)
        key = f"{username}@{hostname}:{port}:{ssh_key_file}".encode()
        digest = hashlib.sha256(key).hexdigest()[:16]
        self._control_path = str(cdir / f"cm-{digest}")
        self.endpoint = f"{username}@{hostname}" if username else hostname

    # ------------------------------------------------------------------
    def _base_args(self) -> List[str]:
        args = [
            "ssh",
            "-o", "ControlMaster=auto",
            "-o", f"ControlPath={self._control_path}",
            "-o", f"ControlPersist={self.control_persist}",
            "-o", "StrictHostKeyChecking=no",
            "-o", "UserKnownHostsFile=/dev/null",
            "-o", "LogLevel=ERROR",
            "-o", "BatchMode=yes",
            "-o", f"ConnectTimeout={int(self.connect_timeout)}",
            "-p", str(self.port),
        ]
        if self.ssh_key_file:
            args += ["-i", self.ssh_key_file]
        if self.username:
            args += ["-l", self.username]
        args += self.extra_options
        return args

    async def _ssh_exec(
        self,
        command: str,
        input_data: Optional[bytes] = None,
        timeout: Optional[float] = None,
    ) -> CompletedCommand:
        argv = self._base_args() + [self.hostname, "--", command]
        proc = await asyncio.create_subprocess_exec(
            *argv,
            stdin=asyncio.subprocess.PIPE if input_data is not None else asyncio.subprocess.DEVNULL,
            stdout=asyncio.subprocess.PIPE,
            stderr=asyncio.subprocess.PIPE,
        )
        try:
            stdout, stderr = await asyncio.wait_for(
                proc.communicate(input=input_data), timeout=timeout
            )
        except asyncio.TimeoutError:
            proc.kill()
            await proc.wait()
            raise
        return CompletedCommand(proc.returncode, stdout, stderr)

    # ------------------------------------------------------------------
    async def connect(self) -> None:
        """Establish (or verify) the ControlMaster.  Idempotent and cheap
        when the master is already up (multiplexed ``true``)."""
        result = await self._ssh_exec("true", timeout=self.connect_timeout + 10)
        if result.returncode == _SSH_CLIENT_ERR or (
            result.returncode != 0 and not self._connected
        ):
            raise TransportConnectError(
                f"ssh connect to {self.endpoint} failed "
                f"(rc={result.returncode}): {result.text_err().strip()}"
            )
        self._connected = True

    @property
    def is_connected(self) -> bool:
        return self._connected

    async def run(
        self,
        command: str,
        *,
        input_data: Optional[bytes] = None,
        env: Optional[dict] = None,
        timeout: Optional[float] = None,
    ) -> CompletedCommand:
        if not self._connected:
            raise TransportConnectError("transport not connected")
        result = await self._ssh_exec(
            self._env_prefix(env) + command, input_data=input_data, timeout=timeout
        )
        if result.returncode == _SSH_CLIENT_ERR:
            # The ssh client (not the remote command) failed — connection
            # dropped under us.  Surface as a connect error so the pool /
            # retry policy can act.
            self._connected = False
            raise TransportConnectError(
                f"ssh channel to {self.endpoint} failed: {result.text_err().strip()}"
            )
        return result

    async def put_files(self, files: Sequence[Tuple[str, str]]) -> None:
        if not files:
            return
        tar_bytes, base = make_tar_stream(files)
        cmd = f"tar -xf - -C /" if base == "/" else "tar -xf -"
        result = await self.run(cmd, input_data=tar_bytes)
        if not result.ok:
            raise TransportConnectError(
                f"file upload to {self.endpoint} failed: {result.text_err().strip()}"
            )

    async def get_file(self, remote_path: str, local_path: str) -> None:
        """Stream the remote file to disk in chunks — a multi-GiB result
        fetched over the discrete template path must not hold a full
        in-RAM copy (matches the fused path's streaming)."""
        import shlex

        Path(local_path).parent.mkdir(parents=True, exist_ok=True)
        proc = await self.open_pipe(f"cat -- {shlex.quote(remote_path)}")
        proc.stdin.close()
        stderr_acc = bytearray()

        async def drain_stderr():
            while True:
                chunk = await proc.stderr.read(1 << 20)
                if not chunk:
                    break
                if len(stderr_acc) < (1 << 16):
                    stderr_acc.extend(chunk)

        err_task = asyncio.ensure_future(drain_stderr())
        try:
            with open(local_path, "wb") as f:
                while True:
                    chunk = await proc.stdout.read(1 << 20)
                    if not chunk:
                        break
                    await asyncio.to_thread(f.write, chunk)
        finally:
            await err_task
        rc = await proc.wait()
        if rc != 0:
            try:
                os.remove(local_path)
            except OSError:
                pass
            err = bytes(stderr_acc).decode(errors="replace").strip()
            if rc == _SSH_CLIENT_ERR:
                self._connected = False
                raise TransportConnectError(
                    f"ssh channel to {self.endpoint} failed: {err}"
                )
            raise FileNotFoundError(f"{self.endpoint}:{remote_path}: {err}")

    async def open_channel(self, command: str, env: Optional[dict] = None):
        from .channel import spawn_channel_process

        argv = self._base_args() + [self.hostname, "--", self._env_prefix(env) + command]
        return await spawn_channel_process(argv, label=f"worker@{self.endpoint}")

    async def open_pipe(self, command: str, env: Optional[dict] = None):
        argv = self._base_args() + [self.hostname, "--", self._env_prefix(env) + command]
        return await asyncio.create_subprocess_exec(
            *argv,
            stdin=asyncio.subprocess.PIPE,
            stdout=asyncio.subprocess.PIPE,
            stderr=asyncio.subprocess.PIPE,
            limit=4 * 1024 * 1024,
        )

    async def close(self) -> None:
        if not self._connected:
            return
        # Ask the master to exit; ignore failures (it may have timed out).
        argv = self._base_args() + ["-O", "exit", self.hostname]
        proc = await asyncio.create_subprocess_exec(
            *argv,
            stdout=asyncio.subprocess.DEVNULL,
            stderr=asyncio.subprocess.DEVNULL,
        )
        await proc.wait()
        self._connected = False
