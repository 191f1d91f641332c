"""``device_tensor_args`` against a worker that cannot take device
arguments: the electron fails with the documented RuntimeError, and the
argument frame has still been taken off the channel, so the same worker
serves the next electron.

The dispatcher here has no built GPU library to ship (patched away), so the
worker has none whether or not the host has a GPU: without a GPU it reports
that it sees none, with one that the library was not provisioned.  Both are
the same documented error and the same drain path."""

import asyncio

import pytest

torch = pytest.importorskip("torch")


def test_failed_device_argument_is_drained(local_executor, monkeypatch):
    from covalent_ssh_plugin_amd.gpu import probe

    monkeypatch.setattr(probe, "local_gpu_lib_path", lambda: "")
    ex = local_executor(persistent_workers=True, device_tensor_args=True, cpu_workers=1)

    def takes_tensor(t):
        return float(t.sum())  # must never run

    def plain(x):
        import os

        return x + 1, os.getpid()

    big = torch.arange(300 * 1024 // 4, dtype=torch.float32)  # 300 KiB

    async def main():
        # a first plain electron tells us the worker's pid
        _, pid0 = await ex.execute(plain, [0], {}, dispatch_id="d", node_id=0)
        with pytest.raises(RuntimeError, match="need a GPU worker with the CDNA4 library"):
            await ex.execute(takes_tensor, [big], {}, dispatch_id="d", node_id=1)
        failed_meta = ex.last_task_record.remote_meta
        value, pid1 = await ex.execute(plain, [41], {}, dispatch_id="d", node_id=2)
        served = ex.last_task_record.remote_meta["served"]
        await ex.close_pool()
        return pid0, failed_meta, value, pid1, served

    pid0, failed_meta, value, pid1, served = asyncio.run(main())
    assert value == 42
    assert pid1 == pid0 == failed_meta["pid"], "the worker was replaced"
    assert served == 3
    assert failed_meta["arg_staging"]["mode"] == "none"
    assert failed_meta["arg_staging"]["verified"] == 0
    assert "user_fn" not in failed_meta["phases_ms"]
