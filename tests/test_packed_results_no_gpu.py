"""``pack_tensor_results`` without a GPU: the two options and their
validation, the dispatcher's rebuild of a packed buffer into views, its
integrity check of result buffers that carry a checksum, a CPU-only worker
with the option on, and the rendered worker text."""

import asyncio

import cloudpickle
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.remote import workers  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402

PACKED = "__csp_packed_tensor_v1__"
PLAIN = "__csp_tensor_buffer_v1__"


# -- configuration -----------------------------------------------------------


def test_defaults():
    from covalent_ssh_plugin_amd.ssh import _EXECUTOR_PLUGIN_DEFAULTS

    assert _EXECUTOR_PLUGIN_DEFAULTS["pack_tensor_results"] is False
    assert _EXECUTOR_PLUGIN_DEFAULTS["pack_results_min_bytes"] == 65536


def test_option_needs_a_worker_mode(local_executor):
    with pytest.raises(ValueError, match="pack_tensor_results"):
        local_executor(pack_tensor_results=True)
    ex = local_executor()
    assert ex.pack_tensor_results is False
    assert ex.pack_results_min_bytes == 65536


def test_option_accepted_with_either_worker_mode(local_executor):
    ex = local_executor(pack_tensor_results=True, persistent_workers=True)
    assert ex.pack_tensor_results is True
    ex = local_executor(
        pack_tensor_results=True, isolate_tasks=True, pack_results_min_bytes=0
    )
    assert ex.pack_tensor_results is True
    assert ex.pack_results_min_bytes == 0


def test_cluster_passes_both_options_through(tmp_path):
    from covalent_ssh_plugin_amd.cluster import SSHClusterExecutor

    common = dict(transport="local", local_home=str(tmp_path), cache_dir=str(tmp_path / "c"))
    cluster = SSHClusterExecutor(
        ["node-a", "node-b"], persistent_workers=True, pack_tensor_results=True,
        pack_results_min_bytes=4096, **common,
    )
    for ex in cluster.executors:
        assert ex.pack_tensor_results is True
        assert ex.pack_results_min_bytes == 4096
    with pytest.raises(ValueError, match="pack_tensor_results"):
        SSHClusterExecutor(["node-a"], pack_tensor_results=True, **common)


# -- _reconstruct on a hand-built packed reply -------------------------------


def _seeded():
    gen = torch.Generator().manual_seed(7)
    return [
        torch.randn(5, 3, generator=gen),  # 60 bytes: 4 bytes of padding follow
        torch.randn(33, generator=gen).to(torch.bfloat16),  # 66 bytes
        torch.randint(-(1 << 40), 1 << 40, (2, 2, 2), generator=gen),  # int64
        torch.rand(21, generator=gen) > 0.5,  # bool, 21 bytes
        torch.empty(0, 7),
        torch.tensor(3.25, dtype=torch.float64),  # 0-dim
    ]


def _arena(tensors, destination):
    """Lay ``tensors`` out under the 16-byte rule into ``destination(total)``
    and return (buffer, meta entry)."""
    entries = []
    total = 0
    for t in tensors:
        n = t.numel() * t.element_size()
        entries.append({
            "dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
            "offset": total, "nbytes": n,
        })
        total += (n + 15) // 16 * 16
    buf = destination(total)
    view = memoryview(buf).cast("B")
    view[:] = b"\0" * total
    for t, e in zip(tensors, entries):
        if e["nbytes"]:
            raw = t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
            view[e["offset"] : e["offset"] + e["nbytes"]] = raw
    return buf, {"packed": entries, "nbytes": total}


def _native_destination(total):
    buf = native_io.alloc_buffer(total)
    assert buf is not None, "libcsp_io.so was not built"
    return buf


@pytest.mark.parametrize("destination", [bytearray, _native_destination, bytes])
def test_reconstruct_packed_views(destination):
    tensors = _seeded()
    if destination is bytes:  # a frame below the large-frame threshold
        buf, info = _arena(tensors, bytearray)
        buf = bytes(buf)
    else:
        buf, info = _arena(tensors, destination)
    plain = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    plain_raw = bytearray(plain.numpy().tobytes())
    buffer_meta = [info, {"dtype": "int32", "shape": [3, 4]}]
    Pair = __import__("collections").namedtuple("Pair", "first second")
    shipped = {
        "list": [(PACKED, 0, j) for j in range(len(tensors))],
        "again": (PACKED, 0, 0),
        "pair": Pair((PACKED, 0, 1), (PLAIN, 1)),
        "n": 5,
    }
    out = workers._reconstruct(shipped, buffer_meta, [buf, plain_raw])
    assert out["n"] == 5
    for got, want in zip(out["list"], tensors):
        assert got.dtype == want.dtype
        assert got.shape == want.shape
        assert torch.equal(got, want)
    assert out["again"] is out["list"][0], "a tensor placed twice came back as two"
    assert isinstance(out["pair"], Pair)
    assert torch.equal(out["pair"].first, tensors[1])
    assert torch.equal(out["pair"].second, plain)
    # the views do not overlap: writing through one changes no other
    out["list"][0].fill_(-1.0)
    out["list"][3].fill_(True)
    assert torch.equal(out["list"][1], tensors[1])
    assert torch.equal(out["list"][2], tensors[2])
    assert torch.equal(out["list"][5], tensors[5])
    assert torch.equal(out["pair"].second, plain)
    if destination is not bytes:
        # zero-copy: the views are windows on the received buffer itself
        assert bytes(memoryview(buf).cast("B")[:4]) == torch.tensor(-1.0).numpy().tobytes()


# -- integrity check in run_task ---------------------------------------------


class _FakeChannel:
    """Replays a worker's reply: the ack, R1, then the raw buffers."""

    def __init__(self, main, extras):
        self.main = main
        self.extras = extras

    async def exchange(self, frames, reply_frames, timeout=None):
        assert reply_frames(cloudpickle.dumps(("A1", "op"))) is None
        assert reply_frames(self.main) == len(self.extras)
        return self.main, self.extras


def _reply(sum_of, tamper=False):
    tensors = _seeded()
    buf, info = _arena(tensors, bytearray)
    sums = sum_of(buf)
    info["sum"] = [int(sums[0]), int(sums[1])]
    if tamper:
        buf[20] ^= 0x01
    result = [(PACKED, 0, j) for j in range(len(tensors))]
    meta = {"buffers": [info], "phases_ms": {}}
    main = cloudpickle.dumps(("R1", cloudpickle.dumps((result, None)), meta, 1))
    handle = workers.WorkerHandle(channel=_FakeChannel(main, [buf]), startup_meta={}, key=("k",))
    return handle, tensors


def _run(handle):
    return asyncio.run(workers.run_task(handle, "op", ".", b""))


def test_matching_sum_passes_and_is_counted():
    assert native_io.load() is not None, "libcsp_io.so was not built"
    handle, tensors = _reply(native_io.checksum)
    result, exception, meta = _run(handle)
    assert exception is None
    assert meta["result_integrity"] == {"verified": 1}
    for got, want in zip(result, tensors):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want)


def test_changed_byte_fails_integrity():
    assert native_io.load() is not None, "libcsp_io.so was not built"
    handle, _ = _reply(native_io.checksum, tamper=True)
    with pytest.raises(RuntimeError, match="integrity") as failure:
        _run(handle)
    assert "result buffer 0" in str(failure.value)


def test_wrong_sum_fails_integrity():
    assert native_io.load() is not None, "libcsp_io.so was not built"

    def off_by_one(buf):
        s0, s1 = native_io.checksum(buf)
        return s0, (s1 + 1) % (1 << 64)

    handle, _ = _reply(off_by_one)
    with pytest.raises(RuntimeError, match="integrity"):
        _run(handle)


def test_check_skipped_without_the_library(monkeypatch):
    assert native_io.load() is not None, "libcsp_io.so was not built"
    handle, tensors = _reply(native_io.checksum, tamper=True)
    monkeypatch.setattr(native_io, "checksum", lambda *a, **k: None)
    result, exception, meta = _run(handle)
    assert exception is None
    assert meta["result_integrity"] == {"verified": 0}
    assert len(result) == len(tensors)


# -- a CPU-only worker with the option on ------------------------------------


def test_cpu_worker_with_option_on(local_executor):
    ex = local_executor(
        persistent_workers=True, pack_tensor_results=True, pack_results_min_bytes=0,
        cpu_workers=1, hip_visible_devices_policy="none",
    )

    def electron(seed):
        import torch

        gen = torch.Generator().manual_seed(seed)
        return {"w": torch.randn(64, 3, generator=gen), "b": [torch.arange(5)]}

    async def main():
        out = await ex.execute(electron, [3], {}, dispatch_id="p", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    out, meta = asyncio.run(main())
    gen = torch.Generator().manual_seed(3)
    assert torch.equal(out["w"], torch.randn(64, 3, generator=gen))
    assert torch.equal(out["b"][0], torch.arange(5))
    assert all("packed" not in info for info in meta["buffers"])
    assert meta["staging"]["packed_tensors"] == 0
    assert meta["staging"]["packed_bytes"] == 0
    assert "result_integrity" not in meta


# -- the rendered worker -----------------------------------------------------


def test_rendered_worker_has_no_token_left():
    from covalent_ssh_plugin_amd.remote.stub import render_worker

    text = render_worker(pack_results=True, pack_min_bytes=12345)
    assert "__CSP_" not in text
    compile(text, "worker.py", "exec")
    assert "PACK_RESULTS = bool(True)" in text
    assert "PACK_MIN_BYTES = int(12345)" in text
    off = render_worker()
    assert "__CSP_" not in off
    assert "PACK_RESULTS = bool(False)" in off
