"""``pack_tensor_args`` without a GPU: the checksum composed from the
segments' own checksums, a ``FrameParts`` through a real channel, what
``extract_arg_buffers`` emits with the option on and off, option validation,
and a packed request against a worker that cannot take device arguments."""

import asyncio
import hashlib
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covalent_ssh_plugin_amd.gpu.probe import pack_layout  # noqa: E402
from covalent_ssh_plugin_amd.ops import build as ops_build  # noqa: E402
from covalent_ssh_plugin_amd.remote import workers as worker_pool  # noqa: E402
from covalent_ssh_plugin_amd.transport import native_io  # noqa: E402
from covalent_ssh_plugin_amd.transport.channel import (  # noqa: E402
    FrameParts,
    open_subprocess_channel,
)

THRESHOLD = 256 * 1024


@pytest.fixture
def io_lib():
    ops_build.build_io(verbose=False)
    assert native_io.load() is not None, "libcsp_io.so did not load"


def reference(data: bytes):
    """(s0, s1) as the protocol defines them: pad to 4 bytes, view as
    little-endian u32, widen to u64, wrapping sums."""
    words = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype="<u4").astype(np.uint64)
    weight = (np.arange(len(words), dtype=np.uint64) % np.uint64(1 << 32)) + np.uint64(1)
    with np.errstate(over="ignore"):
        return (
            int(words.sum(dtype=np.uint64)),
            int((words * weight).sum(dtype=np.uint64)),
        )


def raw(t) -> bytes:
    """The contiguous bytes of a CPU tensor."""
    if t.numel() == 0:
        return b""
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def materialise(blobs):
    """The arena that the layout rule describes, as bytes."""
    offsets, total = pack_layout([len(b) for b in blobs])
    arena = bytearray(total)
    for off, b in zip(offsets, blobs):
        arena[off : off + len(b)] = b
    return bytes(arena), offsets


# -- the composed checksum ----------------------------------------------------


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_composed_checksum_is_the_arena_checksum(io_lib, seed):
    rng = np.random.default_rng(seed)
    sizes = [int(n) for n in rng.integers(0, 70000, 60)]
    sizes[0:8] = [0, 1, 2, 3, 5, 15, 17, 0]
    sizes.append((1 << 20) + 3)
    sizes.append(0)
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    arena, offsets = materialise(blobs)
    sums = [native_io.checksum(b) if b else (0, 0) for b in blobs]
    got = worker_pool.compose_packed_checksum(sums, offsets)
    assert got == tuple(native_io.checksum(arena))
    assert got == reference(arena)


# -- FrameParts through a channel ---------------------------------------------

ECHO_CHILD = r"""
import os, struct, sys
def read_exact(n):
    chunks = []
    while n:
        c = os.read(0, min(n, 1 << 20))
        if not c:
            sys.exit(3)
        chunks.append(c)
        n -= len(c)
    return b"".join(chunks)
def write_all(b):
    view = memoryview(b)
    while view:
        view = view[os.write(1, view):]
while True:
    (n,) = struct.unpack(">Q", read_exact(8))
    if n == 0:
        break
    body = read_exact(n)
    write_all(struct.pack(">Q", n) + body)
"""


def test_frame_parts_arrive_as_one_frame(tmp_path):
    script = tmp_path / "echo.py"
    script.write_text(ECHO_CHILD)
    rng = np.random.default_rng(11)
    # runs of small parts, parts at and above 64 KiB, a run longer than the
    # gather size, empty parts, odd sizes
    sizes = [5, 0, 4095, 65535, 65536, 17, 300000, 1, (1 << 20) + 3] + [40000] * 40 + [7]
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    arena, _offsets = materialise(blobs)
    parts = []
    for b in blobs:
        parts.append(np.frombuffer(b, dtype=np.uint8) if b else b"")
        if len(b) % 16:
            parts.append(bytes(16 - len(b) % 16))
    payload = FrameParts(parts)
    assert payload.nbytes == len(arena)
    assert payload.tobytes() == arena
    writes = list(payload.writes())
    assert b"".join(bytes(w) for w in writes) == arena
    assert len(writes) < len([p for p in parts if len(p)]), "small parts were not gathered"
    assert all(len(w) <= FrameParts.GATHER + FrameParts.SMALL for w in writes if isinstance(w, bytes))

    async def run():
        ch = await open_subprocess_channel([sys.executable, str(script)], "echo")
        try:
            await ch.send_frame(payload)
            await ch.send_frame(b"end")
            first = await ch.recv_frame(timeout=60)
            second = await ch.recv_frame(timeout=60)
        finally:
            await ch.close()
        return bytes(first), bytes(second)

    first, second = asyncio.run(run())
    assert len(first) == len(arena)
    assert hashlib.sha256(first).digest() == hashlib.sha256(arena).digest()
    assert second == b"end"


# -- extract_arg_buffers --------------------------------------------------------


def make_args():
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(1000, generator=gen)  # 4000 bytes
    b = torch.randn(33, 7, generator=gen).to(torch.bfloat16)  # 462 bytes: padded
    c = torch.empty(0, 3)
    d = torch.randn(40, 30, generator=gen).t()  # not contiguous
    e = torch.tensor(7, dtype=torch.int64)
    big = torch.randn(THRESHOLD // 4 + 1, generator=gen)  # above the threshold
    args = [a, {"b": b, "c": c, "again": a}]
    kwargs = {"d": d, "pair": (e, big), "n": 3}
    return args, kwargs, [a, b, c, d, e], big


def test_packed_entry_layout_markers_and_dedup(io_lib):
    args, kwargs, small, big = make_args()
    new_args, new_kwargs, meta, buffers = worker_pool.extract_arg_buffers(
        args, kwargs, THRESHOLD, to_device=True, pack_min_bytes=1024
    )
    assert len(meta) == 2 and len(buffers) == 2
    entry = meta[0]
    sizes = [t.numel() * t.element_size() for t in small]
    offsets, total = pack_layout(sizes)
    assert entry["device"] is True and entry["nbytes"] == total
    assert "cache" not in entry and "dtype" not in entry
    assert entry["packed"] == [
        {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
         "offset": off, "nbytes": n}
        for t, off, n in zip(small, offsets, sizes)
    ]
    # the frame is the materialised arena, the checksum is the arena's
    view, keep = buffers[0]
    assert isinstance(view, FrameParts) and view.nbytes == total
    arena, _ = materialise([raw(t) for t in small])
    assert view.tobytes() == arena
    assert entry["sum"] == list(native_io.checksum(arena))
    assert len(keep) == len(small)
    # markers: one per tensor object, the tensor met twice has one
    marker = lambda j: ("__csp_packed_tensor_v1__", 0, j)  # noqa: E731
    assert new_args == [marker(0), {"b": marker(1), "c": marker(2), "again": marker(0)}]
    assert new_kwargs == {
        "d": marker(3), "pair": (marker(4), ("__csp_tensor_buffer_v1__", 1)), "n": 3,
    }
    # the big tensor travels as without the option
    assert meta[1] == {
        "dtype": "float32", "shape": list(big.shape), "device": True,
        "sum": list(native_io.checksum(big.numpy().tobytes())),
    }
    # the caller's containers were not modified
    assert args[0] is small[0] and kwargs["d"] is small[3]


def _per_tensor(args, kwargs, **options):
    return worker_pool.extract_arg_buffers(args, kwargs, THRESHOLD, to_device=True, **options)


def _same_extraction(got, want):
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert len(got[3]) == len(want[3])
    for (view_a, _ka), (view_b, _kb) in zip(got[3], want[3]):
        assert not isinstance(view_a, FrameParts)
        assert bytes(view_a) == bytes(view_b)


def test_option_off_is_the_per_tensor_extraction(io_lib):
    args, kwargs, small, big = make_args()
    off = _per_tensor(args, kwargs)
    _same_extraction(_per_tensor(args, kwargs, pack_min_bytes=None), off)
    new_args, new_kwargs, meta, buffers = off
    marker = lambda i: ("__csp_tensor_buffer_v1__", i)  # noqa: E731
    # one entry per tensor met, the tensor met twice extracted twice
    assert new_args == [marker(0), {"b": marker(1), "c": marker(2), "again": marker(3)}]
    assert new_kwargs == {"d": marker(4), "pair": (marker(5), marker(6)), "n": 3}
    order = [small[0], small[1], small[2], small[0], small[3], small[4], big]
    assert len(meta) == len(order)
    for info, t in zip(meta, order):
        data = raw(t)
        assert info == {
            "dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
            "device": True, "sum": list(native_io.checksum(data)),
        }
    # without to_device the option changes nothing either
    host = worker_pool.extract_arg_buffers(args, kwargs, THRESHOLD)
    host_packed = worker_pool.extract_arg_buffers(args, kwargs, THRESHOLD, pack_min_bytes=0)
    _same_extraction(host_packed, host)
    assert len(host[2]) == 1


def test_fallbacks_to_the_per_tensor_path(io_lib, monkeypatch):
    args, kwargs, small, big = make_args()
    want = _per_tensor(args, kwargs)
    _, total = pack_layout([t.numel() * t.element_size() for t in small])
    # below pack_args_min_bytes (at it, the tensors are packed)
    _same_extraction(_per_tensor(args, kwargs, pack_min_bytes=total + 1), want)
    assert "packed" in _per_tensor(args, kwargs, pack_min_bytes=total)[2][0]
    # one qualifying tensor, even when it is met twice
    one = [small[0], small[0], big]
    _same_extraction(_per_tensor(one, {}, pack_min_bytes=0), _per_tensor(one, {}))
    # above the cap (patched down): at the cap the tensors are packed
    monkeypatch.setattr(worker_pool, "PACK_ARGS_MAX_BYTES", total - 1)
    _same_extraction(_per_tensor(args, kwargs, pack_min_bytes=0), want)
    monkeypatch.setattr(worker_pool, "PACK_ARGS_MAX_BYTES", total)
    assert "packed" in _per_tensor(args, kwargs, pack_min_bytes=0)[2][0]


def test_cache_key_and_what_stays_out_of_the_arena(io_lib):
    args, kwargs, small, big = make_args()
    _, total = pack_layout([t.numel() * t.element_size() for t in small])
    # a tensor at or above arg_cache_min_bytes keeps its own key and entry
    _a, _k, meta, _b = _per_tensor(args, kwargs, pack_min_bytes=0, cache_min_bytes=4800)
    assert [n["nbytes"] for n in meta[0]["packed"]] == [4000, 462, 0, 8]
    assert meta[0]["nbytes"] == 4480 and "cache" not in meta[0]
    own = [info for info in meta[1:] if info["shape"] == [30, 40]]
    assert len(own) == 1 and "key" in own[0]["cache"]
    # an arena below arg_cache_min_bytes carries no key; at it, a key of keys
    _a, _k, meta, _b = _per_tensor(args, kwargs, pack_min_bytes=0, cache_min_bytes=total + 1)
    assert "packed" in meta[0] and "cache" not in meta[0]
    _a, _k, meta, _b = _per_tensor(args, kwargs, pack_min_bytes=0, cache_min_bytes=total)
    key = meta[0]["cache"]["key"]
    again = _per_tensor(args, kwargs, pack_min_bytes=0, cache_min_bytes=total)[2][0]
    assert again["cache"]["key"] == key and again["sum"] == meta[0]["sum"]
    expect = hashlib.blake2b(b"csp-packed-v1", digest_size=16)
    for t in small:
        data = raw(t)
        expect.update(bytes.fromhex(worker_pool.content_key(data)))
        expect.update(len(data).to_bytes(8, "little"))
    assert key == expect.hexdigest()
    # other bytes, another key
    changed = [small[0] + 1, args[1]]
    other = _per_tensor(changed, kwargs, pack_min_bytes=0, cache_min_bytes=total)[2][0]
    assert other["cache"]["key"] != key


def test_without_the_io_library_there_is_no_sum_and_no_key(monkeypatch):
    monkeypatch.setattr(native_io, "force_absent", True)
    assert native_io.load() is None
    args, kwargs, small, big = make_args()
    _a, _k, meta, _b = _per_tensor(args, kwargs, pack_min_bytes=0, cache_min_bytes=16)
    assert "packed" in meta[0]
    assert "sum" not in meta[0] and "cache" not in meta[0]


# -- options --------------------------------------------------------------------


def test_option_validation(local_executor):
    with pytest.raises(ValueError, match="pack_tensor_args needs device_tensor_args"):
        local_executor(persistent_workers=True, pack_tensor_args=True)
    with pytest.raises(ValueError, match="pack_args_min_bytes must not be negative"):
        local_executor(
            persistent_workers=True, device_tensor_args=True, pack_tensor_args=True,
            pack_args_min_bytes=-1,
        )
    ex = local_executor(persistent_workers=True, device_tensor_args=True)
    assert ex.pack_tensor_args is False and ex.pack_args_min_bytes >= 0
    ex = local_executor(isolate_tasks=True, device_tensor_args=True, pack_tensor_args=True)
    assert ex.pack_tensor_args is True


# -- a worker that cannot take device arguments -----------------------------------


def test_failed_packed_argument_is_drained(local_executor, monkeypatch):
    from covalent_ssh_plugin_amd.gpu import probe

    monkeypatch.setattr(probe, "local_gpu_lib_path", lambda: "")
    ex = local_executor(
        persistent_workers=True, device_tensor_args=True, pack_tensor_args=True,
        pack_args_min_bytes=0, cpu_workers=1,
        # one CPU-tagged worker also on a host that has GPUs
        hip_visible_devices_policy="none",
    )

    def takes_state(state):
        return float(sum(t.sum() for t in state.values()))  # must never run

    def plain(x):
        import os

        return x + 1, os.getpid()

    state = {
        "a": torch.arange(300 * 1024 // 4, dtype=torch.float32),  # 300 KiB
        "b": torch.arange(1001, dtype=torch.float32),
        "c": torch.ones(3, dtype=torch.uint8),
    }

    async def main():
        # a first plain electron tells us the worker's pid
        _, pid0 = await ex.execute(plain, [0], {}, dispatch_id="d", node_id=0)
        with pytest.raises(RuntimeError, match="need a GPU worker with the CDNA4 library"):
            await ex.execute(takes_state, [state], {}, dispatch_id="d", node_id=1)
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
