"""MI355X tests for packed tensor results: csp_pack_dev on its own (every
size class at every source alignment, zero padding, guard bytes, the
per-block tile loop, refused layouts) and ``pack_tensor_results`` end to end
through persistent and fork-isolated workers, the integrity failure
included."""

import asyncio
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
OFFSETS = [0, 1, 2, 4, 8]  # source start, from a 16-byte aligned base
GRID_CAP = 2048  # blocks of the pack kernel; more tiles than this loop


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


def _sizes(tile):
    return [0, 1, 15, 16, 17, 4095, tile, tile + 1, 3 * tile + 5, (1 << 20) + 3]


@pytest.fixture(scope="module")
def cases(probe):
    """Every size at every source offset, as (start, nbytes) slices of one
    seeded random device tensor that is shared and never written to.  Each
    source starts ``offset`` bytes after a 16-byte boundary."""
    tile = probe.pack_tile_bytes()
    spans = []
    cursor = 0
    for nbytes in _sizes(tile):
        for offset in OFFSETS:
            start = (cursor + 15) // 16 * 16 + offset
            spans.append((start, nbytes))
            cursor = start + nbytes
    gen = torch.Generator().manual_seed(20241021)
    host = torch.randint(0, 256, (cursor,), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return dev, host.numpy(), spans


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


def _expected(host, spans, offsets, total):
    """The arena assembled on the host from the same layout rule; bytes no
    segment owns are zero."""
    want = np.zeros(total, dtype=np.uint8)
    for (start, nbytes), off in zip(spans, offsets):
        want[off : off + nbytes] = host[start : start + nbytes]
    return want


def _pack_and_check(probe, dev, host, spans):
    """Pack ``spans`` of ``dev`` into an arena inside a larger 0xA5-filled
    tensor and assert: byte-equal to the host's arena (which has every
    padding byte zero), and the guard bytes untouched.  Returns the arena."""
    offsets, total = probe.pack_layout([n for _, n in spans])
    assert all(off % 16 == 0 for off in offsets) and total % 16 == 0
    outer = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert outer.data_ptr() % 16 == 0
    segments = [
        (dev.data_ptr() + start, off, nbytes)
        for (start, nbytes), off in zip(spans, offsets)
    ]
    report = probe.pack_device(segments, outer.data_ptr(), total)
    assert report["kernel_ms"] >= 0.0
    got = outer.cpu().numpy()
    want = _expected(host, spans, offsets, total)
    assert np.array_equal(got[:total], want), "arena differs from the host's"
    for (_, nbytes), off in zip(spans, offsets):
        pad_end = off + (nbytes + 15) // 16 * 16
        assert not got[off + nbytes : pad_end].any(), "padding is not zero"
    assert (got[total:] == FILL).all(), "wrote past the arena"
    return outer[:total], want


# -- csp_pack_dev ------------------------------------------------------------


def test_tile_size_is_whole_vectors(probe):
    tile = probe.pack_tile_bytes()
    assert tile > 0 and tile % (256 * 16) == 0


def test_every_size_at_every_offset_in_one_call(probe, cases):
    dev, host, spans = cases
    for (start, _), offset in zip(spans, OFFSETS * (len(spans) // len(OFFSETS))):
        assert (dev.data_ptr() + start) % 16 == offset
    _pack_and_check(probe, dev, host, spans)


def test_every_size_at_every_offset_alone(probe, cases):
    dev, host, spans = cases
    for span in spans:
        _pack_and_check(probe, dev, host, [span])


def test_more_tiles_than_blocks(probe, cases):
    dev, host, _ = cases
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 5001, size=3000).tolist()
    assert sum(1 for n in sizes if n) > GRID_CAP  # one tile each: a second trip
    spans = []
    cursor = 0
    for nbytes in sizes:  # back to back: the sources land on every alignment
        if cursor + nbytes > len(host):
            cursor = 0  # sources may share bytes, nothing writes to them
        spans.append((cursor, nbytes))
        cursor += nbytes
    assert len({start % 16 for start, _ in spans}) == 16
    arena, want = _pack_and_check(probe, dev, host, spans)
    assert probe.checksum_device(arena.data_ptr(), arena.numel()) == reference(want.tobytes())


def test_bad_layouts_are_refused(probe, cases):
    dev, host, _ = cases
    spans = [(0, 100), (128, 33), (256, 4096)]
    offsets, total = probe.pack_layout([n for _, n in spans])
    assert offsets == [0, 112, 160] and total == 160 + 4096
    outer = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def segments(offs):
        return [(dev.data_ptr() + s, o, n) for (s, n), o in zip(spans, offs)]

    with pytest.raises(probe.GpuLibError, match="layout rule"):
        probe.pack_device(segments([0, 100, 160]), outer.data_ptr(), total)
    with pytest.raises(probe.GpuLibError, match="layout rule"):
        probe.pack_device(segments([16, 128, 176]), outer.data_ptr(), total + 16)
    with pytest.raises(probe.GpuLibError, match="arena_bytes"):
        probe.pack_device(segments(offsets), outer.data_ptr(), total + 16)
    with pytest.raises(probe.GpuLibError, match="16-byte aligned"):
        probe.pack_device(segments(offsets), outer.data_ptr() + 4, total)
    torch.cuda.synchronize()
    assert (outer.cpu().numpy() == FILL).all(), "a refused call launched something"
    # the library is fine
    _pack_and_check(probe, dev, host, spans)


# -- end to end --------------------------------------------------------------

THRESHOLD = 1 << 20
BIG_ELEMS = THRESHOLD // 4 + 100  # fp32: just above the threshold


def _make_electron():
    """Local functions, so cloudpickle ships them (and the namedtuple
    class) by value."""

    def build(seed, device):
        """The result, seeded on the CPU; ``device`` is where the electron
        moves it.  With "cpu" it is what the dispatcher expects back."""
        import collections

        import torch

        gen = torch.Generator().manual_seed(seed)

        def rn(*shape):
            return torch.randn(*shape, generator=gen)

        def ri(hi, shape, dtype):
            return torch.randint(0, hi, shape, generator=gen).to(dtype)

        Head = collections.namedtuple("Head", "weight bias scale")
        state = {}
        for i in range(12):
            state["layer%d.weight" % i] = rn(17 + i, 33).to(device)
            state["layer%d.bias" % i] = rn(17 + i).to(device)
        for i in range(3):  # together above the large-frame threshold
            state["embed%d" % i] = rn(131072 + 3 * i).to(device)
        shared = rn(5, 5).to(device)
        bf16_base = rn(1001).to(torch.bfloat16).to(device)
        u8_base = ri(256, (777,), torch.uint8).to(device)
        return {
            "state": state,
            "misc": [
                rn(1000).to(torch.bfloat16).to(device),
                rn(333).to(torch.float16).to(device),
                ri(1 << 40, (3, 7), torch.int64).to(device),
                ri(256, (4099,), torch.uint8).to(device),
                (rn(21) > 0).to(device),
                torch.complex(rn(9, 2), rn(9, 2)).to(device),
                torch.tensor(2.5).to(device),  # 0-dim
                torch.empty(0, 7).to(device),
                rn(30, 50).to(device).t(),  # not contiguous
                bf16_base[1:],  # source 2 bytes past an aligned base
                u8_base[3:],  # source 3 bytes past an aligned base
                shared,
            ],
            "head": Head(rn(64, 10).to(device), rn(10).to(device), shared),
            "big": rn(BIG_ELEMS).to(device),  # own streamed frame
            "cpu_small": rn(50),  # stays where it is
            "seed": seed,
        }

    def electron(seed):
        import os

        import torch

        out = build(seed, "cuda")
        assert out["misc"][9].data_ptr() % 16 == 2
        assert out["misc"][10].data_ptr() % 16 == 3
        assert not out["cpu_small"].is_cuda
        torch.cuda.synchronize()
        return out, os.getpid()

    return build, electron


_build, _electron = _make_electron()


def _flatten(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in _flatten(v)]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in _flatten(v)]
    return []


def _assert_same(out, want):
    assert set(out) == set(want)
    assert out["seed"] == want["seed"]
    assert set(out["state"]) == set(want["state"])
    assert type(out["head"]).__name__ == "Head" and out["head"]._fields == want["head"]._fields
    assert isinstance(out["misc"], list) and len(out["misc"]) == len(want["misc"])
    got_flat, want_flat = _flatten(out), _flatten(want)
    assert len(got_flat) == len(want_flat) >= 40
    for i, (g, w) in enumerate(zip(got_flat, want_flat)):
        assert not g.is_cuda
        assert g.dtype == w.dtype, i
        assert g.shape == w.shape, i
        assert torch.equal(g, w), i


def _packable(want):
    """(count, bytes) of the distinct tensors the worker should pack."""
    seen = {}
    for t in _flatten(want):
        if t is want["big"] or t is want["cpu_small"]:
            continue
        seen[id(t)] = t.numel() * t.element_size()
    return len(seen), sum(seen.values())


def _make_executor(kind, tmp_path, sshim, monkeypatch, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor
    from covalent_ssh_plugin_amd.transport import native_io
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    monkeypatch.setattr(Channel, "large_frame_threshold", 1 << 20)
    common = dict(
        cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        pack_tensor_results=True,
        pack_results_min_bytes=0,
        # one slot, so every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        pinned_staging_threshold_bytes=THRESHOLD,
    )
    common.update(overrides)
    if kind == "local":
        home = tmp_path / "home"
        home.mkdir()
        return SSHExecutor(transport="local", local_home=str(home), **common)
    monkeypatch.setenv(
        "SSHIM_PASS_ENV",
        "HSA_ENABLE_IPC_MODE_LEGACY,LD_LIBRARY_PATH,HIP_VISIBLE_DEVICES,"
        "ROCR_VISIBLE_DEVICES,PYTORCH_ROCM_ARCH,TMPDIR",
    )
    return SSHExecutor(
        transport="ssh", hostname=sshim.hostname, username="mi355x",
        ssh_key_file=str(sshim.key), **common,
    )


def _assert_packed_meta(meta, want):
    count, nbytes = _packable(want)
    assert "pack_fallback" not in meta["staging"], meta["staging"]
    assert meta["staging"]["packed_tensors"] == count, meta["staging"]
    assert meta["staging"]["packed_bytes"] == nbytes, meta["staging"]
    assert meta["staging"]["mode"] == "pinned"
    # exactly two out-of-band buffers: the arena and the large tensor
    assert len(meta["buffers"]) == 2, meta["buffers"]
    packed = [info for info in meta["buffers"] if "packed" in info]
    assert len(packed) == 1
    entries = packed[0]["packed"]
    assert len(entries) == count
    assert all(e["offset"] % 16 == 0 for e in entries)
    assert sum(e["nbytes"] for e in entries) == nbytes
    assert packed[0]["nbytes"] == sum((e["nbytes"] + 15) // 16 * 16 for e in entries)
    assert meta["staging"]["pinned_tensors"] == 1  # the large one
    assert meta["result_integrity"]["verified"] >= 1


@pytest.mark.parametrize("kind", ["local", "sshim"])
def test_end_to_end_packed_results(kind, tmp_path, sshim, monkeypatch):
    ex = _make_executor(kind, tmp_path, sshim, monkeypatch)

    async def run():
        first = await ex.execute(_electron, [51], {}, dispatch_id="p", node_id=0)
        meta1 = ex.last_task_record.remote_meta
        second = await ex.execute(_electron, [52], {}, dispatch_id="p", node_id=1)
        meta2 = ex.last_task_record.remote_meta
        await ex.close_pool()
        return first, meta1, second, meta2

    first, meta1, second, meta2 = asyncio.run(run())
    for (out, pid), meta, seed in ((first, meta1, 51), (second, meta2, 52)):
        want = _build(seed, "cpu")
        _assert_same(out, want)
        assert out["head"].scale is out["misc"][-1], "a tensor placed twice came back as two"
        _assert_packed_meta(meta, want)
        assert pid == meta["pid"]
    assert meta1["pid"] == meta2["pid"], "second electron ran on another worker"
    assert meta2["served"] == meta1["served"] + 1


def test_integrity_failure_then_same_worker(tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    ex = _make_executor("local", tmp_path, sshim, monkeypatch)
    real = native_io.checksum

    def off_by_one(*args, **kwargs):
        s0, s1 = real(*args, **kwargs)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        (_, pid0) = await ex.execute(_electron, [61], {}, dispatch_id="i", node_id=0)
        meta0 = ex.last_task_record.remote_meta
        with monkeypatch.context() as patch:
            patch.setattr(native_io, "checksum", off_by_one)
            with pytest.raises(RuntimeError, match="integrity") as failure:
                await ex.execute(_electron, [62], {}, dispatch_id="i", node_id=1)
        out, pid2 = await ex.execute(_electron, [63], {}, dispatch_id="i", node_id=2)
        meta2 = ex.last_task_record.remote_meta
        await ex.close_pool()
        return pid0, meta0, str(failure.value), out, pid2, meta2

    pid0, meta0, message, out, pid2, meta2 = asyncio.run(run())
    assert "result buffer" in message, message
    assert pid0 == pid2 == meta0["pid"] == meta2["pid"], "the worker was replaced"
    # the failed electron was served in between
    assert meta2["served"] == meta0["served"] + 2
    want = _build(63, "cpu")
    _assert_same(out, want)
    _assert_packed_meta(meta2, want)


def test_isolated_worker_packs_in_the_child(tmp_path, sshim, monkeypatch):
    ex = _make_executor(
        "local", tmp_path, sshim, monkeypatch,
        persistent_workers=False, isolate_tasks=True, isolate_preload="torch",
    )

    async def run():
        out = await ex.execute(_electron, [71], {}, dispatch_id="z", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    (out, pid), meta = asyncio.run(run())
    want = _build(71, "cpu")
    _assert_same(out, want)
    assert meta["isolated"] is True
    assert meta["pid"] == pid
    _assert_packed_meta(meta, want)


def test_below_min_bytes_nothing_is_packed(tmp_path, sshim, monkeypatch):
    ex = _make_executor(
        "local", tmp_path, sshim, monkeypatch, pack_results_min_bytes=1 << 30
    )

    async def run():
        out = await ex.execute(_electron, [81], {}, dispatch_id="m", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    (out, _pid), meta = asyncio.run(run())
    _assert_same(out, _build(81, "cpu"))
    assert meta["staging"]["packed_tensors"] == 0
    assert meta["staging"]["packed_bytes"] == 0
    assert "pack_fallback" not in meta["staging"]
    assert len(meta["buffers"]) == 1  # the large tensor alone
    assert all("packed" not in info for info in meta["buffers"])


def test_option_off_reply_is_unchanged(tmp_path, sshim, monkeypatch):
    ex = _make_executor("local", tmp_path, sshim, monkeypatch, pack_tensor_results=False)

    async def run():
        out = await ex.execute(_electron, [91], {}, dispatch_id="o", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    (out, _pid), meta = asyncio.run(run())
    _assert_same(out, _build(91, "cpu"))
    assert meta["buffers"] == [{"dtype": "float32", "shape": [BIG_ELEMS]}]
    assert set(meta["staging"]) == {"tensors", "pinned_tensors", "bytes", "mode"}
    assert "result_integrity" not in meta

    def keys(obj):
        if isinstance(obj, dict):
            return set(obj) | {k for v in obj.values() for k in keys(v)}
        if isinstance(obj, (list, tuple)):
            return {k for v in obj for k in keys(v)}
        return set()

    assert "packed" not in keys(meta)
