"""MI355X tests for tensor arguments that land in HBM: csp_h2d_stream_fd on
its own (ring wrap, odd sizes, exact consumption, writer gone mid-frame,
wrong header, drain mode), csp_checksum_dev against the numpy reference,
and ``device_tensor_args`` end to end through persistent and fork-isolated
workers, the integrity failure included."""

import asyncio
import os
import struct
import sys
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CHUNK = 64 * 1024  # tiny, so the two-chunk ring wraps on tiny data
SIZES = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17, 3 * CHUNK]
# the last one is more than one pass of a 1024 x 256-lane grid of 16-byte
# loads (4 MiB), so the single-vector loop takes a second trip; the 4-way
# unrolled loop starts at 12 MiB and is covered by test_gpu_checksum_edges
SUM_SIZES = [0, 1, 3, 4, 15, 16, 17, CHUNK - 1, 256 * 16 * 3 + 5, (4 << 20) + 4096 + 3]
GUARD = 64
MARKER = b"\x5a"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests require a visible MI355X (torch.cuda unavailable)")


@pytest.fixture(scope="module")
def probe():
    from covalent_ssh_plugin_amd.gpu import probe as gpu_probe

    gpu_probe.load()  # GpuLibError if the extension was not built/shipped
    return gpu_probe


@pytest.fixture(scope="module")
def source():
    """Seeded random bytes, on the host and on the GPU, shared by every
    case and never written to."""
    gen = torch.Generator().manual_seed(20241020)
    host = torch.randint(0, 256, (max(SUM_SIZES),), dtype=torch.uint8, generator=gen)
    dev = host.cuda()
    torch.cuda.synchronize()
    return dev, host.numpy().tobytes()


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


def _frame(payload: bytes, announce=None) -> bytes:
    return struct.pack(">Q", len(payload) if announce is None else announce) + payload


def _feed(w, data: bytes):
    """Thread that writes ``data`` to ``w`` and closes it."""

    def run():
        try:
            view = memoryview(data)
            while view:
                view = view[os.write(w, view[: 1 << 16]) :]
        except OSError:
            pass  # the reader left first
        finally:
            os.close(w)

    t = threading.Thread(target=run)
    t.start()
    return t


def _guarded(nbytes):
    dst = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return dst


# -- csp_h2d_stream_fd -------------------------------------------------------


@pytest.mark.parametrize("nbytes", SIZES)
def test_h2d_frame_is_exact(probe, source, nbytes):
    _dev, host = source
    dst = _guarded(nbytes)
    r, w = os.pipe()
    t = _feed(w, _frame(host[:nbytes]) + MARKER)
    try:
        report = probe.stream_fd_to_device(r, dst.data_ptr(), nbytes, CHUNK, 5000)
        after = os.read(r, 16)
    finally:
        os.close(r)  # first: a writer still blocked on a full pipe gets EPIPE
        t.join()
    assert report["rc"] == probe.H2D_OK, report
    got = dst.cpu().numpy().tobytes()
    assert got[:nbytes] == host[:nbytes]
    assert got[nbytes:] == b"\xa5" * GUARD, "wrote past the destination"
    # exactly 8 + nbytes consumed: the marker is the next byte, and the last
    assert after == MARKER


def test_h2d_default_chunk(probe, source):
    _dev, host = source
    n = len(host)
    dst = _guarded(n)
    r, w = os.pipe()
    t = _feed(w, _frame(host))
    try:
        report = probe.stream_fd_to_device(r, dst.data_ptr(), n, 0, 5000)
    finally:
        os.close(r)  # first: a writer still blocked on a full pipe gets EPIPE
        t.join()
    assert report["rc"] == probe.H2D_OK, report
    assert dst.cpu().numpy().tobytes() == host + b"\xa5" * GUARD


def test_writer_gone_mid_frame_then_clean_call(probe, source):
    _dev, host = source
    nbytes = 3 * CHUNK
    dst = _guarded(nbytes)
    r, w = os.pipe()
    t = _feed(w, _frame(host[:CHUNK], announce=nbytes))  # header + one chunk, then EOF
    t0 = time.monotonic()
    try:
        report = probe.stream_fd_to_device(r, dst.data_ptr(), nbytes, CHUNK, 5000)
    finally:
        os.close(r)  # first: a writer still blocked on a full pipe gets EPIPE
        t.join()
    assert time.monotonic() - t0 < 5.0
    assert report["rc"] == probe.H2D_FAILED_STREAM, report
    assert dst.cpu().numpy().tobytes()[nbytes:] == b"\xa5" * GUARD

    n2 = 2 * CHUNK + 17  # the ring went back clean
    dst = _guarded(n2)
    r, w = os.pipe()
    t = _feed(w, _frame(host[:n2]))
    try:
        report = probe.stream_fd_to_device(r, dst.data_ptr(), n2, CHUNK, 5000)
    finally:
        os.close(r)  # first: a writer still blocked on a full pipe gets EPIPE
        t.join()
    assert report["rc"] == probe.H2D_OK, report
    assert dst.cpu().numpy().tobytes()[:n2] == host[:n2]


def test_header_announcing_another_length(probe, source):
    _dev, host = source
    dst = _guarded(CHUNK)
    r, w = os.pipe()
    t = _feed(w, _frame(host[: CHUNK + 1]))
    try:
        report = probe.stream_fd_to_device(r, dst.data_ptr(), CHUNK, CHUNK, 5000)
    finally:
        os.close(r)
        t.join()
    assert report["rc"] == probe.H2D_FAILED_STREAM, report
    assert dst.cpu().numpy().tobytes() == b"\xa5" * (CHUNK + GUARD), "copied despite the header"


def test_drain_mode_keeps_the_stream_aligned(probe, source):
    _dev, host = source
    n1, n2 = 2 * CHUNK + 17, CHUNK + 1
    dst = _guarded(n2)
    r, w = os.pipe()
    t = _feed(w, _frame(host[:n1]) + _frame(host[n1 : n1 + n2]))
    try:
        drained = probe.stream_fd_to_device(r, 0, n1, CHUNK, 5000)
        second = probe.stream_fd_to_device(r, dst.data_ptr(), n2, CHUNK, 5000)
    finally:
        os.close(r)  # first: a writer still blocked on a full pipe gets EPIPE
        t.join()
    assert drained["rc"] == probe.H2D_OK, drained
    assert second["rc"] == probe.H2D_OK, second
    assert dst.cpu().numpy().tobytes() == host[n1 : n1 + n2] + b"\xa5" * GUARD


# -- csp_checksum_dev --------------------------------------------------------


@pytest.mark.parametrize("n", SUM_SIZES)
def test_checksum_device_matches_reference(probe, source, n):
    dev, host = source
    assert probe.checksum_device(dev.data_ptr(), n) == reference(host[:n])


def test_checksum_device_agrees_with_host_library(probe, source):
    from covalent_ssh_plugin_amd.transport import native_io

    dev, host = source
    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    n = 2 * CHUNK + 17
    assert probe.checksum_device(dev.data_ptr(), n) == native_io.checksum(host[:n])


def test_one_flipped_byte_changes_the_result(probe, source):
    dev, _host = source
    n = 2 * CHUNK + 17
    work = dev[:n].clone()
    torch.cuda.synchronize()
    before = probe.checksum_device(work.data_ptr(), n)
    work[CHUNK + 5] ^= 0x10
    torch.cuda.synchronize()
    after = probe.checksum_device(work.data_ptr(), n)
    assert after[0] != before[0] and after[1] != before[1]


def test_exchanging_two_blocks_changes_s1_only(probe, source):
    dev, host = source
    n = 2 * CHUNK + 17
    a, b = 16 * 3, 16 * 4001
    assert host[a : a + 16] != host[b : b + 16]
    work = dev[:n].clone()
    work[a : a + 16] = dev[b : b + 16]
    work[b : b + 16] = dev[a : a + 16]
    torch.cuda.synchronize()
    before = probe.checksum_device(dev.data_ptr(), n)
    after = probe.checksum_device(work.data_ptr(), n)
    assert after[0] == before[0]
    assert after[1] != before[1]


def test_unaligned_device_pointer_is_refused(probe, source):
    dev, host = source
    with pytest.raises(probe.GpuLibError, match="16-byte aligned"):
        probe.checksum_device(dev.data_ptr() + 4, 1024)
    # nothing was launched, the library is fine
    assert probe.checksum_device(dev.data_ptr(), 1024) == reference(host[:1024])


# -- end to end --------------------------------------------------------------

BIG_BYTES = (3 << 20) + 10  # bf16: an odd number of 2-byte elements' worth


def _arguments(seed):
    gen = torch.Generator().manual_seed(seed)
    return {
        "big_bf16": torch.randn(BIG_BYTES // 2, generator=gen).to(torch.bfloat16),
        "small": torch.randn(1000, generator=gen),
        "transposed": torch.randn(300, 512, generator=gen).t(),
        "empty": torch.empty(0, 7),
        "n": seed,
    }


def _make_electron():
    """A local function, so cloudpickle ships it by value."""

    def electron(d):
        import os

        for key, value in d.items():
            if key != "n":
                assert value.is_cuda, key
        assert d["transposed"].shape == (512, 300)
        return d, os.getpid()

    return electron


_electron = _make_electron()


def _make_executor(kind, tmp_path, sshim, monkeypatch, **overrides):
    from covalent_ssh_plugin_amd import SSHExecutor

    common = dict(
        cache_dir=str(tmp_path / "cache"),
        python_path=sys.executable,
        gpu_slots=max(1, torch.cuda.device_count()),
        persistent_workers=True,
        device_tensor_args=True,
        # one slot, so every electron meets the same warm worker
        hip_visible_devices_policy="fixed",
        fixed_gpu=0,
        pinned_staging_threshold_bytes=1 << 20,
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


def _assert_returned(out, want):
    assert set(out) == set(want)
    assert out["n"] == want["n"]
    for key in ("big_bf16", "small", "transposed", "empty"):
        assert out[key].dtype == want[key].dtype, key
        assert out[key].shape == want[key].shape, key
        assert torch.equal(out[key].cpu(), want[key]), key


@pytest.mark.parametrize("kind", ["local", "sshim"])
def test_end_to_end_device_arguments(kind, tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io
    from covalent_ssh_plugin_amd.transport.channel import Channel

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    # the big tensor comes back through the D2H stream and the native receive
    monkeypatch.setattr(Channel, "large_frame_threshold", 1 << 20)
    ex = _make_executor(kind, tmp_path, sshim, monkeypatch)

    async def run():
        first = await ex.execute(_electron, [_arguments(21)], {}, dispatch_id="a", node_id=0)
        meta1 = ex.last_task_record.remote_meta
        second = await ex.execute(_electron, [_arguments(22)], {}, dispatch_id="a", node_id=1)
        meta2 = ex.last_task_record.remote_meta
        await ex.close_pool()
        return first, meta1, second, meta2

    first, meta1, second, meta2 = asyncio.run(run())
    for (out, pid), meta, seed in ((first, meta1, 21), (second, meta2, 22)):
        want = _arguments(seed)
        _assert_returned(out, want)
        stage = meta["arg_staging"]
        assert stage["mode"] == "pinned-h2d", meta
        assert stage["tensors"] == 4 and stage["verified"] == 4, meta
        assert stage["bytes"] == BIG_BYTES + 4000 + 512 * 300 * 4, meta
        assert pid == meta["pid"]
        assert meta["staging"]["pinned_tensors"] == 1, meta
    assert meta1["pid"] == meta2["pid"], "second electron ran on another worker"
    assert meta2["served"] == meta1["served"] + 1


def test_integrity_failure_then_same_worker(tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    ex = _make_executor("local", tmp_path, sshim, monkeypatch)
    real = native_io.checksum

    def off_by_one(*args, **kwargs):
        s0, s1 = real(*args, **kwargs)
        return s0, (s1 + 1) % (1 << 64)

    async def run():
        (_, pid0) = await ex.execute(_electron, [_arguments(31)], {}, dispatch_id="i", node_id=0)
        with monkeypatch.context() as patch:
            patch.setattr(native_io, "checksum", off_by_one)
            with pytest.raises(RuntimeError, match="integrity") as failure:
                await ex.execute(_electron, [_arguments(32)], {}, dispatch_id="i", node_id=1)
        bad_meta = ex.last_task_record.remote_meta
        out, pid2 = await ex.execute(_electron, [_arguments(33)], {}, dispatch_id="i", node_id=2)
        good_meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return pid0, str(failure.value), bad_meta, out, pid2, good_meta

    pid0, message, bad_meta, out, pid2, good_meta = asyncio.run(run())
    assert "argument buffer 0" in message, message
    assert "user_fn" not in bad_meta["phases_ms"], "user code ran on bad data"
    assert bad_meta["pid"] == pid0 == pid2 == good_meta["pid"]
    _assert_returned(out, _arguments(33))
    assert good_meta["arg_staging"]["verified"] == 4
    assert good_meta["served"] == bad_meta["served"] + 1


def test_isolated_worker_moves_arguments_in_the_child(tmp_path, sshim, monkeypatch):
    from covalent_ssh_plugin_amd.transport import native_io

    assert native_io.load() is not None, "libcsp_io.so was not built/shipped"
    ex = _make_executor(
        "local", tmp_path, sshim, monkeypatch,
        persistent_workers=False, isolate_tasks=True, isolate_preload="torch",
    )

    async def run():
        out = await ex.execute(_electron, [_arguments(41)], {}, dispatch_id="z", node_id=0)
        meta = ex.last_task_record.remote_meta
        await ex.close_pool()
        return out, meta

    (out, pid), meta = asyncio.run(run())
    _assert_returned(out, _arguments(41))
    assert meta["isolated"] is True
    assert meta["pid"] == pid
    assert meta["arg_staging"]["mode"] == "isolated-copy", meta
    assert meta["arg_staging"]["verified"] == 4, meta
